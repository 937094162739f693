"""Training of the cross-view fusion model (MODEL.NAME `multiview_pose_hrnet`) on MHP multi-view frames, with
tools/train3D.py's flags (reference tools/train.py with lib/models/multiview_pose_hrnet.py and the MHP_mv branch of
lib/core/function.py:195-276):

    python tools/train_fusion.py --cfg experiments/MHP/MHP_HRNet_w32_fusion_v1.yaml
        [--views '[1,2,3,4]'] [--model_path <2-D checkpoint>] [--batches-per-epoch N] [KEY value ...]

Per batch of B frames and V views (core/function_fusion.py): the backbone once on the B * V images, the fusion layer (ONE
hrnet_view_fusion launch; its backward one hrnet_view_fusion_bwd call), then LOSS.HEATMAP_LOSS_FACTOR * HeatmapLoss and /
or LOSS.POSE2D_LOSS_FACTOR * JointsMSELoss on the concatenation [single; fused] against the targets repeated twice.
TRAIN.IMAGES_PER_GPU counts multi-view frames. Validation reports the mean 2-D end-point error of the single-view maps
and of the fused maps separately.

The optimiser is torch.optim.Adam with two groups and no weight decay: the backbone's trainable parameters (stage4 and
the head; the rest is frozen) and the fusion layer, both at TRAIN.LR, each stepped by TRAIN.LR_FACTOR at TRAIN.LR_STEP.
Checkpoints and AUTO_RESUME are tools/train_vol.py's: checkpoint.pth.tar / model_best.pth.tar every epoch,
final_state.pth.tar (the whole model's state_dict, which `tools/evaluate_3D.py --model_path` reads) at the end.

--model_path (or MODEL.BACKBONE_MODEL_PATH) names a 2-D backbone checkpoint: loaded non-strictly into the backbone, the
`module.` prefix stripped, as the reference does; a checkpoint.pth.tar of this run found by AUTO_RESUME takes precedence.

Refused before any device work (check_config): a MODEL.NAME other than multiview_pose_hrnet; a dataset other than
MHP_mv; a MODEL.HEATMAP_SIZE that is not square or not MODEL.IMAGE_SIZE / 4; another BACKBONE_NAME; MODEL.AGGRE false
(there is then no fusion layer to train: tools/train.py trains the backbone alone); both loss flags off; WORLD_SIZE > 1
(data-parallel training of this model is not built); a missing <DATA_DIR>/MHP/annotated_frames.
"""
import os
import pprint

import _init_paths  # noqa: F401
import torch

from config import cfg, update_config
from core.function_fusion import DATASETS, train, validate
from core.loss import HeatmapLoss, JointsMSELoss
from dataset import mhp
from models.multiview_pose_hrnet import MultiViewPoseNet, check_fusion_config
from train3D import parse_args, parse_views          # one set of flags and one rule for --views in the 3-D tools
from utils.utils import create_logger, save_checkpoint

MODEL_NAME = 'multiview_pose_hrnet'
GROUPS = (('backbone', 'LR'), ('aggre_layer', 'LR'))


def check_config(config, world=1):
    """everything this tool refuses, checked before any device work; raises ValueError"""
    if config.MODEL.NAME != MODEL_NAME:
        raise ValueError('MODEL.NAME {!r}: tools/train_fusion.py trains the cross-view fusion model, MODEL.NAME '
                         '{!r}'.format(config.MODEL.NAME, MODEL_NAME))
    for key, names in (('DATASET.DATASET', config.DATASET.DATASET), ('DATASET.TEST_DATASET',
                                                                     config.DATASET.TEST_DATASET)):
        if not names or any(n not in DATASETS for n in names):
            raise ValueError('{} {}: the fusion model trains and validates on the multi-view reader {}'.format(
                key, list(names), list(DATASETS)))
    check_fusion_config(config)
    if not config.MODEL.AGGRE:
        raise ValueError('MODEL.AGGRE false: there is no fusion layer to train (tools/train.py trains the 2-D backbone '
                         'alone)')
    if not (config.LOSS.WITH_HEATMAP_LOSS or config.LOSS.WITH_POSE2D_LOSS):
        raise ValueError('LOSS.WITH_HEATMAP_LOSS and LOSS.WITH_POSE2D_LOSS are both false: nothing to train on')
    if world > 1:
        raise ValueError('WORLD_SIZE {}: data-parallel training of the fusion model is not built; run one '
                         'process'.format(world))
    frames = mhp.frames_dir(config.DATA_DIR)
    if not os.path.isdir(frames):
        raise ValueError('{} not found: the fusion model trains on the MHP multi-view frames (DATA_DIR/MHP/'
                         'annotated_frames); there is no synthetic multi-view loader'.format(frames))


def build_criterion(config):
    """the loss modules of core.function_fusion.AverageMeterFusion, keyed as it expects them"""
    criterion = {}
    if config.LOSS.WITH_HEATMAP_LOSS:
        criterion['heatmap_loss'] = HeatmapLoss()
    if config.LOSS.WITH_POSE2D_LOSS:
        criterion['pose2d_loss'] = JointsMSELoss()
    return criterion


def build_optimizer(config, model):
    """torch.optim.Adam over two groups, no weight decay: the backbone's parameters that require a gradient and the
    fusion layer, each at its own rate (kept as `initial_lr`)"""
    groups = []
    for child, key in GROUPS:
        params = [p for p in getattr(model, child).parameters() if p.requires_grad]
        lr = getattr(config.TRAIN, key)
        groups.append({'params': params, 'lr': lr, 'initial_lr': lr, 'name': child})
    return torch.optim.Adam(groups, lr=config.TRAIN.LR)


def lr_factor(config, epoch):
    return config.TRAIN.LR_FACTOR ** sum(epoch >= s for s in config.TRAIN.LR_STEP)


def main(argv=None):
    args = parse_args(argv)
    update_config(cfg, args)
    views = parse_views(args.views)
    world = int(os.environ.get('WORLD_SIZE', '1'))
    check_config(cfg, world)
    start = args.model_path or cfg.MODEL.BACKBONE_MODEL_PATH
    if start and not os.path.isfile(start):
        raise ValueError('--model_path / MODEL.BACKBONE_MODEL_PATH {}: no such file'.format(start))
    local = int(os.environ.get('LOCAL_RANK', str(args.local_rank)))
    torch.cuda.set_device(local)
    device = torch.device('cuda', local)
    logger, final_output_dir, tb_log_dir = create_logger(cfg, args.cfg, 'train')
    logger.info(pprint.pformat(vars(args)))

    c = cfg.clone()
    c.defrost()
    c.MODEL.BACKBONE_MODEL_PATH = start
    c.freeze()
    model = MultiViewPoseNet(c)
    best_perf, begin_epoch = float('inf'), cfg.TRAIN.BEGIN_EPOCH
    ckpt_file = os.path.join(final_output_dir, 'checkpoint.pth.tar')
    ckpt = None
    if cfg.AUTO_RESUME and os.path.exists(ckpt_file):
        ckpt = torch.load(ckpt_file, map_location='cpu')
        sd = {k[7:] if k.startswith('module.') else k: v for k, v in ckpt['state_dict'].items()}
        model.load_state_dict(sd, strict=True)
        begin_epoch, best_perf = ckpt['epoch'], ckpt.get('loss', best_perf)
        logger.info('=> resumed from {} (epoch {})'.format(ckpt_file, begin_epoch))
    model = model.to(device)

    criterion = build_criterion(cfg)
    optimizer = build_optimizer(cfg, model)
    if ckpt is not None and 'optimizer' in ckpt:
        optimizer.load_state_dict(ckpt['optimizer'])
    writer_dict = {'writer': None, 'train_global_steps': 0, 'valid_global_steps': 0}
    if ckpt is not None:
        writer_dict['train_global_steps'] = ckpt.get('train_global_steps', 0)
        writer_dict['valid_global_steps'] = ckpt.get('valid_global_steps', 0)

    heatmaps = bool(cfg.LOSS.WITH_HEATMAP_LOSS)
    train_loader = {n: mhp.make_loader(cfg, n, cfg.DATASET.TRAIN_SET, True, 0, 1, False, args.batches_per_epoch,
                                       heatmaps, views=views) for n in cfg.DATASET.DATASET}
    valid_loader = {n: mhp.make_loader(cfg, n, cfg.DATASET.TEST_SET, False, heatmaps=heatmaps, views=views)
                    for n in cfg.DATASET.TEST_DATASET}
    for epoch in range(begin_epoch, cfg.TRAIN.END_EPOCH):
        for g in optimizer.param_groups:          # MultiStepLR(LR_STEP, LR_FACTOR), each group from its own rate
            g['lr'] = g['initial_lr'] * lr_factor(cfg, epoch)
        for loader in train_loader.values():
            loader.sampler.set_epoch(epoch)
        train(cfg, args, True, train_loader, model, criterion, optimizer, epoch, final_output_dir, tb_log_dir,
              writer_dict, logger, device=device)
        perf = best_perf
        if not cfg.WITHOUT_EVAL:
            recorder = validate(cfg, args, True, valid_loader, model, criterion, final_output_dir, tb_log_dir,
                                writer_dict, logger, device=device)
            perf = recorder.avg_total_loss
        is_best = perf < best_perf
        best_perf = min(best_perf, perf)
        logger.info('=> saving checkpoint to {} (best: {})'.format(final_output_dir, is_best))
        save_checkpoint({'epoch': epoch + 1, 'model': cfg.MODEL.NAME, 'state_dict': model.state_dict(),
                         'loss': perf, 'optimizer': optimizer.state_dict(),
                         'train_global_steps': writer_dict['train_global_steps'],
                         'valid_global_steps': writer_dict['valid_global_steps']}, is_best, final_output_dir)
    final = os.path.join(final_output_dir, 'final_state.pth.tar')
    logger.info('saving final model state to {}'.format(final))
    torch.save(model.state_dict(), final)


if __name__ == '__main__':
    main()
