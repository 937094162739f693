"""Training of the volumetric triangulation model (MODEL.NAME `vol`) on MHP multi-view frames, with tools/train3D.py's
flags (reference tools/train3D.py with VolumetricTriangulationNet, lib/models/triangulation.py:277-470):

    python tools/train_vol.py --cfg experiments/MHP/MHP_VolTriangulation_w32_v1.yaml
        [--views '[1,2,3,4]'] [--model_path <2-D checkpoint>] [--batches-per-epoch N] [KEY value ...]

Per batch of B frames and V views (core/function_vol.py): projection matrices from world coordinates to heat-map pixels,
the model (backbone -> base point -> process_features -> unprojection -> V2V -> 3-D soft-argmax, all on HIP kernels),
then LOSS.POSE3D_LOSS_FACTOR * Joints3DMSELoss + LOSS.VOLUMETRIC_LOSS_FACTOR * VolumetricCELoss, plus the heat-map and
pose2d terms when their flags are on. TRAIN.IMAGES_PER_GPU counts multi-view frames.

The optimiser is torch.optim.Adam with three groups and no weight decay, as the reference builds it
(tools/train3D.py:190-197): the backbone's trainable parameters (stage4 and the head; the rest is frozen) at TRAIN.LR,
process_features at TRAIN.PROCESS_FEATURE_LR, volume_net at TRAIN.VOLUME_NET_LR. Each group is stepped by
TRAIN.LR_FACTOR at TRAIN.LR_STEP from its own initial rate. Checkpoints and AUTO_RESUME are tools/train3D.py's; the
saved state_dict is the whole model's, which `tools/evaluate_vol.py --model_path <final_state.pth.tar>` reads.

--model_path (or MODEL.BACKBONE_MODEL_PATH) names a 2-D backbone checkpoint: loaded non-strictly into the backbone, the
`module.` prefix stripped, as the reference does; a checkpoint.pth.tar of this run found by AUTO_RESUME takes precedence.

Refused before any device work (check_config): a MODEL.NAME other than vol; what models/triangulation.py refuses (a conf*
aggregation, a VOLUME_SIZE that is no multiple of 32, another BACKBONE_NAME, MODEL.ALG_CONFIDENCES); a dataset other
than MHP_mv; LOSS.WITH_POSE3D_LOSS false and the loss terms this loop does not evaluate; a missing
<DATA_DIR>/MHP/annotated_frames; WORLD_SIZE > 1 (data-parallel training of this model is not built).

MODEL.NAME vol_CPM (experiments/MHP/MHP_VolTriangulation_CPM_v1.yaml) is the same model on the CPM backbone
(VolumetricTriangulationNet_CPM on CPM_volumetric), trained on the reader MHP_CPM_mv, whose batches carry the centre
maps and the k + 1 channel heat-map targets. The three Adam groups are the same; `backbone` then means
Mconv3/4/5_stage6, the only layers of CPM_volumetric that train. It refuses what check_vol_cpm_config refuses
(MODEL.VOL_CONFIDENCES false among it) and any reader but MHP_CPM_mv.
"""
import os
import pprint

import _init_paths  # noqa: F401
import torch

from config import cfg, update_config
from core.function_vol import train, validate
from core.loss import HeatmapLoss, Joints3DMSELoss, JointsMSELoss, VolumetricCELoss
from dataset import mhp
from models.triangulation import (VolumetricTriangulationNet, VolumetricTriangulationNet_CPM, check_vol_config,
                                  check_vol_cpm_config)
from train3D import parse_args, parse_views          # one set of flags and one rule for --views in the 3-D tools
from utils.utils import create_logger, save_checkpoint

MODEL_NAME = 'vol'
# MODEL.NAME -> (the model, what it refuses of a config, the multi-view reader it trains and validates on)
MODELS = {'vol': (VolumetricTriangulationNet, check_vol_config, 'MHP_mv'),
          'vol_CPM': (VolumetricTriangulationNet_CPM, check_vol_cpm_config, 'MHP_CPM_mv')}
UNUSED_TERMS = ('WITH_BONE_LOSS', 'WITH_JOINTANGLE_LOSS', 'WITH_TIME_CONSISTENCY_LOSS', 'WITH_KCS_LOSS',
                'WITH_KCS_TC_LOSS')
GROUPS = (('backbone', 'LR'), ('process_features', 'PROCESS_FEATURE_LR'), ('volume_net', 'VOLUME_NET_LR'))


def check_config(config, world=1):
    """everything this tool refuses, checked before any device work; raises ValueError or NotImplementedError"""
    if config.MODEL.NAME not in MODELS:
        raise ValueError('MODEL.NAME {!r}: tools/train_vol.py trains the volumetric triangulation model, MODEL.NAME '
                         '{!r} (or vol_CPM, the same on the CPM backbone; tools/train3D.py trains pose_hrnet_softmax on '
                         'the 3-D loss)'.format(config.MODEL.NAME, MODEL_NAME))
    _model, check, reader = MODELS[config.MODEL.NAME]
    check(config)
    for key, names in (('DATASET.DATASET', config.DATASET.DATASET), ('DATASET.TEST_DATASET',
                                                                     config.DATASET.TEST_DATASET)):
        if not names or any(n != reader for n in names):
            raise ValueError('{} {}: the volumetric model trains and validates on the multi-view reader {}'.format(
                key, list(names), [reader]))
    if not config.LOSS.WITH_POSE3D_LOSS:
        raise ValueError('LOSS.WITH_POSE3D_LOSS false: tools/train_vol.py trains the 3-D loss of the volumetric model')
    on = [k for k in UNUSED_TERMS if getattr(config.LOSS, k)]
    if on:
        raise ValueError('LOSS.{} true: the volumetric loop evaluates the pose3d, volumetric cross-entropy, heat-map '
                         'and pose2d terms only'.format(on[0]))
    if world > 1:
        raise ValueError('WORLD_SIZE {}: data-parallel training of the volumetric model is not built; run one '
                         'process'.format(world))
    frames = mhp.frames_dir(config.DATA_DIR)
    if not os.path.isdir(frames):
        raise ValueError('{} not found: the volumetric model trains on the MHP multi-view frames (DATA_DIR/MHP/'
                         'annotated_frames); there is no synthetic multi-view loader'.format(frames))


def build_criterion(config):
    """the loss modules of core.function_vol.AverageMeterVol, keyed as it expects them"""
    criterion = {'pose3d_loss': Joints3DMSELoss()}
    if config.LOSS.WITH_VOLUMETRIC_CE_LOSS:
        criterion['volumetric_ce_loss'] = VolumetricCELoss()
    if config.LOSS.WITH_HEATMAP_LOSS:
        criterion['heatmap_loss'] = HeatmapLoss()
    if config.LOSS.WITH_POSE2D_LOSS:
        criterion['pose2d_loss'] = JointsMSELoss()
    return criterion


def build_optimizer(config, model):
    """torch.optim.Adam over three groups, no weight decay (reference tools/train3D.py:190-197): the backbone's
    parameters that require a gradient, process_features, volume_net, each at its own rate (kept as `initial_lr`)"""
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
    model = MODELS[cfg.MODEL.NAME][0](c, is_train=True)
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

    # MHP_CPM_mv carries its own heat maps (k + 1 channels, the background first): the loader generates none
    heatmaps = bool(cfg.LOSS.WITH_HEATMAP_LOSS) and cfg.MODEL.NAME == MODEL_NAME
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
