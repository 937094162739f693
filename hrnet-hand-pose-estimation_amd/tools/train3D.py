"""3-D-loss training on MHP multi-view frames, with tools/train.py's flags (reference tools/train3D.py with
AlgebraicTriangulationNet, lib/models/triangulation.py):

    python tools/train3D.py --cfg experiments/MHP/MHP_HRNet_w32_trainable_softmax_pose3dloss_v1.yaml
        [--views '[1,2,3,4]'] [--model_path <2-D checkpoint>] [--batches-per-epoch N] [KEY value ...]

The 2-D backbone pose_hrnet_softmax is fine-tuned end to end on the error of the triangulated joints: per batch of B
frames and V views, model -> expectation decode -> ONE differentiable hrnet_triangulate launch through the batch's
`hm_inverse` -> Joints3DMSELoss against the world joints (core/function3D.py; the backward of the lifting is one
hrnet_triangulate_bwd launch). LOSS.WITH_HEATMAP_LOSS / WITH_POSE2D_LOSS add the 2-D terms on the same predictions.
TRAIN.IMAGES_PER_GPU counts multi-view frames: the model sees B * V images per step. Checkpoints, optimiser,
LR steps, AUTO_RESUME and the multi-GPU plumbing are tools/train.py's; the saved state_dict is the backbone's own, so
`tools/evaluate_3D.py --model_path <final_state.pth.tar>` reads it unchanged and reports the trained quantity.

--model_path (or MODEL.BACKBONE_MODEL_PATH) starts from a 2-D checkpoint: a strict load, the `module.` prefix stripped;
a checkpoint.pth.tar of this run found by AUTO_RESUME takes precedence.

Refused with a ValueError before any device work: a MODEL.NAME other than pose_hrnet_softmax; MODEL.HEATMAP_SOFTMAX
false (the arg-max decode has no gradient); MODEL.ALG_CONFIDENCES true (the confidence head of
pose_hrnet_volumetric is not built); a dataset other than MHP_mv; LOSS.WITH_POSE3D_LOSS false and the loss terms this
loop does not evaluate; a missing <DATA_DIR>/MHP/annotated_frames (there is no synthetic multi-view loader).

Deviations from the reference: every parameter trains (the reference freezes the backbone below stage4); the points go
through each image's `hm_inverse`, not 640/64 and 480/64; there is no confidence head.
"""
import argparse
import os
import pprint

import _init_paths  # noqa: F401
import torch

from config import cfg, update_config
from core.evaluate2d import load_checkpoint_state
from core.function3D import DATASETS, train, validate
from core.loss import HeatmapLoss, Joints3DMSELoss, JointsMSELoss
from dataset import mhp
from evaluate_3D import parse_views          # one rule for --views in both tools
from models import pose_hrnet_softmax
from utils.utils import create_logger, get_optimizer, save_checkpoint

MODEL_NAME = 'pose_hrnet_softmax'
UNUSED_TERMS = ('WITH_BONE_LOSS', 'WITH_JOINTANGLE_LOSS', 'WITH_TIME_CONSISTENCY_LOSS', 'WITH_VOLUMETRIC_CE_LOSS',
                'WITH_KCS_LOSS', 'WITH_KCS_TC_LOSS')


def parse_args(argv=None):
    p = argparse.ArgumentParser(description='Train keypoints network on the 3-D loss')
    p.add_argument('--cfg', help='experiment configure file name', required=True, type=str)
    p.add_argument('opts', help='Modify config options using the command-line', default=None, nargs=argparse.REMAINDER)
    p.add_argument('--gpus', help='gpus id for multiprocessing training', type=str)
    p.add_argument('--world-size', default=1, type=int)
    p.add_argument('--dist-url', default='tcp://127.0.0.1:23456', type=str)
    p.add_argument('--rank', default=0, type=int)
    p.add_argument('--local_rank', default=0, type=int)
    p.add_argument('--batches-per-epoch', default=None, type=int, help='batches per training epoch (default: all)')
    p.add_argument('--views', default='[1,2,3,4]', type=str, help="cameras to triangulate from, e.g. '[1,2,3,4]'")
    p.add_argument('--model_path', default='', type=str,
                   help='2-D checkpoint to start from (default: MODEL.BACKBONE_MODEL_PATH)')
    return p.parse_args(argv)


def check_config(config):
    """everything this tool refuses, checked before any device work; raises ValueError"""
    if config.MODEL.NAME != MODEL_NAME:
        raise ValueError('MODEL.NAME {!r}: tools/train3D.py trains {} on the 3-D loss (the volumetric and triangulation '
                         'model families are not built in this project)'.format(config.MODEL.NAME, MODEL_NAME))
    if not config.MODEL.HEATMAP_SOFTMAX:
        raise ValueError('MODEL.HEATMAP_SOFTMAX false: the arg-max decode has no gradient, the 3-D loss needs the '
                         'expectation decode (set MODEL.HEATMAP_SOFTMAX true)')
    if config.MODEL.ALG_CONFIDENCES:
        raise ValueError('MODEL.ALG_CONFIDENCES true: the confidence head of pose_hrnet_volumetric is not built in '
                         'this project; every view is triangulated with weight 1 (set MODEL.ALG_CONFIDENCES false)')
    for key, names in (('DATASET.DATASET', config.DATASET.DATASET), ('DATASET.TEST_DATASET',
                                                                     config.DATASET.TEST_DATASET)):
        if not names or any(n not in DATASETS for n in names):
            raise ValueError('{} {}: the 3-D loss trains and validates on the multi-view reader {}'.format(
                key, list(names), list(DATASETS)))
    if not config.LOSS.WITH_POSE3D_LOSS:
        raise ValueError('LOSS.WITH_POSE3D_LOSS false: tools/train3D.py trains the 3-D loss; tools/train.py trains the '
                         '2-D terms alone')
    on = [k for k in UNUSED_TERMS if getattr(config.LOSS, k)]
    if on:
        raise ValueError('LOSS.{} true: the 3-D loop evaluates the pose3d, heat-map and pose2d terms only'.format(on[0]))
    frames = mhp.frames_dir(config.DATA_DIR)
    if not os.path.isdir(frames):
        raise ValueError('{} not found: the 3-D loss trains on the MHP multi-view frames (DATA_DIR/MHP/'
                         'annotated_frames); there is no synthetic multi-view loader'.format(frames))


def build_criterion(config):
    """the loss modules of core.function3D.AverageMeter3D, keyed as it expects them"""
    criterion = {'pose3d_loss': Joints3DMSELoss()}
    if config.LOSS.WITH_HEATMAP_LOSS:
        criterion['heatmap_loss'] = HeatmapLoss()
    if config.LOSS.WITH_POSE2D_LOSS:
        criterion['pose2d_loss'] = JointsMSELoss()
    return criterion


def main(argv=None):
    args = parse_args(argv)
    update_config(cfg, args)
    views = parse_views(args.views)
    check_config(cfg)
    start = args.model_path or cfg.MODEL.BACKBONE_MODEL_PATH
    if start and not os.path.isfile(start):
        raise ValueError('--model_path / MODEL.BACKBONE_MODEL_PATH {}: no such file'.format(start))
    world = int(os.environ.get('WORLD_SIZE', '1'))
    rank = int(os.environ.get('RANK', '0'))
    local = int(os.environ.get('LOCAL_RANK', str(args.local_rank)))
    torch.cuda.set_device(local)
    device = torch.device('cuda', local)
    if world > 1:
        torch.distributed.init_process_group(backend=cfg.DIST_BACKEND, device_id=device)
    master = rank == 0
    logger, final_output_dir, tb_log_dir = create_logger(cfg, args.cfg, 'train')
    if master:
        logger.info(pprint.pformat(vars(args)))

    model = pose_hrnet_softmax.get_pose_net(cfg, is_train=True)
    best_perf, begin_epoch = float('inf'), cfg.TRAIN.BEGIN_EPOCH
    ckpt_file = os.path.join(final_output_dir, 'checkpoint.pth.tar')
    ckpt = None
    if cfg.AUTO_RESUME and os.path.exists(ckpt_file):
        ckpt = torch.load(ckpt_file, map_location='cpu')
        sd = {k[7:] if k.startswith('module.') else k: v for k, v in ckpt['state_dict'].items()}
        model.load_state_dict(sd, strict=True)
        begin_epoch, best_perf = ckpt['epoch'], ckpt.get('loss', best_perf)
        logger.info('=> resumed from {} (epoch {})'.format(ckpt_file, begin_epoch))
    elif start:
        load_checkpoint_state(model, start)                # strict, `module.` stripped
        logger.info('=> backbone weights from {}'.format(start))
    model = model.to(device)
    sync = None
    if world > 1:
        from hipnet.optim import GradSync
        sync = GradSync(model)        # broadcasts rank 0's parameters / buffers, as DDP's constructor does

    criterion = build_criterion(cfg)
    optimizer = get_optimizer(cfg, model)
    if sync is not None:
        sync.attach(optimizer)
    if ckpt is not None and 'optimizer' in ckpt:
        optimizer.load_state_dict(ckpt['optimizer'])
    writer_dict = {'writer': None, 'train_global_steps': 0, 'valid_global_steps': 0}
    if ckpt is not None:
        writer_dict['train_global_steps'] = ckpt.get('train_global_steps', 0)
        writer_dict['valid_global_steps'] = ckpt.get('valid_global_steps', 0)

    def lr_at(epoch):
        return cfg.TRAIN.LR * (cfg.TRAIN.LR_FACTOR ** sum(epoch >= s for s in cfg.TRAIN.LR_STEP))

    heatmaps = bool(cfg.LOSS.WITH_HEATMAP_LOSS)
    train_loader = {n: mhp.make_loader(cfg, n, cfg.DATASET.TRAIN_SET, True, rank, world, world > 1,
                                       args.batches_per_epoch, heatmaps, views=views) for n in cfg.DATASET.DATASET}
    valid_loader = {n: mhp.make_loader(cfg, n, cfg.DATASET.TEST_SET, False, heatmaps=heatmaps, views=views)
                    for n in cfg.DATASET.TEST_DATASET}
    for epoch in range(begin_epoch, cfg.TRAIN.END_EPOCH):
        for g in optimizer.param_groups:          # MultiStepLR(LR_STEP, LR_FACTOR)
            g['lr'] = lr_at(epoch)
        for loader in train_loader.values():
            loader.sampler.set_epoch(epoch)
        train(cfg, args, master, train_loader, model, criterion, optimizer, epoch, final_output_dir, tb_log_dir,
              writer_dict, logger, device=device)
        perf = best_perf
        if not cfg.WITHOUT_EVAL:
            recorder = validate(cfg, args, master, valid_loader, model, criterion, final_output_dir, tb_log_dir,
                                writer_dict, logger, device=device)
            perf = recorder.avg_total_loss
        is_best = perf < best_perf
        best_perf = min(best_perf, perf)
        if master:
            logger.info('=> saving checkpoint to {} (best: {})'.format(final_output_dir, is_best))
            save_checkpoint({'epoch': epoch + 1, 'model': cfg.MODEL.NAME, 'state_dict': model.state_dict(),
                             'loss': perf, 'optimizer': optimizer.state_dict(),
                             'train_global_steps': writer_dict['train_global_steps'],
                             'valid_global_steps': writer_dict['valid_global_steps']}, is_best, final_output_dir)
    if master:
        final = os.path.join(final_output_dir, 'final_state.pth.tar')
        logger.info('saving final model state to {}'.format(final))
        torch.save(model.state_dict(), final)
    if world > 1:
        torch.distributed.destroy_process_group()


if __name__ == '__main__':
    main()
