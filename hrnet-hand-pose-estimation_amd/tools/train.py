"""Training entry point with the reference's flags (tools/train.py:57-92):

    python tools/train.py --cfg experiments/RHD/RHD_HRNet_w32_max_hmloss_v1.yaml [KEY value ...]
    python -m torch.distributed.run --nproc-per-node N --master-addr 127.0.0.1 tools/train.py --cfg ...

cfg -> eval(cfg.MODEL.NAME + '.get_pose_net') -> criterion dict -> optimizer -> MultiStepLR ->
core.function.train / validate per epoch -> checkpoint.pth.tar / model_best.pth.tar /
final_state.pth.tar (tools/train.py:126-405). One process per GPU; multi-GPU = RCCL all-reduce of the
flat gradient overlapped with backward (hipnet.optim.GradSync), not DataParallel. Data: the RHD
reader (dataset/rhd.py) when <DATA_DIR>/RHD/<subset>/anno_<subset>.pickle exists - DATASET.DATASET with TRAIN_SET
for training (shuffled, this rank's share), TEST_DATASET with TEST_SET for validation (every sample, with heat
maps) - or the MHP readers (dataset/mhp.py: MHP_kpt, MHP, and MHP_seq for pose_hrnet_PoseAggr and pose_hrnet_transformer, the latter on one GPU) when
<DATA_DIR>/MHP/annotated_frames exists - otherwise the synthetic RHD-shaped loader (dataset/build.py). --batches-per-epoch caps a real epoch only
when given; the synthetic loader is 8 batches (validation 2) unless it is given.
"""
import argparse
import os
import pprint

import _init_paths  # noqa: F401
import torch

from config import cfg, update_config
from core.function import train, validate
from core.loss import BoneLengthLoss, HeatmapLoss, JointAngleLoss, JointsMSELoss
from dataset.build import make_dataloader
from models import CPM, pose_hrnet, pose_hrnet_PoseAggr, pose_hrnet_hamburger, pose_hrnet_softmax, pose_hrnet_transformer, predrnn, swin_transformer  # noqa: F401  (dispatched by name below)
from utils.utils import create_logger, get_optimizer, save_checkpoint


def parse_args():
    p = argparse.ArgumentParser(description='Train keypoints network')
    p.add_argument('--cfg', help='experiment configure file name', required=True, type=str)
    p.add_argument('opts', help='Modify config options using the command-line', default=None, nargs=argparse.REMAINDER)
    p.add_argument('--gpus', help='gpus id for multiprocessing training', type=str)
    p.add_argument('--world-size', default=1, type=int)
    p.add_argument('--dist-url', default='tcp://127.0.0.1:23456', type=str)
    p.add_argument('--rank', default=0, type=int)
    p.add_argument('--local_rank', default=0, type=int)
    p.add_argument('--batches-per-epoch', default=None, type=int,
                   help='batches per training epoch (synthetic loader: default 8; a real dataset: every batch)')
    return p.parse_args()


def build_criterion(cfg, device=None):
    """the loss modules the LOSS.WITH_* flags ask for, keyed as core.function.AverageMeter expects them (reference
    tools/train.py:256-265); the modules hold no parameters, so `device` None leaves them where they are. The 'bone_loss' / 'jointangle_loss'
    entries SELECT the terms that AverageMeter.computeLosses evaluates in one fused launch (core.loss.structure_losses);
    the module objects under those two keys are not called by the loop - they are there for direct use"""
    criterion = {}
    if cfg.LOSS.WITH_HEATMAP_LOSS:
        criterion['heatmap_loss'] = HeatmapLoss()
    if cfg.LOSS.WITH_POSE2D_LOSS:
        criterion['pose2d_loss'] = JointsMSELoss()
    if cfg.LOSS.WITH_BONE_LOSS:
        criterion['bone_loss'] = BoneLengthLoss()
    if cfg.LOSS.WITH_JOINTANGLE_LOSS:
        criterion['jointangle_loss'] = JointAngleLoss()
    return criterion if device is None else {k: m.to(device) for k, m in criterion.items()}


def check_config(cfg):
    """what this tool refuses of a config, before any device work"""
    if cfg.MODEL.NAME == 'swin_transformer':
        raise ValueError('MODEL.NAME swin_transformer: {} (no backward kernels, no stochastic depth); evaluation works: '
                         'tools/evaluate_2D.py and tools/inference.py run it'.format(swin_transformer.NOT_BUILT))
    if cfg.MODEL.NAME == 'pose_hrnet_hamburger':
        raise ValueError('MODEL.NAME pose_hrnet_hamburger: {} (no SyncBN batch statistics, no backward through the NMF, no '
                         'Dropout2d); evaluation works: tools/evaluate_2D.py and tools/inference.py run it'.format(
                             pose_hrnet_hamburger.NOT_BUILT))
    if cfg.MODEL.NAME == 'CPM':
        raise ValueError('MODEL.NAME CPM: {} (no backward of the K x K convolution and the pools, no six-stage heat-map '
                         'loss, no training transforms in MHP_CPM_kpt); evaluation works: tools/evaluate_2D.py runs '
                         'it'.format(CPM.NOT_BUILT))
    if cfg.MODEL.NAME == 'predrnn':
        raise ValueError('MODEL.NAME predrnn: {} (no backward through the L x layers spatio-temporal LSTM cells, no 3-D '
                         'pose loss on frame windows); inference works: tools/evaluate_predrnn.py runs it'.format(
                             predrnn.NOT_BUILT))


def main():
    args = parse_args()
    update_config(cfg, args)
    check_config(cfg)
    world = int(os.environ.get('WORLD_SIZE', '1'))
    rank = int(os.environ.get('RANK', '0'))
    local = int(os.environ.get('LOCAL_RANK', str(args.local_rank)))
    torch.cuda.set_device(local)
    device = torch.device('cuda', local)
    if world > 1 and cfg.MODEL.NAME == 'pose_hrnet_transformer':
        # the gradient exchange (hipnet.optim.GradSync) covers the backbone's flat gradient buffer, not the autograd
        # .grad tensors of the transformer head
        raise ValueError('WORLD_SIZE {}: data-parallel training of pose_hrnet_transformer is not built; run one '
                         'process'.format(world))
    if world > 1:
        torch.distributed.init_process_group(backend=cfg.DIST_BACKEND, device_id=device)
    master = rank == 0
    logger, final_output_dir, tb_log_dir = create_logger(cfg, args.cfg, 'train')
    if master:
        logger.info(pprint.pformat(vars(args)))

    model = eval(cfg.MODEL.NAME + '.get_pose_net')(cfg, is_train=True)
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
    sync = None
    if world > 1:
        from hipnet.optim import GradSync
        sync = GradSync(model)        # broadcasts rank 0's parameters / buffers, as DDP's constructor does

    criterion = build_criterion(cfg, device)
    optimizer = get_optimizer(cfg, model)
    if sync is not None:
        sync.attach(optimizer)        # 1/world: folded into FlatAdam, applied in finish() for torch optimizers
    if ckpt is not None and 'optimizer' in ckpt:
        optimizer.load_state_dict(ckpt['optimizer'])
    writer_dict = {'writer': None, 'train_global_steps': 0, 'valid_global_steps': 0}
    if ckpt is not None:
        writer_dict['train_global_steps'] = ckpt.get('train_global_steps', 0)
        writer_dict['valid_global_steps'] = ckpt.get('valid_global_steps', 0)

    def lr_at(epoch):
        return cfg.TRAIN.LR * (cfg.TRAIN.LR_FACTOR ** sum(epoch >= s for s in cfg.TRAIN.LR_STEP))

    synthetic_batches = 8 if args.batches_per_epoch is None else args.batches_per_epoch
    train_loader = make_dataloader(cfg, True, world > 1, synthetic_batches, rank, world,
                                   max_batches=args.batches_per_epoch)
    valid_loader = make_dataloader(cfg, False, world > 1, max(1, synthetic_batches // 4), rank, world, heatmaps=True)
    for epoch in range(begin_epoch, cfg.TRAIN.END_EPOCH):
        for g in optimizer.param_groups:          # MultiStepLR(LR_STEP, LR_FACTOR)
            g['lr'] = lr_at(epoch)
        for loader in train_loader.values():
            loader.sampler.set_epoch(epoch)
        train(cfg, args, master, train_loader, model, criterion, optimizer, epoch, final_output_dir, tb_log_dir,
              writer_dict, logger, fp16=cfg.FP16.ENABLED, device=device)
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
