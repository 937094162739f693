"""Training entry point of MODEL.NAME pose_hrnet_hamburger (HamNet), with tools/train.py's flags:

    python tools/train_hamburger.py --cfg experiments/RHD/RHD_HRNet_w32_Hamburger_v2.yaml [KEY value ...]

tools/train.py refuses the model; this tool builds it with trainable=True (models.pose_hrnet_hamburger: the frozen backbone
under no_grad, the head under autograd through hipnet.burger_train and hipnet.nmf_train - the one-step ham gradient, the
BatchNorms on batch statistics, Dropout2d) and runs tools/train_swin.py's loop on it: criterion dict of build_criterion ->
the torch optimiser of utils.get_optimizer (the head's gradients are autograd .grad tensors; the yaml asks for SGD, lr
0.009) -> the learning-rate schedule -> core.function.train / validate per epoch (validation under no_grad, on the
inference path, with the running statistics training left) -> checkpoint.pth.tar / model_best.pth.tar /
final_state.pth.tar with the reference's keys: tools/evaluate_2D.py --model_path loads final_state.pth.tar with the same
yaml. One process, one GPU. Data as tools/train.py: the RHD reader when <DATA_DIR>/RHD/<subset>/anno_<subset>.pickle
exists, otherwise the synthetic RHD-shaped loader (8 batches, validation 2, unless --batches-per-epoch is given).

TRAIN.LR_SCHEDULE: `warmup` is warmup_factor below, the reference's get_linear_schedule_with_warmup (lib/utils/utils.py:
95-105) stepped once per EPOCH with (WARMUP_EPOCHS, END_EPOCH - BEGIN_EPOCH), as its tools/train.py:304-310 and :349 do; the
scheduler is built with last_epoch = BEGIN_EPOCH and steps once when it is built, so epoch e trains at factor(e + 1).
`multi_step` is MultiStepLR(LR_STEP, LR_FACTOR) as in tools/train_swin.py.
"""
import os
import pprint

import _init_paths  # noqa: F401
import torch

from config import cfg, update_config
from core.function import train, validate
from dataset.build import make_dataloader
from models import pose_hrnet_hamburger
from train import build_criterion, parse_args
from utils.utils import create_logger, get_optimizer, save_checkpoint


def warmup_factor(step, warmup, total):
    """the reference's lr_lambda (lib/utils/utils.py:100-103): step / max(1, warmup) up to and including `warmup`, then
    max(0.5, total - step) / max(1, total - warmup) - the floor of 0.5 is on the numerator"""
    if step <= warmup:
        return float(step) / float(max(1, warmup))
    return max(0.5, float(total - step)) / float(max(1, total - warmup))


def lr_at(cfg, epoch):
    """the learning rate of `epoch` (counted from 0)"""
    T = cfg.TRAIN
    if T.LR_SCHEDULE == 'warmup':
        return T.LR * warmup_factor(epoch + 1, int(T.WARMUP_EPOCHS), int(T.END_EPOCH) - int(T.BEGIN_EPOCH))
    if T.LR_SCHEDULE == 'multi_step':
        return T.LR * (T.LR_FACTOR ** sum(epoch >= s for s in T.LR_STEP))
    raise ValueError('TRAIN.LR_SCHEDULE {!r}: expected \'warmup\' or \'multi_step\''.format(T.LR_SCHEDULE))


def check_config(cfg):
    """what this tool refuses of a config, before any device work"""
    if cfg.MODEL.NAME != 'pose_hrnet_hamburger':
        raise ValueError('MODEL.NAME {}: tools/train_hamburger.py trains pose_hrnet_hamburger; tools/train.py trains the '
                         'other 2-D models'.format(cfg.MODEL.NAME))
    world = int(os.environ.get('WORLD_SIZE', '1'))
    if world > 1:
        raise ValueError('WORLD_SIZE {}: data-parallel training of pose_hrnet_hamburger is not built; run one '
                         'process'.format(world))
    lr_at(cfg, 0)


def main():
    args = parse_args()
    update_config(cfg, args)
    check_config(cfg)
    local = int(os.environ.get('LOCAL_RANK', str(args.local_rank)))
    torch.cuda.set_device(local)
    device = torch.device('cuda', local)
    logger, final_output_dir, tb_log_dir = create_logger(cfg, args.cfg, 'train')
    logger.info(pprint.pformat(vars(args)))

    model = pose_hrnet_hamburger.get_pose_net(cfg, is_train=True, trainable=True)
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

    criterion = build_criterion(cfg, device)
    optimizer = get_optimizer(cfg, model)
    if ckpt is not None and 'optimizer' in ckpt:
        optimizer.load_state_dict(ckpt['optimizer'])
    writer_dict = {'writer': None, 'train_global_steps': 0, 'valid_global_steps': 0}
    if ckpt is not None:
        writer_dict['train_global_steps'] = ckpt.get('train_global_steps', 0)
        writer_dict['valid_global_steps'] = ckpt.get('valid_global_steps', 0)

    synthetic_batches = 8 if args.batches_per_epoch is None else args.batches_per_epoch
    train_loader = make_dataloader(cfg, True, False, synthetic_batches, 0, 1, max_batches=args.batches_per_epoch)
    valid_loader = make_dataloader(cfg, False, False, max(1, synthetic_batches // 4), 0, 1, heatmaps=True)
    for epoch in range(begin_epoch, cfg.TRAIN.END_EPOCH):
        for g in optimizer.param_groups:
            g['lr'] = lr_at(cfg, epoch)
        logger.info('Start training [{}/{}] lr: {:.4e}'.format(epoch, cfg.TRAIN.END_EPOCH - cfg.TRAIN.BEGIN_EPOCH,
                                                               lr_at(cfg, epoch)))
        for loader in train_loader.values():
            loader.sampler.set_epoch(epoch)
        train(cfg, args, True, train_loader, model, criterion, optimizer, epoch, final_output_dir, tb_log_dir,
              writer_dict, logger, fp16=False, device=device)
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
