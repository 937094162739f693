"""Training entry point of MODEL.NAME FTL (FTLMultiviewNet), with tools/train_cpm.py's flags:

    python tools/train_ftl.py --cfg experiments/MHP/MHP_HRNet_w32_softmax_pose2dloss_FTL_v1.yaml [--iterations N]
        [--batches-per-epoch N] [KEY value ...]

tools/train.py and tools/train3D.py refuse the model; this tool builds it with trainable=True (models.FTL_encoder_decoder:
the head on batch statistics as one autograd node on hipnet.ftl_train) and runs the reference's step (tools/train3D.py,
lib/core/function3D.py:135-149): the backbone (MODEL.BACKBONE_MODEL_PATH) is frozen and runs in eval mode under no_grad,
only the head learns. Loss schedule of the reference: epochs 1 .. 20 the 2-D joints loss (JointsMSELoss with visibility)
on pose2d_pred in heat-map pixels; later epochs 0.1 x the same loss plus Joints3DMSELoss on pose3d_pred. Both go through
core.function3D.AverageMeter3D.computeLosses (the first phase with the 3-D factor at 0, so the sums and the log line keep
one layout). Optimizer: hipnet.optim.FlatAdam over the head's parameters only (TRAIN.OPTIMIZER adam, TRAIN.LR, TRAIN.WD,
MultiStepLR(TRAIN.LR_STEP, TRAIN.LR_FACTOR) by epoch, TRAIN.BEGIN_EPOCH .. TRAIN.END_EPOCH). checkpoint.pth.tar per epoch
and final_state.pth.tar - the whole model's state_dict under the reference's keys, which tools/evaluate_ftl.py
--model_path loads strict - go to the run's output directory. One process, one GPU.

Data: the MHP_mv reader on DATASET.TRAIN_SET (four-view frames, evaluation-style resize, fixed order: the reference's
random image transforms are not built for this reader) when <DATA_DIR>/MHP/annotated_frames exists; otherwise synthetic
four-view batches (random images, random cameras around a drawn hand, its projections as targets; 8 per epoch unless
--batches-per-epoch is given), so that the tool runs without a dataset.
"""
import argparse
import logging
import os
import pprint

import _init_paths  # noqa: F401
import numpy as np
import torch

from config import cfg, update_config
from core.function3D import AverageMeter3D
from core.loss import Joints3DMSELoss, JointsMSELoss
from dataset import mhp
from utils.utils import create_logger, save_checkpoint

MODEL_NAME = 'FTL'
PHASE_ONE_EPOCHS = 20            # the reference's `if epoch <= 20`
PHASE_TWO_POSE2D = 0.1

logger = logging.getLogger(__name__)


def parse_args(argv=None):
    p = argparse.ArgumentParser(description='Train the head of FTLMultiviewNet')
    p.add_argument('--cfg', help='experiment configure file name', required=True, type=str)
    p.add_argument('opts', help='Modify config options using the command-line', default=None, nargs=argparse.REMAINDER)
    p.add_argument('--local_rank', default=0, type=int)
    p.add_argument('--iterations', default=None, type=int, help='stop after this many iterations in all')
    p.add_argument('--batches-per-epoch', default=None, type=int,
                   help='batches per epoch (synthetic data: default 8; the MHP reader: every batch)')
    return p.parse_args(argv)


def check_config(config):
    """what this tool refuses of a config, before any device work"""
    from models.FTL_encoder_decoder import check_config as check_ftl_config
    if config.MODEL.NAME != MODEL_NAME:
        raise ValueError('MODEL.NAME {!r}: tools/train_ftl.py trains FTLMultiviewNet, MODEL.NAME {!r}; tools/train.py and '
                         'the other train_*.py tools train the other models'.format(config.MODEL.NAME, MODEL_NAME))
    check_ftl_config(config)
    if list(config.DATASET.DATASET) != ['MHP_mv']:
        raise ValueError('DATASET.DATASET {}: FTL trains on MHP_mv (multi-view frames with cameras)'.format(
            list(config.DATASET.DATASET)))
    if config.TRAIN.OPTIMIZER != 'adam':
        raise ValueError('TRAIN.OPTIMIZER {}: FTL trains with hipnet.optim.FlatAdam (adam)'.format(config.TRAIN.OPTIMIZER))
    world = int(os.environ.get('WORLD_SIZE', '1'))
    if world > 1:
        raise ValueError('WORLD_SIZE {}: data-parallel training of the FTL head is not built; run one process'.format(world))


def lr_at(config, epoch):
    """MultiStepLR by epoch"""
    return config.TRAIN.LR * (config.TRAIN.LR_FACTOR ** sum(epoch >= s for s in config.TRAIN.LR_STEP))


def loss_factors(epoch):
    """(POSE2D_LOSS_FACTOR, POSE3D_LOSS_FACTOR) of an epoch: the reference's schedule"""
    return (1.0, 0.0) if epoch <= PHASE_ONE_EPOCHS else (PHASE_TWO_POSE2D, 1.0)


def _rotation(rng):
    q, r = np.linalg.qr(rng.standard_normal((3, 3)))
    q = q * np.sign(np.diag(r))
    if np.linalg.det(q) < 0:
        q[:, 0] = -q[:, 0]
    return q


def synthetic_batch(config, B, seed):
    """one batch in the MHP_mv reader's layout: a hand of K joints about 600 mm in front of V random cameras that look at
    it, its projections as 2-D targets in heat-map pixels, random images"""
    rng = np.random.RandomState(seed)
    V, K = int(config.DATASET.NUM_VIEWS), int(config.DATASET.NUM_JOINTS)
    W, H = config.MODEL.IMAGE_SIZE
    hw, hh = config.MODEL.HEATMAP_SIZE
    Kmat = np.array([[614.878, 0, 313.219], [0, 615.479, 231.288], [0, 0, 1]])
    fw, fh = 640.0, 480.0
    pose3d = rng.uniform(-60, 60, (B, K, 3))
    ext = np.empty((B, V, 3, 4))
    pose2d = np.empty((B, V, K, 2))
    for b in range(B):
        for v in range(V):
            R = _rotation(rng)
            t = np.array([rng.uniform(-40, 40), rng.uniform(-40, 40), rng.uniform(500, 700)])
            ext[b, v, :, :3], ext[b, v, :, 3] = R, t
            cam = pose3d[b] @ R.T + t
            uv = cam @ Kmat.T
            pose2d[b, v] = uv[:, :2] / uv[:, 2:] * np.array([hw / fw, hh / fh])
    inv = np.array([[fw / hw, 0, 0], [0, fh / hh, 0]])
    f32 = lambda a: torch.tensor(a, dtype=torch.float32)
    return {'imgs': f32(rng.standard_normal((B * V, 3, H, W)) * 0.5), 'extrinsic_matrices': f32(ext),
            'intrinsic_matrix': f32(np.broadcast_to(Kmat, (B, 3, 3)).copy()), 'pose2d': f32(pose2d.reshape(B * V, K, 2)),
            'pose3d': f32(pose3d), 'visibility': torch.ones(B * V, K, 1), 'hm_inverse': f32(np.broadcast_to(inv, (B * V, 2, 3)).copy())}


class SyntheticViews(object):
    def __init__(self, config, batches):
        self.config, self.batches = config, batches

    def __len__(self):
        return self.batches

    def __iter__(self):
        for i in range(self.batches):
            yield synthetic_batch(self.config, int(self.config.TRAIN.IMAGES_PER_GPU), 1234 + i)


def make_loader(config, batches_per_epoch=None):
    frames = mhp.frames_dir(config.DATA_DIR)
    if os.path.isdir(frames):
        c = config.clone()
        c.defrost()
        c.TEST.IMAGES_PER_GPU = config.TRAIN.IMAGES_PER_GPU
        return mhp.make_loader(c, 'MHP_mv', config.DATASET.TRAIN_SET, False, max_batches=batches_per_epoch)
    logger.warning('%s not found: training on synthetic four-view batches', frames)
    return SyntheticViews(config, 8 if batches_per_epoch is None else batches_per_epoch)


def train_step(config, model, optimizer, recorder, ret, epoch, device):
    """one step of the reference's schedule on a batch of the MHP_mv layout; returns computeLosses' dict"""
    V = model.num_views
    imgs = ret['imgs'].to(device, non_blocking=True)
    B = imgs.shape[0] // V
    _, pose2d, pose3d = model(imgs.view(B, V, *imgs.shape[1:]), ret['extrinsic_matrices'].to(device), ret['intrinsic_matrix'],
                              to_frame=ret['hm_inverse'].to(device))
    vis = ret['visibility'].to(device)
    L = recorder.config.LOSS
    L.POSE2D_LOSS_FACTOR, L.POSE3D_LOSS_FACTOR = loss_factors(epoch)
    out = recorder.computeLosses(pose3d, ret['pose3d'].to(device).float(), pose2d_pred=pose2d.reshape(B * V, -1, 2),
                                 pose2d_gt=ret['pose2d'].to(device).float(), visibility=vis.reshape(vis.shape[0], -1))
    optimizer.zero_grad()
    out['total_loss'].backward()
    optimizer.step()
    return out


def make_recorder(config):
    c = config.clone()
    c.defrost()                                  # the factors follow the schedule
    return AverageMeter3D(c, {'pose3d_loss': Joints3DMSELoss(), 'pose2d_loss': JointsMSELoss()})


def save_final_state(model, output_dir):
    """final_state.pth.tar: the whole model's state_dict under the reference's keys (tools/evaluate_ftl.py --model_path)"""
    final = os.path.join(output_dir, 'final_state.pth.tar')
    torch.save({k: v.detach().clone().cpu() for k, v in model.state_dict().items()}, final)
    return final


def main(argv=None):
    global logger
    args = parse_args(argv)
    update_config(cfg, args)
    check_config(cfg)
    from hipnet.optim import FlatAdam
    from models.FTL_encoder_decoder import get_pose_net
    local = int(os.environ.get('LOCAL_RANK', str(args.local_rank)))
    torch.cuda.set_device(local)
    device = torch.device('cuda', local)
    logger, final_output_dir, _ = create_logger(cfg, args.cfg, 'train')
    logger.info(pprint.pformat(vars(args)))

    model = get_pose_net(cfg, is_train=True, trainable=True).to(device).train()
    optimizer = FlatAdam(model, lr=cfg.TRAIN.LR, weight_decay=cfg.TRAIN.WD)
    loader = make_loader(cfg, args.batches_per_epoch)
    recorder = make_recorder(cfg)
    it, done = 0, False
    for epoch in range(cfg.TRAIN.BEGIN_EPOCH, cfg.TRAIN.END_EPOCH):
        for g in optimizer.param_groups:
            g['lr'] = lr_at(cfg, epoch)
        total, count = 0.0, 0
        for i, ret in enumerate(loader):
            out = train_step(cfg, model, optimizer, recorder, ret, epoch, device)
            it += 1
            if i % cfg.PRINT_FREQ == 0:
                value = float(out['total_loss'].detach())
                total, count = total + value, count + 1
                logger.info('Epoch: [{}][{}/{}] iteration {} lr {:.3g} loss {:.6f} pose2d {:.6f} pose3d {:.6f}'.format(
                    epoch, i, len(loader), it, optimizer.param_groups[0]['lr'], value, float(out['pose2d_loss'].detach()),
                    float(out['pose3d_loss'].detach())))
            if args.iterations is not None and it >= args.iterations:
                done = True
                break
        save_checkpoint({'epoch': epoch + 1, 'model': cfg.MODEL.NAME, 'state_dict': model.state_dict(),
                         'loss': total / max(count, 1), 'optimizer': optimizer.state_dict()}, False, final_output_dir)
        if done:
            break
    final = save_final_state(model, final_output_dir)
    logger.info('saved the final model state to {}'.format(final))
    return final


if __name__ == '__main__':
    main()
