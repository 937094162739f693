"""Training entry point of MODEL.NAME CPM (the Convolutional Pose Machine), with tools/train.py's flags:

    python tools/train_cpm.py --cfg experiments/MHP/MHP_CPM_v1.yaml [--iterations N] [KEY value ...]

tools/train.py refuses the model; this tool builds it with trainable=True (models.CPM: the K x K weight and data gradients
and the pool backward on hipnet.conv_kxk_train) and runs the reference's CPM step (lib/core/function.py:29-32): forward,
HeatmapLoss of the LAST stage's maps against the batch's heat maps (models.CPM.cpm_loss; TRAIN.CPM_STAGE_WEIGHTS adds the
other stages), backward, hipnet.optim.FlatAdam (the yaml's adam, TRAIN.LR 1e-4, MultiStepLR(LR_STEP, LR_FACTOR)). The loss
is logged every PRINT_FREQ iterations; checkpoint.pth.tar per epoch and final_state.pth.tar (the reference's 80 keys:
tools/evaluate_2D.py --model_path loads it strict) go to the run's output directory. One process, one GPU.

DEVIATION from the reference: the training frames are DATASET.TRAIN_SET read through MHP_CPM_kpt(..., is_train=False),
i.e. resized and normalised as for evaluation, in a fixed order. The reference's random transforms of the training reader
are not built (MHP_CPM_kpt refuses is_train=True), so this tool trains without augmentation and without shuffling.
"""
import argparse
import os
import pprint

import _init_paths  # noqa: F401
import torch

from config import cfg, update_config
from dataset import mhp
from hipnet.optim import FlatAdam
from models import CPM
from utils.utils import create_logger, save_checkpoint


def parse_args():
    p = argparse.ArgumentParser(description='Train CPM')
    p.add_argument('--cfg', help='experiment configure file name', required=True, type=str)
    p.add_argument('opts', help='Modify config options using the command-line', default=None, nargs=argparse.REMAINDER)
    p.add_argument('--local_rank', default=0, type=int)
    p.add_argument('--iterations', default=None, type=int, help='stop after this many iterations in all')
    return p.parse_args()


def check_config(cfg):
    """what this tool refuses of a config, before any device work; returns the six stage weights"""
    if cfg.MODEL.NAME != 'CPM':
        raise ValueError('MODEL.NAME {}: tools/train_cpm.py trains CPM; tools/train.py trains the other 2-D '
                         'models'.format(cfg.MODEL.NAME))
    if list(cfg.DATASET.DATASET) != ['MHP_CPM_kpt']:
        raise ValueError('DATASET.DATASET {}: CPM trains on MHP_CPM_kpt (heat maps and centre maps)'.format(
            list(cfg.DATASET.DATASET)))
    if cfg.TRAIN.OPTIMIZER != 'adam':
        raise ValueError('TRAIN.OPTIMIZER {}: CPM trains with hipnet.optim.FlatAdam (adam)'.format(cfg.TRAIN.OPTIMIZER))
    world = int(os.environ.get('WORLD_SIZE', '1'))
    if world > 1:
        raise ValueError('WORLD_SIZE {}: data-parallel training of CPM is not built; run one process'.format(world))
    weights = tuple(float(v) for v in cfg.TRAIN.get('CPM_STAGE_WEIGHTS', (0, 0, 0, 0, 0, 1)))
    if len(weights) != 6 or min(weights) < 0 or not any(weights):
        raise ValueError('TRAIN.CPM_STAGE_WEIGHTS {}: six non-negative weights, one of them positive'.format(list(weights)))
    return weights


def main():
    args = parse_args()
    update_config(cfg, args)
    weights = check_config(cfg)
    local = int(os.environ.get('LOCAL_RANK', str(args.local_rank)))
    torch.cuda.set_device(local)
    device = torch.device('cuda', local)
    logger, final_output_dir, _ = create_logger(cfg, args.cfg, 'train')
    logger.info(pprint.pformat(vars(args)))

    model = CPM.get_pose_net(cfg, is_train=True, trainable=True).to(device).train()
    optimizer = FlatAdam(model, lr=cfg.TRAIN.LR, weight_decay=cfg.TRAIN.WD)
    c = cfg.clone()
    c.defrost()
    c.TEST.IMAGES_PER_GPU = cfg.TRAIN.IMAGES_PER_GPU
    loader = mhp.make_loader(c, 'MHP_CPM_kpt', cfg.DATASET.TRAIN_SET, False, heatmaps=True)

    def lr_at(epoch):
        return cfg.TRAIN.LR * (cfg.TRAIN.LR_FACTOR ** sum(epoch >= s for s in cfg.TRAIN.LR_STEP))

    it, done = 0, False
    for epoch in range(cfg.TRAIN.BEGIN_EPOCH, cfg.TRAIN.END_EPOCH):
        for g in optimizer.param_groups:
            g['lr'] = lr_at(epoch)
        total, count = 0.0, 0
        for i, ret in enumerate(loader):
            optimizer.zero_grad()
            maps = model(ret['imgs'].to(device), ret['centermaps'].to(device))
            loss = CPM.cpm_loss(maps, ret['heatmaps'].to(device).float(), weights)
            loss.backward()
            optimizer.step()
            it += 1
            if i % cfg.PRINT_FREQ == 0:
                value = float(loss)
                total, count = total + value, count + 1
                logger.info('Epoch: [{}][{}/{}] iteration {} lr {:.3g} loss {:.6f}'.format(epoch, i, len(loader), it,
                                                                                         optimizer.param_groups[0]['lr'], value))
            if args.iterations is not None and it >= args.iterations:
                done = True
                break
        save_checkpoint({'epoch': epoch + 1, 'model': cfg.MODEL.NAME, 'state_dict': model.state_dict(),
                         'loss': total / max(count, 1), 'optimizer': optimizer.state_dict()}, False, final_output_dir)
        if done:
            break
    final = os.path.join(final_output_dir, 'final_state.pth.tar')
    logger.info('saving final model state to {}'.format(final))
    torch.save({k: v.detach().clone() for k, v in model.state_dict().items()}, final)


if __name__ == '__main__':
    main()
