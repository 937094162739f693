"""3-D evaluation of FTLMultiviewNet (MODEL.NAME `FTL`) on MHP, with the flags of tools/evaluate_vol.py:

    python tools/evaluate_ftl.py --cfg experiments/MHP/MHP_HRNet_w32_softmax_pose2dloss_FTL_v1.yaml
        --model_path <whole-model state_dict.pth.tar> --views '[1,2,3,4]' --batch_size 2 [--num_batches N] [--gpu 0]

cfg -> FTLMultiviewNet (models/FTL_encoder_decoder.py), strict load of a whole-model checkpoint ('module.' prefix
stripped; a dict with 'state_dict' is taken too) -> the multi-view reader MHP_mv on DATASET.TEST_SET -> per batch, in
eval mode under no_grad: the model on the images as (B, V, 3, H, W) with the batch's extrinsic and intrinsic matrices and
its `hm_inverse` (heat-map pixels -> frame pixels, in front of the DLT), then core/evaluate3d.py's accumulators fed with
`pose3d_pred` and the heat-map predictions. Prints fps (multi-view frames per second, after warm-up as
tools/evaluate_3D.py), the 2-D and 3-D EPE and both PCK AUCs; writes mse2d_each_joint.txt, mse3d_each_joint.txt, PCK2d.txt
and PCK3d.txt to <OUTPUT_DIR>/eval3D_results_<EXP_NAME>/.
Refused: a MODEL.NAME other than FTL, what models/FTL_encoder_decoder.py refuses, a number of --views other than
DATASET.NUM_VIEWS (fuse_after_FTL's width is built for it); --model_path is required and must exist (the tool never
evaluates random weights).
"""
import argparse
import os
import sys
import time

import _init_paths  # noqa: F401
import numpy as np
import torch

from config import cfg, update_config
from core.evaluate2d import load_checkpoint_state
from core.evaluate3d import Eval3DAccumulator, auc
from dataset import mhp
from evaluate_3D import parse_views
from models.FTL_encoder_decoder import FTLMultiviewNet, check_config as check_ftl_config

MODEL_NAME = 'FTL'


def parse_args(argv=None):
    p = argparse.ArgumentParser(description='Evaluate FTLMultiviewNet on MHP')
    p.add_argument('--cfg', required=True, type=str)
    p.add_argument('opts', default=None, nargs=argparse.REMAINDER)
    p.add_argument('--gpu', default=-1, type=int)
    p.add_argument('--views', default='[1,2,3,4]', type=str, help="cameras to fuse and lift from, e.g. '[1,2,3,4]'")
    p.add_argument('--batch_size', default=2, type=int)
    p.add_argument('--model_path', default='', type=str, help='whole-model checkpoint (required)')
    p.add_argument('--num_batches', default=None, type=int, help='batches to evaluate (default: every batch)')
    return p.parse_args(argv)


def check_config(config, views=None):
    if config.MODEL.NAME != MODEL_NAME:
        raise ValueError('MODEL.NAME {!r}: tools/evaluate_ftl.py evaluates FTLMultiviewNet, MODEL.NAME {!r} '
                         '(tools/evaluate_3D.py evaluates the 2-D models by triangulation)'.format(
                             config.MODEL.NAME, MODEL_NAME))
    check_ftl_config(config)
    if views is not None and len(views) != int(config.DATASET.NUM_VIEWS):
        raise ValueError('--views {}: {} views, the model fuses DATASET.NUM_VIEWS = {}'.format(
            list(views), len(views), config.DATASET.NUM_VIEWS))


def main(argv=None):
    args = parse_args(argv)
    update_config(cfg, args)
    views = parse_views(args.views)
    check_config(cfg, views)
    if not args.model_path or not os.path.isfile(args.model_path):
        raise ValueError('--model_path {!r}: no such file; tools/evaluate_ftl.py evaluates a trained whole-model '
                         'checkpoint, never random weights'.format(args.model_path))
    frames = mhp.frames_dir(cfg.DATA_DIR)
    if not os.path.isdir(frames):
        sys.exit('evaluate_ftl: {} not found: the 3-D evaluation reads the MHP multi-view frames '
                 '(DATA_DIR/MHP/annotated_frames)'.format(frames))
    device = torch.device('cuda', max(args.gpu, 0))
    torch.cuda.set_device(device)
    model = FTLMultiviewNet(cfg, is_train=False)
    load_checkpoint_state(model, args.model_path)          # strict, `module.` stripped
    model = model.to(device).eval()
    c = cfg.clone()
    c.defrost()
    c.TEST.IMAGES_PER_GPU = args.batch_size
    loader = mhp.make_loader(c, 'MHP_mv', cfg.DATASET.TEST_SET, False, max_batches=args.num_batches, views=views)
    K, V = cfg.MODEL.NUM_JOINTS, len(views)
    acc = Eval3DAccumulator(K, cfg.MODEL.HEATMAP_SIZE[0])
    timed, t_total = 0, 0.0
    with torch.no_grad():
        for i, ret in enumerate(loader):
            imgs = ret['imgs']                                         # (B*V, 3, H, W), slot b * V + v
            B = imgs.shape[0] // V
            extrinsic = ret['extrinsic_matrices'].to(device, non_blocking=True)
            hm_inverse = ret['hm_inverse'].to(device, non_blocking=True)
            torch.cuda.synchronize()
            t0 = time.time()
            imgs = imgs.to(device, non_blocking=True)
            _, pred, pose3d = model(imgs.view(B, V, *imgs.shape[1:]), extrinsic, ret['intrinsic_matrix'],
                                    to_frame=hm_inverse)
            torch.cuda.synchronize()
            if i >= 20 or i >= len(loader) // 2:
                t_total += time.time() - t0
                timed += B
            acc.add(pred.reshape(B * V, K, 2).cpu().numpy(), ret['pose2d'].numpy(), ret['visibility'].numpy(),
                    ret['hm_inverse'].numpy(), pose3d.cpu().numpy(), ret['pose3d'].numpy())
    out_dir = os.path.join(cfg.OUTPUT_DIR or 'output', 'eval3D_results_' + cfg.EXP_NAME)
    mse2d, pck2d, mse3d, pck3d = acc.save(out_dir)
    print('fps: {:.1f} (multi-view frames of {} views per second)'.format(timed / max(t_total, 1e-9), V))
    print('valid samples: {}'.format(acc.n_valid))
    print('2D pose EPE: {:.4f} px'.format(np.nanmean(mse2d)))
    print('3D pose EPE: {:.4f} mm'.format(np.nanmean(mse3d) if acc.n_valid else float('nan')))
    print('2D PCKAUC: {:.4f}'.format(auc(pck2d[0], pck2d[1])))
    print('3D PCKAUC: {:.4f}'.format(auc(pck3d[0], pck3d[1])))
    print('results in {}'.format(out_dir))


if __name__ == '__main__':
    main()
