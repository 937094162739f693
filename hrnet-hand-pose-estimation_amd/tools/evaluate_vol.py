"""3-D evaluation of the volumetric triangulation model (MODEL.NAME `vol`) on MHP, with the flags of
tools/evaluate_3D.py that apply:

    python tools/evaluate_vol.py --cfg experiments/MHP/MHP_VolTriangulation_w32_v1.yaml
        --model_path <whole-model state_dict.pth.tar> --views '[1,2,3,4]' --batch_size 4 [--num_batches N] [--gpu 0]

cfg -> VolumetricTriangulationNet (models/triangulation.py), strict load of a whole-model checkpoint ('module.' prefix
stripped; a dict with 'state_dict' is taken too) -> the multi-view reader MHP_mv on DATASET.TEST_SET -> per batch, in
eval mode under no_grad: projection matrices from world coordinates to heat-map pixels (core/function_vol.py), the
model, then core/evaluate3d.py's accumulators fed with `vol_keypoints_3d` and the heat-map predictions. Prints fps
(multi-view frames per second, after warm-up as tools/evaluate_3D.py), the 2-D and 3-D EPE and both PCK AUCs; writes
mse2d_each_joint.txt, mse3d_each_joint.txt, PCK2d.txt and PCK3d.txt to <OUTPUT_DIR>/eval3D_results_<EXP_NAME>/.
Refusals are tools/train_vol.py's that apply: a MODEL.NAME other than vol and what models/triangulation.py refuses;
--model_path is required and must exist (the tool never evaluates random weights).
MODEL.NAME vol_CPM (experiments/MHP/MHP_VolTriangulation_CPM_v1.yaml) is evaluated the same way: the model is
VolumetricTriangulationNet_CPM, the reader MHP_CPM_mv, the refusals check_vol_cpm_config's.
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
from core.function_vol import run_model
from dataset import mhp
from evaluate_3D import parse_views
from models.triangulation import (VolumetricTriangulationNet, VolumetricTriangulationNet_CPM, check_vol_config,
                                  check_vol_cpm_config)

MODEL_NAME = 'vol'
# MODEL.NAME -> (the model, what it refuses of a config, its multi-view reader)
MODELS = {'vol': (VolumetricTriangulationNet, check_vol_config, 'MHP_mv'),
          'vol_CPM': (VolumetricTriangulationNet_CPM, check_vol_cpm_config, 'MHP_CPM_mv')}


def parse_args(argv=None):
    p = argparse.ArgumentParser(description='Evaluate the volumetric triangulation model on MHP')
    p.add_argument('--cfg', required=True, type=str)
    p.add_argument('opts', default=None, nargs=argparse.REMAINDER)
    p.add_argument('--gpu', default=-1, type=int)
    p.add_argument('--views', default='[1,2,3,4]', type=str, help="cameras to lift from, e.g. '[1,2,3,4]'")
    p.add_argument('--batch_size', default=4, type=int)
    p.add_argument('--model_path', default='', type=str, help='whole-model checkpoint (required)')
    p.add_argument('--num_batches', default=None, type=int, help='batches to evaluate (default: every batch)')
    return p.parse_args(argv)


def check_config(config):
    if config.MODEL.NAME not in MODELS:
        raise ValueError('MODEL.NAME {!r}: tools/evaluate_vol.py evaluates the volumetric triangulation model, '
                         'MODEL.NAME {!r} (or vol_CPM, the same on the CPM backbone; tools/evaluate_3D.py evaluates the '
                         '2-D models by triangulation)'.format(config.MODEL.NAME, MODEL_NAME))
    MODELS[config.MODEL.NAME][1](config)


def main(argv=None):
    args = parse_args(argv)
    update_config(cfg, args)
    views = parse_views(args.views)
    check_config(cfg)
    if not args.model_path or not os.path.isfile(args.model_path):
        raise ValueError('--model_path {!r}: no such file; tools/evaluate_vol.py evaluates a trained whole-model '
                         'checkpoint (tools/train_vol.py writes final_state.pth.tar), never random weights'.format(
                             args.model_path))
    frames = mhp.frames_dir(cfg.DATA_DIR)
    if not os.path.isdir(frames):
        sys.exit('evaluate_vol: {} not found: the 3-D evaluation reads the MHP multi-view frames '
                 '(DATA_DIR/MHP/annotated_frames)'.format(frames))
    device = torch.device('cuda', max(args.gpu, 0))
    torch.cuda.set_device(device)
    model_class, _check, reader = MODELS[cfg.MODEL.NAME]
    model = model_class(cfg, is_train=False)
    load_checkpoint_state(model, args.model_path)          # strict, `module.` stripped
    model = model.to(device).eval()
    c = cfg.clone()
    c.defrost()
    c.TEST.IMAGES_PER_GPU = args.batch_size
    loader = mhp.make_loader(c, reader, cfg.DATASET.TEST_SET, False, max_batches=args.num_batches, views=views)
    K, V = cfg.MODEL.NUM_JOINTS, len(views)
    acc = Eval3DAccumulator(K, cfg.MODEL.HEATMAP_SIZE[0])
    timed, t_total = 0, 0.0
    with torch.no_grad():
        for i, ret in enumerate(loader):
            B = ret['imgs'].shape[0] // V
            torch.cuda.synchronize()
            t0 = time.time()
            pose3d, pred = run_model(ret, model, device)[:2]
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
