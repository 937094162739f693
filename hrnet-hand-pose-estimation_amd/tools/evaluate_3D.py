"""3-D evaluation on MHP with the reference's flags (tools/evaluate_3D.py:29-60,178-190,270-419):

    python tools/evaluate_3D.py --cfg <yaml> --model_path <state_dict.pth.tar> --views '[1,2,3,4]' --batch_size 32

cfg -> MODEL.NAME pose_hrnet / pose_hrnet_softmax, strict load ('module.' prefix stripped) -> the multi-view reader
MHP_mv (dataset/mhp.py) on DATASET.TEST_SET of <DATA_DIR>/MHP, whatever DATASET.TEST_DATASET names (every 2-D MHP
yaml names a single-view reader, on which the reference's tool fails); a missing <DATA_DIR>/MHP/annotated_frames is an
error, there is no synthetic multi-view loader. Per batch of B frames and V views, on the device: model(imgs) ->
get_final_preds(heatmaps, MODEL.HEATMAP_SOFTMAX) -> projection matrices K [R|t] -> ONE hrnet_triangulate launch
(utils/multiview.py) that maps the heat-map predictions to frame pixels through the batch's `hm_inverse` and lifts
every joint of every frame -> core/evaluate3d.py accumulators (vectorised, no per-joint or per-sample loop). Prints
fps (multi-view frames per second of model + decode + triangulation, after warm-up as tools/evaluate_2D.py), the
2-D and 3-D EPE and both PCK AUCs (the reference's trapezoid, :121,134); writes mse2d_each_joint.txt,
mse3d_each_joint.txt, PCK2d.txt and PCK3d.txt to <OUTPUT_DIR>/eval3D_results_<EXP_NAME>/.

The reference lifts pose_hrnet predictions with DLT_sii_pytorch (lib/utils/misc.py:64-97), two shifted inverse
iterations from a torch.rand start; this tool computes the vector they converge to (see utils/multiview.py).
The models alg, ransac, vol, vol_CPM and FTL are not built: they are refused with a ValueError.

Reference defects not reproduced:
- get_final_preds(heatmaps, cfg) (:296) passes the cfg as `use_softmax`, which is always truthy, so every model is
  decoded by expectation; here MODEL.HEATMAP_SOFTMAX chooses, as in tools/evaluate_2D.py;
- the input() pauses and the per-joint prints (:374-387) are gone; --is_vis is accepted, nothing is plotted;
- the reference scales the heat-map y by orig_height / heatmap_size[0] (:300), which does not invert its own crop of
  the frame; here the points are mapped through each image's heat-map inverse, as tools/evaluate_2D.py does for MHP.
"""
import argparse
import ast
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
from models import pose_hrnet, pose_hrnet_softmax
from utils.heatmap_decoding import get_final_preds
from utils.multiview import triangulate_batch_of_points

MODELS = {'pose_hrnet': pose_hrnet.get_pose_net, 'pose_hrnet_softmax': pose_hrnet_softmax.get_pose_net}
NOT_BUILT = ('alg', 'ransac', 'vol', 'vol_CPM', 'FTL')


def parse_args(argv=None):
    p = argparse.ArgumentParser(description='Please specify the mode [training/assessment/predicting]')
    p.add_argument('--cfg', required=True, type=str)
    p.add_argument('opts', default=None, nargs=argparse.REMAINDER)
    p.add_argument('--gpu', default=-1, type=int)
    p.add_argument('--world-size', default=1, type=int)
    p.add_argument('--is_vis', default=0, type=int)
    p.add_argument('--views', default='[1,2,3,4]', type=str, help="cameras to triangulate from, e.g. '[1,2,3,4]'")
    p.add_argument('--batch_size', default=32, type=int)
    p.add_argument('--model_path', default='', type=str)
    p.add_argument('--num_batches', default=None, type=int, help='batches to evaluate (default: every batch)')
    return p.parse_args(argv)


def parse_views(text):
    """'[1,2,3,4]' -> (1, 2, 3, 4): two or more distinct views of 1..4"""
    try:
        views = ast.literal_eval(text)
    except (ValueError, SyntaxError):
        raise ValueError('--views {!r}: expected a list such as [1,2,3,4]'.format(text))
    views = tuple(views) if isinstance(views, (list, tuple)) else (views,)
    if len(views) < 2 or len(set(views)) != len(views) or not all(isinstance(v, int) and v in mhp.VIEWS
                                                                   for v in views):
        raise ValueError('--views {!r}: two or more distinct views of {}'.format(text, list(mhp.VIEWS)))
    return views


def build_model(name):
    if name in NOT_BUILT:
        raise ValueError('MODEL.NAME {!r} is not built in this project: tools/evaluate_3D.py evaluates {}'.format(
            name, ' / '.join(MODELS)))
    if name not in MODELS:
        raise ValueError('MODEL.NAME {!r}: tools/evaluate_3D.py evaluates {}'.format(name, ' / '.join(MODELS)))
    return MODELS[name]


def main(argv=None):
    args = parse_args(argv)
    update_config(cfg, args)
    views = parse_views(args.views)
    get_pose_net = build_model(cfg.MODEL.NAME)
    frames = mhp.frames_dir(cfg.DATA_DIR)
    if not os.path.isdir(frames):
        sys.exit('evaluate_3D: {} not found: the 3-D evaluation reads the MHP multi-view frames '
                 '(DATA_DIR/MHP/annotated_frames)'.format(frames))
    device = torch.device('cuda', max(args.gpu, 0))
    torch.cuda.set_device(device)
    model = get_pose_net(cfg, is_train=False)
    if args.model_path:
        load_checkpoint_state(model, args.model_path)
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
            intrinsic = ret['intrinsic_matrix'].to(device, non_blocking=True)
            extrinsic = ret['extrinsic_matrices'].to(device, non_blocking=True)
            hm_inverse = ret['hm_inverse'].to(device, non_blocking=True)
            torch.cuda.synchronize()
            t0 = time.time()
            hm = model(imgs)[0]      # (heatmaps, inter_feat[, temperature])
            pred = get_final_preds(hm, cfg.MODEL.HEATMAP_SOFTMAX)     # (B*V, K, 2) heat-map pixels
            proj = intrinsic[:, None] @ extrinsic                      # (B, V, 3, 4)
            pose3d = triangulate_batch_of_points(proj, pred.view(B, V, K, 2), to_frame=hm_inverse)
            torch.cuda.synchronize()
            if i >= 20 or i >= len(loader) // 2:
                t_total += time.time() - t0
                timed += B
            acc.add(pred.cpu().numpy(), ret['pose2d'].numpy(), ret['visibility'].numpy(), ret['hm_inverse'].numpy(),
                    pose3d.cpu().numpy(), ret['pose3d'].numpy())
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
