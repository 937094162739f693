"""3-D evaluation on MHP with the reference's flags (tools/evaluate_3D.py:29-60,178-190,270-419):

    python tools/evaluate_3D.py --cfg <yaml> --model_path <state_dict.pth.tar> --views '[1,2,3,4]' --batch_size 32
        [--triangulation {dlt,ransac}] [--ransac_epsilon 25] [--ransac_iters 0] [--seed 0]

cfg -> MODEL.NAME pose_hrnet / pose_hrnet_softmax / multiview_pose_hrnet, strict load ('module.' prefix stripped) -> the multi-view reader
MHP_mv (dataset/mhp.py) on DATASET.TEST_SET of <DATA_DIR>/MHP, whatever DATASET.TEST_DATASET names (every 2-D MHP
yaml names a single-view reader, on which the reference's tool fails); a missing <DATA_DIR>/MHP/annotated_frames is an
error, there is no synthetic multi-view loader. Per batch of B frames and V views, on the device: model(imgs) ->
get_final_preds(heatmaps, MODEL.HEATMAP_SOFTMAX) -> projection matrices K [R|t] -> ONE hrnet_triangulate launch
(utils/multiview.py) that maps the heat-map predictions to frame pixels through the batch's `hm_inverse` and lifts
every joint of every frame -> core/evaluate3d.py accumulators (vectorised, no per-joint or per-sample loop). Prints
fps (multi-view frames per second of model + decode + triangulation, after warm-up as tools/evaluate_2D.py), the
2-D and 3-D EPE and both PCK AUCs (the reference's trapezoid, :121,134); writes mse2d_each_joint.txt,
mse3d_each_joint.txt, PCK2d.txt and PCK3d.txt to <OUTPUT_DIR>/eval3D_results_<EXP_NAME>/.

MODEL.NAME multiview_pose_hrnet (models/multiview_pose_hrnet.py, trained by tools/train_fusion.py) takes the batch as
(B, V, 3, H, W); its FUSED heat maps are decoded and triangulated, or its single-view maps when MODEL.AGGRE is false. The
lifting, DLT or --triangulation ransac, is the same.

The reference lifts pose_hrnet predictions with DLT_sii_pytorch (lib/utils/misc.py:64-97), two shifted inverse
iterations from a torch.rand start; this tool computes the vector they converge to (see utils/multiview.py).
The models alg, ransac, vol, vol_CPM and FTL are not built in this tool: they are refused with a ValueError (vol and
vol_CPM are evaluated by tools/evaluate_vol.py, FTL by tools/evaluate_ftl.py).

--triangulation ransac lifts with the reference's RANSAC over the views instead (lib/utils/misc.py:178-240, called by
RANSACTriangulationNet.forward, lib/models/triangulation.py:72-118), as a lifting method for the same two models: ONE
hrnet_triangulate_ransac launch per batch in place of the hrnet_triangulate one (utils/multiview.py). The MHP_mv
reader paints a disc over one joint per view (dataset/mhp.py), whose prediction in that view is a gross outlier that
the all-view DLT takes in at full weight; RANSAC drops the views that disagree with the best two-view solution.
--ransac_epsilon is the reference's threshold in the reference's unit, HALF the frame-pixel distance (25, its value,
keeps views within 50 px). --ransac_iters 0 (default) tries every pair of views in lexicographic order - deterministic,
and a superset of what random draws can see; N > 0 tries N random pairs per joint drawn as the reference draws them,
from --seed (drawn on the host before the timed region; the kernel draws nothing). The four result files keep their
format; the tool also prints the mean number of inlier views per joint and the share of points dropped per camera, and
writes ransac_inliers.txt (V x K: the share of frames in which the view was kept for the joint).
MODEL.DIRECT_OPTIMIZATION true (the reference's scipy Huber refinement of the RANSAC result) is not built and is
refused with --triangulation ransac.

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
import random
import sys
import time

import _init_paths  # noqa: F401
import numpy as np
import torch

from config import cfg, update_config
from core.evaluate2d import load_checkpoint_state
from core.evaluate3d import Eval3DAccumulator, auc
from dataset import mhp
from models import multiview_pose_hrnet, pose_hrnet, pose_hrnet_softmax
from utils.heatmap_decoding import get_final_preds
from utils.multiview import (MAX_HYPOTHESES, all_view_pairs, sample_view_pairs, triangulate_batch_of_points,
                             triangulate_ransac_batch)

MODELS = {'pose_hrnet': pose_hrnet.get_pose_net, 'pose_hrnet_softmax': pose_hrnet_softmax.get_pose_net,
          'multiview_pose_hrnet': multiview_pose_hrnet.get_pose_net}
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
    p.add_argument('--triangulation', default='dlt', choices=('dlt', 'ransac'),
                   help='lifting: DLT over all views, or RANSAC over the views and DLT over the inliers')
    p.add_argument('--ransac_epsilon', default=25.0, type=float,
                   help='inlier threshold on HALF the frame-pixel reprojection distance (the reference\'s unit)')
    p.add_argument('--ransac_iters', default=0, type=int,
                   help='0: every pair of views; N > 0: N sampled pairs per joint (the reference draws 10)')
    p.add_argument('--seed', default=0, type=int, help='seed of the sampled pairs')
    args = p.parse_args(argv)
    if not 0 <= args.ransac_iters <= MAX_HYPOTHESES:
        p.error('--ransac_iters {}: 0 (every pair) to {}'.format(args.ransac_iters, MAX_HYPOTHESES))
    if args.ransac_epsilon != args.ransac_epsilon:
        p.error('--ransac_epsilon is NaN')
    return args


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
        hint = ' (RANSAC is a lifting method here: --triangulation ransac)' if name == 'ransac' else ''
        if name in ('vol', 'vol_CPM'):
            hint = ' (the volumetric models are evaluated by tools/evaluate_vol.py)'
        raise ValueError('MODEL.NAME {!r} is not built in this project: tools/evaluate_3D.py evaluates {}{}'.format(
            name, ' / '.join(MODELS), hint))
    if name not in MODELS:
        raise ValueError('MODEL.NAME {!r}: tools/evaluate_3D.py evaluates {}'.format(name, ' / '.join(MODELS)))
    return MODELS[name]


def heatmaps_of(model, imgs, V, config):
    """the heat maps to decode, (B * V, K, h, w) in slot order b * V + v, of a batch of images in that order"""
    if config.MODEL.NAME == 'multiview_pose_hrnet':
        out = model(imgs.cuda(non_blocking=True).view(imgs.shape[0] // V, V, *imgs.shape[1:]))
        return out[0] if config.MODEL.AGGRE else out          # (fused, single), or single alone
    return model(imgs)[0]                                     # (heatmaps, inter_feat[, temperature])


def check_lifting(args, config):
    """--triangulation against the cfg: the reference's DIRECT_OPTIMIZATION refinement is not built"""
    if args.triangulation == 'ransac' and config.MODEL.DIRECT_OPTIMIZATION:
        raise ValueError('MODEL.DIRECT_OPTIMIZATION true is not built in this project: --triangulation ransac ends '
                         'with the DLT over the inlier views; set MODEL.DIRECT_OPTIMIZATION false')


def main(argv=None):
    args = parse_args(argv)
    update_config(cfg, args)
    views = parse_views(args.views)
    get_pose_net = build_model(cfg.MODEL.NAME)
    check_lifting(args, cfg)
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
    ransac = args.triangulation == 'ransac'
    shared_pairs = all_view_pairs(V).to(device) if ransac and args.ransac_iters == 0 else None
    kept = torch.zeros(V, K, dtype=torch.float64, device=device)      # frames in which view v was kept for joint k
    n_frames, rng = 0, random.Random(args.seed)
    with torch.no_grad():
        for i, ret in enumerate(loader):
            imgs = ret['imgs']                                         # (B*V, 3, H, W), slot b * V + v
            B = imgs.shape[0] // V
            intrinsic = ret['intrinsic_matrix'].to(device, non_blocking=True)
            extrinsic = ret['extrinsic_matrices'].to(device, non_blocking=True)
            hm_inverse = ret['hm_inverse'].to(device, non_blocking=True)
            pairs = shared_pairs
            if ransac and pairs is None:
                # the host decides the hypotheses: one stream of draws over the whole evaluation, joint after joint
                pairs = sample_view_pairs(B * K, V, args.ransac_iters, rng).to(device)
            torch.cuda.synchronize()
            t0 = time.time()
            hm = heatmaps_of(model, imgs, V, cfg)
            pred = get_final_preds(hm, cfg.MODEL.HEATMAP_SOFTMAX)     # (B*V, K, 2) heat-map pixels
            proj = intrinsic[:, None] @ extrinsic                      # (B, V, 3, 4)
            if ransac:
                pose3d, inl = triangulate_ransac_batch(proj, pred.view(B, V, K, 2), pairs, args.ransac_epsilon,
                                                       to_frame=hm_inverse)
            else:
                pose3d = triangulate_batch_of_points(proj, pred.view(B, V, K, 2), to_frame=hm_inverse)
            torch.cuda.synchronize()
            if i >= 20 or i >= len(loader) // 2:
                t_total += time.time() - t0
                timed += B
            if ransac:
                kept += inl.sum(0).t()
                n_frames += B
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
    if ransac:
        share = (kept / max(n_frames, 1)).cpu().numpy()                # (V, K)
        np.savetxt(os.path.join(out_dir, 'ransac_inliers.txt'), share)
        print('RANSAC inlier views per joint: {:.3f} of {}; dropped per camera: {}'.format(
            share.sum(0).mean(), V, ' '.join('cam{} {:.1%}'.format(c, 1.0 - s) for c, s in zip(views, share.mean(1)))))
    print('results in {}'.format(out_dir))


if __name__ == '__main__':
    main()
