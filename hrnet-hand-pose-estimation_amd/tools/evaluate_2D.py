"""2-D evaluation entry point with the reference's flags (tools/evaluate_2D.py:29-59):

    python tools/evaluate_2D.py --cfg <yaml> --model_path <state_dict.pth.tar> --batch_size 32 --gpu 0

cfg -> get_pose_net(is_train=False) -> strict load ('module.' prefix stripped) -> eval loop:
model(imgs) + get_final_preds -> per-joint end-point error (pixels of the input crop) weighted by
visibility, PCK for thresholds 1..49 px, fps after 20 warm-up iterations; writes
mse2d_each_joint.txt and PCK2d.txt (tools/evaluate_2D.py:172-294). Data: TEST_DATASET / TEST_SET through
dataset/build.py - the RHD reader (every sample, in order; --num_batches caps it only when given) when the
annotations exist, otherwise the synthetic RHD-shaped loader (24 batches unless --num_batches is given). RHD
coordinates are rescaled to original-image pixels with `* crop_size / hm_size + corner` (:235-240). The MHP readers
(dataset/mhp.py: MHP, MHP_kpt, MHP_seq) serve <DATA_DIR>/MHP; their batches carry `hm_inverse`, the inverse of each
sample's heat-map matrix, and the coordinates are mapped back through it. The reference scales MHP by 640/64 and
480/64 instead (:241-245), which does not invert its own 'short'-scale crop of the frame. With MODEL.NAME
pose_hrnet_transformer on MHP_seq the poses evaluated are the model's refined poses of the centre frames. With MODEL.NAME
CPM (MHP_CPM_kpt) the model takes the batch's `centermaps` as well, and the key points are the integer arg-max of the last
stage's map without its background channel (reference :184-189), mapped back to the frame through `hm_inverse`.
"""
import argparse
import os
import time

import _init_paths  # noqa: F401
import numpy as np
import torch

from config import cfg, update_config
from core.evaluate2d import Eval2DAccumulator, load_checkpoint_state
from dataset.build import make_dataloader
from models import CPM, pose_hrnet, pose_hrnet_PoseAggr, pose_hrnet_hamburger, pose_hrnet_softmax, pose_hrnet_transformer, swin_transformer  # noqa: F401
from utils.heatmap_decoding import decode_argmax, get_final_preds


def parse_args():
    p = argparse.ArgumentParser(description='Please specify the mode [training/assessment/predicting]')
    p.add_argument('--cfg', required=True, type=str)
    p.add_argument('opts', default=None, nargs=argparse.REMAINDER)
    p.add_argument('--gpu', default=-1, type=int)
    p.add_argument('--world-size', default=1, type=int)
    p.add_argument('--is_vis', default=0, type=int)
    p.add_argument('--batch_size', default=32, type=int)
    p.add_argument('--model_path', default='', type=str)
    p.add_argument('--num_batches', default=None, type=int,
                   help='batches to evaluate (synthetic loader: default 24; a real dataset: every batch)')
    return p.parse_args()


def main():
    args = parse_args()
    update_config(cfg, args)
    device = torch.device('cuda', max(args.gpu, 0))
    torch.cuda.set_device(device)
    model = eval(cfg.MODEL.NAME + '.get_pose_net')(cfg, is_train=False)
    if args.model_path:
        load_checkpoint_state(model, args.model_path)
    model = model.to(device).eval()
    c = cfg.clone()
    c.defrost()
    c.TEST.IMAGES_PER_GPU = args.batch_size
    loader = list(make_dataloader(c, False, num_batches=24 if args.num_batches is None else args.num_batches,
                                  max_batches=args.num_batches).values())[0]
    K = cfg.MODEL.NUM_JOINTS
    # accumulators and file formats of the reference (tools/evaluate_2D.py:166-169,270-294): per-joint error
    # sums, PCK counted with a strict `<` over all visible joints, PCK2d.txt = two rows (thresholds, PCK);
    # coordinates are scaled from heat-map pixels to original-image pixels with the batch's crop_size / corner (RHD,
    # :235-240) or its hm_inverse matrices (MHP), or to the input crop for the synthetic loader (:241-245 with orig
    # size = crop size)
    acc = Eval2DAccumulator(K, cfg.MODEL.HEATMAP_SIZE[0])
    crop = (cfg.MODEL.IMAGE_SIZE[0], cfg.MODEL.IMAGE_SIZE[1])
    timed, t_total = 0, 0.0
    with torch.no_grad():
        for i, ret in enumerate(loader):
            imgs = ret['imgs'].to(device)
            torch.cuda.synchronize()
            t0 = time.time()
            if cfg.MODEL.NAME == 'pose_hrnet_transformer':
                # MHP_seq's frame-major window batch -> the refined poses of the centre frames, (4 B, K, 2)
                pred = model(imgs, frames=len(cfg.DATASET.SEQ_IDX))[0]
            elif cfg.MODEL.NAME == 'CPM':
                # the last stage's map without its background channel, decoded by integer argmax (the reference's
                # get_kpts, evaluate_2D.py:184-189); MHP_CPM_kpt's hm_inverse maps the stride-8 pixels to the frame
                pred = decode_argmax(model(imgs, ret['centermaps'].to(device))[-1][:, 1:])
            else:
                hm = model(imgs)[0]      # (heatmaps, inter_feat[, temperature])
                pred = get_final_preds(hm, cfg.MODEL.HEATMAP_SOFTMAX)
            torch.cuda.synchronize()
            if i >= 20 or i >= len(loader) // 2:
                t_total += time.time() - t0
                timed += imgs.shape[0]
            if 'hm_inverse' in ret:
                acc.add(pred.cpu().numpy(), ret['pose2d'].numpy(), ret['visibility'].numpy(),
                        inverse=ret['hm_inverse'].numpy())
            elif 'crop_size' in ret:
                acc.add(pred.cpu().numpy(), ret['pose2d'].numpy(), ret['visibility'].numpy(),
                        crop_size=ret['crop_size'].numpy(), corner=ret['corner'].numpy())
            else:
                acc.add(pred.cpu().numpy(), ret['pose2d'].numpy(), ret['visibility'].numpy(), orig_size=crop)
    out_dir = os.path.join(cfg.OUTPUT_DIR or 'output', 'eval2D_results_' + cfg.EXP_NAME)
    mse_each, pck = acc.save(out_dir)
    print('fps: {:.1f}'.format(timed / max(t_total, 1e-9)))
    print('mean EPE {:.3f} px  PCK@20px {:.4f}  AUC(1-49px) {:.4f}'.format(np.nanmean(mse_each), pck[1, 19], pck[1].mean()))


if __name__ == '__main__':
    main()
