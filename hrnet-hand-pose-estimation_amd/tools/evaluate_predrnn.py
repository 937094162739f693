"""Inference of HRNet_PredRNN_ResNet (MODEL.NAME `predrnn`, models/predrnn.py) over MHP frame windows:

    python tools/evaluate_predrnn.py --cfg experiments/Pred_RNN/PredRNN_8frames_256x256_adam_lr1e-3.yaml
        [--model_path <whole-model state_dict.pth.tar>] [--batch_size 1] [--num_batches N] [--gpu 0]

cfg -> the model, a strict load of --model_path when one is given ('module.' prefix stripped; a dict with 'state_dict' is
taken too; MODEL.HRNET_PRETRAINED loads the backbone alone) -> the window reader MHP_seq on DATASET.TEST_SET: a window is
len(DATASET.SEQ_IDX) frames seen by four cameras, and each view of a window is one sequence, so a batch of B windows is
4 B sequences (4 B, L, 3, H, W). When DATA_DIR holds no MHP frames the tool runs on synthetic frame windows instead
(--synthetic_batches of them, seeded noise) and says so. In eval mode under no_grad; prints sequences per second (after a
warm-up: the second half of the batches, at most from the 20th on) and writes the predictions (N, 21, 3) to
<OUTPUT_DIR>/eval_predrnn_<EXP_NAME>/pose3d_pred.npy.

No accuracy is computed or claimed: no checkpoint of this model exists anywhere (the reference has no tool that builds
it), and the model's 63 outputs have no documented frame or unit to compare MHP's labels in.
Refused: a MODEL.NAME other than predrnn, and what models/predrnn.py refuses of a config.
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
from dataset import mhp
from models import predrnn

MODEL_NAME = 'predrnn'


def parse_args(argv=None):
    p = argparse.ArgumentParser(description='Run HRNet_PredRNN_ResNet over MHP frame windows')
    p.add_argument('--cfg', required=True, type=str)
    p.add_argument('opts', default=None, nargs=argparse.REMAINDER)
    p.add_argument('--gpu', default=-1, type=int)
    p.add_argument('--batch_size', default=1, type=int, help='windows per batch (four sequences each)')
    p.add_argument('--model_path', default='', type=str, help='whole-model checkpoint (optional)')
    p.add_argument('--num_batches', default=None, type=int, help='batches to run (default: every batch)')
    p.add_argument('--synthetic_batches', default=4, type=int, help='batches of the synthetic fallback')
    return p.parse_args(argv)


def check_config(config):
    if config.MODEL.NAME != MODEL_NAME:
        raise ValueError('MODEL.NAME {!r}: tools/evaluate_predrnn.py runs HRNet_PredRNN_ResNet, MODEL.NAME {!r}'.format(
            config.MODEL.NAME, MODEL_NAME))
    predrnn.check_predrnn_config(config)
    if len(config.DATASET.SEQ_IDX) < 1:
        raise ValueError('DATASET.SEQ_IDX is empty: a window needs at least one frame')


def sequences(imgs, frames, views):
    """the loader's images (frames * B * views, 3, H, W) in mhp.slot_order (frame-major) -> (B * views, frames, 3, H, W):
    each view of a window is one sequence"""
    n = imgs.shape[0] // frames
    return imgs.view(frames, n, *imgs.shape[1:]).transpose(0, 1).contiguous()


def synthetic_batches(config, batch_size, count, device):
    """seeded noise in place of MHP windows: (4 * batch_size, L, 3, H, W) per batch"""
    g = torch.Generator(device=device).manual_seed(0)
    L, (w, h) = len(config.DATASET.SEQ_IDX), config.MODEL.IMAGE_SIZE
    for _ in range(count):
        yield torch.randn(len(mhp.VIEWS) * batch_size, L, 3, h, w, device=device, generator=g) * 0.5


def main(argv=None):
    args = parse_args(argv)
    update_config(cfg, args)
    check_config(cfg)
    if args.model_path and not os.path.isfile(args.model_path):
        raise ValueError('--model_path {!r}: no such file'.format(args.model_path))
    device = torch.device('cuda', max(args.gpu, 0))
    torch.cuda.set_device(device)
    model = predrnn.get_pose_net(cfg, is_train=False)
    if args.model_path:
        load_checkpoint_state(model, args.model_path)          # strict, `module.` stripped
    else:
        print('evaluate_predrnn: no --model_path: the head runs on its initial weights (throughput only)')
    model = model.to(device).eval()
    L, V = len(cfg.DATASET.SEQ_IDX), len(mhp.VIEWS)
    if os.path.isdir(mhp.frames_dir(cfg.DATA_DIR)):
        c = cfg.clone()
        c.defrost()
        c.TEST.IMAGES_PER_GPU = args.batch_size
        loader = mhp.make_loader(c, 'MHP_seq', cfg.DATASET.TEST_SET, False, max_batches=args.num_batches)
        batches = (sequences(ret['imgs'].to(device, non_blocking=True), L, V) for ret in loader)
        total = len(loader)
    else:
        total = args.synthetic_batches if args.num_batches is None else args.num_batches
        print('evaluate_predrnn: {} not found: running on {} synthetic batches of {} sequences of {} frames'.format(
            mhp.frames_dir(cfg.DATA_DIR), total, V * args.batch_size, L))
        batches = synthetic_batches(cfg, args.batch_size, total, device)
    preds, timed, t_total = [], 0, 0.0
    with torch.no_grad():
        for i, frames in enumerate(batches):
            torch.cuda.synchronize()
            t0 = time.time()
            pose = model(frames)
            torch.cuda.synchronize()
            if i >= 20 or i >= total // 2:
                t_total += time.time() - t0
                timed += frames.shape[0]
            preds.append(pose.cpu().numpy())
    out_dir = os.path.join(cfg.OUTPUT_DIR or 'output', 'eval_predrnn_' + cfg.EXP_NAME)
    os.makedirs(out_dir, exist_ok=True)
    preds = np.concatenate(preds) if preds else np.zeros((0, 21, 3), dtype=np.float32)
    np.save(os.path.join(out_dir, 'pose3d_pred.npy'), preds)
    print('sequences/s: {:.2f} ({} sequences of {} frames timed)'.format(timed / max(t_total, 1e-9), timed, L))
    print('{} predictions (N, 21, 3) in {}'.format(preds.shape[0], os.path.join(out_dir, 'pose3d_pred.npy')))
    return preds


if __name__ == '__main__':
    main()
    sys.exit(0)
