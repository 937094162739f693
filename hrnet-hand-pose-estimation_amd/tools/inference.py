"""Key points of whole images with a trained checkpoint, with the reference's flags (tools/inference.py:27-49):

    python tools/inference.py --cfg <yaml> --model_path <checkpoint> --image_path <image or directory> [--gpu 0]
                              [--batch_size 32] [--output .] [--vis 0|1] [--sequence auto|on|off] [KEY value ...]

Per batch: PIL decode on the host (dataset/preprocess.py) -> one staging buffer, ONE host-to-device copy -> one
hrnet_resize_normalize_u8 launch (resize to MODEL.IMAGE_SIZE + ToTensor + Normalize, reference :117-121) ->
model(x)[0] -> get_final_preds (reference :127-129). A directory is read in name order; only .png/.jpg/.jpeg/.bmp
files are used (the reference skips .mp4). There is no video decoder in this build: a video --image_path is refused.

Sequence mode (pose_hrnet_PoseAggr with MODEL.USE_WARPING_TEST; --sequence auto picks it): the sorted images are
consecutive frames; each batch uploads its frames once, with a halo of two frames either side, and the slot table
builds the 5 * B model input [prev2 | prev1 | current | next1 | next2] from them (neighbours clamped at the sequence ends).

Writes to --output: pose2d_pred.txt (N*K rows (x, y) in model-input pixels: the reference's file and units, :139,
:239), pose2d_pred_image.txt (the same rows in original-image pixels, the reference's dead branch :170-171) and
image_list.txt (the image of each block of K rows); --vis 1 adds vis/<name>.png overlays (matplotlib Agg).
"""
import argparse
import os
import time

import _init_paths  # noqa: F401
import numpy as np
import torch

from config import cfg, update_config
from core.evaluate2d import load_checkpoint_state
from dataset.preprocess import (IMAGE_EXTENSIONS, VIDEO_EXTENSIONS, list_images, pack_images, read_image_rgb,
                                resize_normalize, sequence_windows)
from models import pose_hrnet, pose_hrnet_PoseAggr, pose_hrnet_hamburger, pose_hrnet_softmax, swin_transformer  # noqa: F401
from utils.heatmap_decoding import get_final_preds

# the reference's per-finger colours (tools/inference.py:170-185): wrist -> palm -> ... -> tip
FINGERS = (('Thumb', 'r', range(1, 5)), ('Index', 'g', range(5, 9)), ('Middle', 'b', range(9, 13)),
           ('Ring', 'm', range(13, 17)), ('Pinky', 'y', range(17, 21)))


def parse_args(argv=None):
    p = argparse.ArgumentParser(description='Please specify the mode [training/assessment/predicting]')
    p.add_argument('--cfg', required=True, type=str, help='experiment configure file name')
    p.add_argument('opts', default=None, nargs=argparse.REMAINDER, help='modify config options (KEY value ...)')
    p.add_argument('--gpu', default=-1, type=int, help='device index (-1: cuda:0, there is no CPU forward)')
    p.add_argument('--world-size', default=1, type=int, help='accepted for the reference\'s command lines; ignored')
    p.add_argument('--model_path', default='', type=str)
    p.add_argument('--image_path', required=True, type=str, help='an image file or a directory of images')
    p.add_argument('--batch_size', default=32, type=int, help='images (or centre frames) per forward')
    p.add_argument('--output', default='.', type=str, help='directory of the result files')
    p.add_argument('--vis', default=0, type=int, choices=(0, 1), help='1: save a PNG overlay per image')
    p.add_argument('--sequence', default='auto', choices=('auto', 'on', 'off'),
                   help='frames of one sequence, 5-frame windows (auto: pose_hrnet_PoseAggr with USE_WARPING_TEST)')
    args = p.parse_args(argv)
    if args.batch_size < 1:
        p.error('--batch_size must be >= 1')
    return args


def resolve_sequence(config, mode):
    """--sequence auto|on|off -> bool. auto is on exactly for pose_hrnet_PoseAggr with MODEL.USE_WARPING_TEST (the
    only model that consumes 5-frame windows); on / off that contradict the model raise SystemExit."""
    aggr = config.MODEL.NAME == 'pose_hrnet_PoseAggr' and bool(config.MODEL.USE_WARPING_TEST)
    if mode == 'on' and not aggr:
        raise SystemExit('inference: --sequence on needs MODEL.NAME pose_hrnet_PoseAggr with MODEL.USE_WARPING_TEST')
    if mode == 'off' and aggr:
        raise SystemExit('inference: pose_hrnet_PoseAggr with MODEL.USE_WARPING_TEST takes 5-frame windows; use '
                         '--sequence on (or MODEL.USE_WARPING_TEST False for single frames)')
    return aggr


def collect_inputs(path):
    """--image_path -> list of image files; raises SystemExit with a message for a video or nothing to read"""
    if os.path.isdir(path):
        files = list_images(path)
        if not files:
            raise SystemExit('inference: no {} images in {}'.format('/'.join(IMAGE_EXTENSIONS), path))
        return files
    if path.lower().endswith(VIDEO_EXTENSIONS):
        raise SystemExit('inference: {} is a video; no video decoder is available here - decode its frames to '
                         'images and pass the directory'.format(path))
    if not os.path.isfile(path):
        raise SystemExit('inference: {} does not exist'.format(path))
    return [path]


def to_input_pixels(preds, config):
    """(N, K, 2) heat-map pixels -> (N*K, 2) float64 in model-input pixels (reference :139)"""
    p = np.asarray(preds, dtype=np.float64) * (config.MODEL.IMAGE_SIZE[0] / config.MODEL.HEATMAP_SIZE[0])
    return p.reshape(-1, 2)


def to_image_pixels(preds, sizes, config):
    """(N, K, 2) heat-map pixels, sizes [(H, W)] -> (N*K, 2) float64 in original-image pixels (reference :170-171:
    x * W / HEATMAP_SIZE[0], y * H / HEATMAP_SIZE[0])"""
    p = np.array(preds, dtype=np.float64)
    hs = float(config.MODEL.HEATMAP_SIZE[0])
    s = np.array([[w / hs, h / hs] for h, w in sizes], dtype=np.float64)
    return (p * s[:, None, :]).reshape(-1, 2)


def save_overlay(path, image, kps, title):
    """the reference's prediction figure (:166-185): image, wrist-to-palm segments and finger chains in the
    per-finger colours, saved to `path` instead of plt.show()"""
    import matplotlib
    matplotlib.use('Agg')
    import matplotlib.pyplot as plt
    fig = plt.figure()
    plt.imshow(image)
    for name, colour, idx in FINGERS:
        idx = list(idx)
        plt.plot([kps[0, 0], kps[idx[0], 0]], [kps[0, 1], kps[idx[0], 1]], c=colour, marker='.')
        plt.plot(kps[idx, 0], kps[idx, 1], c=colour, marker='.', label=name)
    plt.title(title)
    plt.axis('off')
    plt.legend(loc='upper right')
    fig.savefig(path)
    plt.close(fig)


def main(argv=None):
    args = parse_args(argv)
    update_config(cfg, args)
    files = collect_inputs(args.image_path)
    sequence = resolve_sequence(cfg, args.sequence)
    if args.gpu < 0:
        print('--gpu -1: this build has no CPU forward; using cuda:0')
    device = torch.device('cuda', max(args.gpu, 0))
    torch.cuda.set_device(device)

    model = eval(cfg.MODEL.NAME + '.get_pose_net')(cfg, is_train=False)
    if args.model_path:
        print('Loading model:', args.model_path)
        info = {}
        load_checkpoint_state(model, args.model_path, strict=False, info=info)
        print('missing keys: {}  unexpected keys: {}'.format(len(info['missing']), len(info['unexpected'])))
        if info['epoch'] is not None:
            print('Model epoch {}'.format(info['epoch']))
    else:
        print('no --model_path: running the untrained initialisation')
    model = model.to(device).eval()

    size = (cfg.MODEL.IMAGE_SIZE[0], cfg.MODEL.IMAGE_SIZE[1])
    n, bs = len(files), args.batch_size
    print('{} image(s), batch {}, {}'.format(n, bs, 'sequence mode (5-frame windows)' if sequence else 'image mode'))
    preds, sizes = [], []
    phase = dict(decode=0.0, upload=0.0, preprocess=0.0, forward=0.0)
    staging = None
    with torch.no_grad():
        for c0 in range(0, n, bs):
            count = min(bs, n - c0)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            if sequence:
                win = sequence_windows(n, c0, count)
                lo, hi = int(win.min()), int(win.max())
                images = [read_image_rgb(f) for f in files[lo:hi + 1]]
                packed = pack_images(images, staging=staging)
                table = packed.table[torch.from_numpy(win - lo)]
                sizes += packed.sizes[c0 - lo:c0 - lo + count]
            else:
                images = [read_image_rgb(f) for f in files[c0:c0 + count]]
                packed = pack_images(images, staging=staging)
                table = packed.table
                sizes += packed.sizes
            if staging is None or packed.buffer.numel() > staging.numel():
                staging = packed.buffer
            t1 = time.perf_counter()
            buf = packed.buffer.to(device, non_blocking=True)
            torch.cuda.synchronize()            # the staging buffer is reused by the next batch
            t2 = time.perf_counter()
            x = resize_normalize(buf, table, size)
            torch.cuda.synchronize()
            t3 = time.perf_counter()
            hm = model(x)[0]
            kp = get_final_preds(hm, use_softmax=cfg.MODEL.HEATMAP_SOFTMAX)
            torch.cuda.synchronize()
            t4 = time.perf_counter()
            print('Inference time: {:.4f} s'.format(t4 - t3))
            preds.append(kp.cpu().numpy())
            for k, v in zip(('decode', 'upload', 'preprocess', 'forward'), (t1 - t0, t2 - t1, t3 - t2, t4 - t3)):
                phase[k] += v
            if args.vis:
                vis_dir = os.path.join(args.output, 'vis')
                os.makedirs(vis_dir, exist_ok=True)
                off = c0 - lo if sequence else 0
                for i in range(count):
                    f = files[c0 + i]
                    kps = to_image_pixels(preds[-1][i:i + 1], [sizes[c0 + i]], cfg)
                    name = os.path.splitext(os.path.basename(f))[0] + '.png'
                    save_overlay(os.path.join(vis_dir, name), images[off + i], kps, f)

    preds = np.concatenate(preds, axis=0)
    os.makedirs(args.output, exist_ok=True)
    np.savetxt(os.path.join(args.output, 'pose2d_pred.txt'), to_input_pixels(preds, cfg))
    np.savetxt(os.path.join(args.output, 'pose2d_pred_image.txt'), to_image_pixels(preds, sizes, cfg))
    with open(os.path.join(args.output, 'image_list.txt'), 'w') as fh:
        fh.write(''.join(f + '\n' for f in files))
    total = sum(phase.values())
    print('{} image(s) in {:.3f} s: {:.1f} images/s (decode {:.3f} s, upload {:.3f} s, preprocess {:.3f} s, '
          'forward+decode {:.3f} s)'.format(n, total, n / max(total, 1e-9), phase['decode'], phase['upload'],
                                           phase['preprocess'], phase['forward']))
    print('wrote', os.path.join(args.output, 'pose2d_pred.txt'))


if __name__ == '__main__':
    main()
