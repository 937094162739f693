"""Input step of tools/inference.py (reference tools/inference.py:117-121 + :196-213): read whole images, pack a
ragged batch of them into one staging buffer, and resize + normalise the batch on the device with one HIP launch
(hrnet_resize_normalize_u8, csrc/preprocess.hip). The RHD reader (dataset/rhd.py) packs the same way and warps its
crops with affine_warp_normalize (hrnet_affine_warp_normalize_u8).

The reference reads with cv2.imread(IMREAD_COLOR | IMREAD_IGNORE_ORIENTATION), resizes with cv2.resize (INTER_LINEAR)
to MODEL.IMAGE_SIZE, swaps BGR -> RGB and applies ToTensor + Normalize (its affine step is the identity on an
already-resized square image). Here PIL decodes (RGB, grey replicated, alpha dropped, EXIF orientation not applied)
and the kernel does the rest. Two documented deviations: cv2 blends with 11-bit fixed-point weights, so a u8 code
may differ from it by 1 at some pixels (the kernel blends in f32); and PIL's JPEG decoder may differ from cv2's."""
import ctypes
import os
from collections import namedtuple

import numpy as np
import torch

from dataset.target_generators import IMAGENET_MEAN, IMAGENET_STD

IMAGE_EXTENSIONS = ('.png', '.jpg', '.jpeg', '.bmp')
VIDEO_EXTENSIONS = ('.mp4', '.avi', '.mov', '.mkv', '.webm')

# pack_images(): `buffer` u8 [total bytes] (pinned when a device is present), `offsets` byte offset of each image,
# `table` int64 [n, 4] = {offset, H, W, row pitch} on the host, `sizes` (H, W) per image
Packed = namedtuple('Packed', ['buffer', 'offsets', 'table', 'sizes'])


def read_image_rgb(path):
    """HxWx3 uint8 RGB of an image file: grey and palette images become 3 channels, alpha is dropped, EXIF
    orientation is NOT applied (cv2.IMREAD_COLOR | IMREAD_IGNORE_ORIENTATION of the reference, then its
    BGR -> RGB swap)."""
    from PIL import Image
    with Image.open(path) as im:
        return np.array(im.convert('RGB'), dtype=np.uint8)          # a writable copy


def list_images(path):
    """image files of a directory sorted by name (the reference iterates os.listdir order); only
    IMAGE_EXTENSIONS are kept (the reference skips .mp4), sub-directories are skipped"""
    names = sorted(os.listdir(path))
    return [os.path.join(path, n) for n in names
            if n.lower().endswith(IMAGE_EXTENSIONS) and os.path.isfile(os.path.join(path, n))]


def validate_table(table, nbytes):
    """raise ValueError unless every row {offset, H, W, pitch} of `table` lies inside a buffer of `nbytes` bytes"""
    t = torch.as_tensor(table)
    if t.dim() != 2 or t.shape[1] != 4 or t.shape[0] < 1:
        raise ValueError('slot table must be (n, 4) int64 {offset, H, W, pitch}, got shape {}'.format(tuple(t.shape)))
    for i, (off, h, w, pitch) in enumerate(t.tolist()):
        if h < 1 or w < 1:
            raise ValueError('slot {}: empty image ({} x {})'.format(i, h, w))
        if pitch < 3 * w:
            raise ValueError('slot {}: row pitch {} < 3 * W = {}'.format(i, pitch, 3 * w))
        if off < 0 or off + (h - 1) * pitch + 3 * w > nbytes:
            raise ValueError('slot {}: bytes [{}, {}) exceed the {}-byte buffer'.format(
                i, off, off + (h - 1) * pitch + 3 * w, nbytes))


def pack_images(images, pin=None, align=64, staging=None):
    """list of HxWx3 uint8 arrays -> Packed: one staging buffer holding every image (rows dense, each image at an
    `align`-byte offset), so that a batch is ONE host-to-device copy. pin=None pins when a HIP device is present.
    `staging` (a u8 tensor from an earlier call) is reused when it is large enough: pinning is slow to allocate."""
    if not images:
        raise ValueError('pack_images: no images')
    offsets, sizes, off = [], [], 0
    for i, im in enumerate(images):
        a = np.asarray(im)
        if a.dtype != np.uint8 or a.ndim != 3 or a.shape[2] != 3 or a.shape[0] < 1 or a.shape[1] < 1:
            raise ValueError('pack_images: image {} must be a non-empty HxWx3 uint8 array, got {} {}'.format(
                i, a.dtype, a.shape))
        offsets.append(off)
        sizes.append((a.shape[0], a.shape[1]))
        off += -(-a.size // align) * align
    if pin is None:
        pin = torch.cuda.is_available()
    if staging is not None and staging.numel() >= off:
        buf = staging[:off]
    else:
        buf = torch.empty(off, dtype=torch.uint8, pin_memory=bool(pin))
    flat = buf.numpy()
    for a, o in zip(images, offsets):
        a = np.ascontiguousarray(a)
        flat[o:o + a.size] = a.reshape(-1)
    table = torch.tensor([[o, h, w, 3 * w] for o, (h, w) in zip(offsets, sizes)], dtype=torch.int64)
    return Packed(buf, offsets, table, sizes)


def resize_normalize(buffer, table, size, bgr=False, mean=IMAGENET_MEAN, std=IMAGENET_STD, validate=True):
    """buffer: uint8 1-D tensor on the HIP device holding the packed images; table: (n, 4) int64 HOST tensor
    {byte offset, H, W, row pitch}; size: (width, height) = MODEL.IMAGE_SIZE -> (n, 3, height, width) f32 on the
    device. validate=False skips the host check: a row outside the buffer then gives a NaN plane (device check)."""
    from hipnet import _capi as C
    if not isinstance(buffer, torch.Tensor) or not buffer.is_cuda or buffer.dtype != torch.uint8 or buffer.dim() != 1:
        raise RuntimeError('resize_normalize expects a 1-D uint8 tensor on the HIP device (no CPU path)')
    t = torch.as_tensor(table)
    if t.is_cuda:
        raise ValueError('resize_normalize: pass the slot table on the host (it is validated, then uploaded)')
    t = t.to(torch.int64).contiguous()
    if validate:
        validate_table(t, buffer.numel())
    wo, ho = int(size[0]), int(size[1])
    n = t.shape[0]
    dev = buffer.device
    slots = t.pin_memory().to(dev, non_blocking=True) if torch.cuda.is_available() else t.to(dev)
    out = torch.empty((n, 3, ho, wo), dtype=torch.float32, device=dev)
    m = (ctypes.c_float * 3)(*mean)
    s = (ctypes.c_float * 3)(*std)
    C.call('hrnet_resize_normalize_u8', buffer.data_ptr(), buffer.numel(), slots.data_ptr(), n, out.data_ptr(), ho, wo,
           m, s, int(bool(bgr)), C.stream_ptr())
    return out


def affine_warp_normalize(buffer, table, inv_mats, size, mean=IMAGENET_MEAN, std=IMAGENET_STD, validate=True):
    """buffer: uint8 1-D tensor on the HIP device; table: (n, 4) int64 HOST slot table (a crop is a slot pointing into
    its image, dataset/rhd.py); inv_mats: (n, 2, 3) or (n, 6) HOST inverse matrices, output pixel -> slot pixel;
    size: (width, height) -> (n, 3, height, width) f32 on the device: warpAffine (INTER_LINEAR, BORDER_CONSTANT 0 outside
    the slot) + ToTensor + Normalize in one launch of hrnet_affine_warp_normalize_u8 (csrc/preprocess.hip)."""
    from hipnet import _capi as C
    if not isinstance(buffer, torch.Tensor) or not buffer.is_cuda or buffer.dtype != torch.uint8 or buffer.dim() != 1:
        raise RuntimeError('affine_warp_normalize expects a 1-D uint8 tensor on the HIP device (no CPU path)')
    t = torch.as_tensor(table)
    m = torch.as_tensor(inv_mats)
    if t.is_cuda or m.is_cuda:
        raise ValueError('affine_warp_normalize: pass the slot table and the matrices on the host')
    t = t.to(torch.int64).contiguous()
    m = m.to(torch.float32).reshape(-1, 6).contiguous()
    if validate:
        validate_table(t, buffer.numel())
    n = t.shape[0]
    if m.shape[0] != n:
        raise ValueError('affine_warp_normalize: {} matrices for {} slots'.format(m.shape[0], n))
    wo, ho = int(size[0]), int(size[1])
    dev = buffer.device
    slots = t.pin_memory().to(dev, non_blocking=True)
    mats = m.pin_memory().to(dev, non_blocking=True)
    out = torch.empty((n, 3, ho, wo), dtype=torch.float32, device=dev)
    cm = (ctypes.c_float * 3)(*mean)
    cs = (ctypes.c_float * 3)(*std)
    C.call('hrnet_affine_warp_normalize_u8', buffer.data_ptr(), buffer.numel(), slots.data_ptr(), mats.data_ptr(), n,
           out.data_ptr(), ho, wo, cm, cs, C.stream_ptr())
    return out


def sequence_windows(n_frames, first, count):
    """frame index of every slot of a PoseAggr batch: `count` centre frames first .. first+count-1, laid out as
    [prev2 | prev1 | current | next1 | next2], each block `count` long (reference pose_hrnet_PoseAggr.py:598-639).
    Slot g*count + i holds frame clamp(first + i + g - 2, 0, n_frames - 1): at either end of the sequence the
    missing neighbours repeat the first / last frame (our choice; the reference's loaders pick the window)."""
    if n_frames < 1 or count < 1 or first < 0 or first + count > n_frames:
        raise ValueError('sequence_windows: frames {}..{} of a {}-frame sequence'.format(first, first + count - 1,
                                                                                          n_frames))
    t = np.arange(first, first + count)
    return np.concatenate([np.clip(t + g - 2, 0, n_frames - 1) for g in range(5)]).astype(np.int64)
