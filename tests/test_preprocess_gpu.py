"""hrnet_resize_normalize_u8 (csrc/preprocess.hip) against a float64 restatement: torch.nn.functional.interpolate
(bilinear, align_corners=False, antialias=False: cv2 INTER_LINEAR geometry) on the CPU, torch.round (half to even),
then ToTensor + Normalize. The kernel's u8 code is recovered exactly from its output as round((out*std + mean)*255);
it must equal the oracle's code except within 1e-3 of a .5 boundary (f32 blend against f64), and never differ by
more than 1."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from spawned import spawned

pytestmark = pytest.mark.gpu

MEAN = torch.tensor([0.485, 0.456, 0.406], dtype=torch.float64).view(3, 1, 1)
STD = torch.tensor([0.229, 0.224, 0.225], dtype=torch.float64).view(3, 1, 1)


def _img(h, w, seed):
    return np.random.default_rng(seed).integers(0, 256, (h, w, 3), dtype=np.uint8)


def _oracle_values(img, ho, wo, bgr=False):
    """(3, ho, wo) float64 blended values before rounding"""
    x = torch.from_numpy(img).double().permute(2, 0, 1)[None]
    if bgr:
        x = x.flip(1)
    return F.interpolate(x, size=(ho, wo), mode='bilinear', align_corners=False, antialias=False)[0]


def _codes(out):
    """(3, ho, wo) f32 kernel output -> the u8 codes it encodes (exact)"""
    return torch.round((out.double().cpu() * STD + MEAN) * 255.0)


def _check(out, img, bgr=False):
    ho, wo = out.shape[-2:]
    v = _oracle_values(img, ho, wo, bgr)
    want = torch.round(v).clamp(0, 255)
    got = _codes(out)
    assert torch.isfinite(got).all()
    diff = (got - want).abs()
    near_half = ((v - v.floor()) - 0.5).abs() < 1e-3
    assert diff.max().item() <= 1.0
    bad = (diff > 0) & ~near_half
    assert not bad.any(), 'codes differ away from a .5 boundary at {} pixels'.format(int(bad.sum()))
    return int((diff > 0).sum())


def _run(images, size, bgr=False):
    from dataset.preprocess import pack_images, resize_normalize
    p = pack_images(images)
    return resize_normalize(p.buffer.cuda(), p.table, size, bgr=bgr)


@spawned
def test_identity_size_is_bit_identical_to_normalize_u8():
    from dataset.target_generators import normalize_u8
    img = _img(96, 80, 1)
    out = _run([img], (80, 96))
    ref = normalize_u8(torch.from_numpy(img)[None].cuda())
    assert out.shape == (1, 3, 96, 80)
    assert torch.equal(out, ref)


@spawned
def test_exact_2x_downscale_is_the_2x2_mean():
    img = _img(512, 512, 2)
    out = _run([img], (256, 256))[0]
    m = torch.from_numpy(img).double().permute(2, 0, 1).reshape(3, 256, 2, 256, 2).mean((2, 4))
    assert torch.equal(_codes(out), torch.round(m))           # the mean is exact in f32: ties round to even


@pytest.mark.parametrize('h,w,ho,wo', [(60, 100, 256, 256),       # upscale
                                       (1080, 1920, 256, 256),    # non-integer downscale
                                       (479, 641, 256, 256),
                                       (1, 1, 256, 256),          # degenerate sources
                                       (1, 37, 256, 256),
                                       (53, 1, 256, 256),
                                       (200, 300, 384, 288)])     # non-square output (IMAGE_SIZE = [288, 384])
@spawned
def test_resize_matches_the_f64_oracle(h, w, ho, wo):
    img = _img(h, w, h * 7 + w)
    out = _run([img], (wo, ho))
    assert out.shape == (1, 3, ho, wo)
    n = _check(out[0], img)
    print('{}x{} -> {}x{}: {} codes one off at a .5 boundary'.format(h, w, ho, wo, n))


@spawned
def test_bgr_reads_the_channels_reversed():
    img = _img(70, 90, 3)
    out = _run([img], (64, 48), bgr=True)[0]
    _check(out, img, bgr=True)
    assert torch.equal(out, _run([np.ascontiguousarray(img[..., ::-1])], (64, 48))[0])


@spawned
def test_row_pitch_larger_than_3w():
    from dataset.preprocess import resize_normalize
    h, w, pitch, off = 41, 29, 3 * 29 + 13, 7
    img = _img(h, w, 4)
    buf = np.full(off + h * pitch, 255, np.uint8)              # padding bytes would show up as bright pixels
    for r in range(h):
        buf[off + r * pitch:off + r * pitch + 3 * w] = img[r].reshape(-1)
    out = resize_normalize(torch.from_numpy(buf).cuda(), torch.tensor([[off, h, w, pitch]]), (50, 60))[0]
    _check(out, img)


@spawned
def test_repeated_slots_and_mixed_sizes_in_one_launch():
    from dataset.preprocess import pack_images, resize_normalize
    ims = [_img(33, 47, 5), _img(300, 200, 6), _img(256, 256, 7)]
    p = pack_images(ims)
    order = [2, 0, 0, 1, 2, 1, 0]
    table = p.table[torch.tensor(order)]
    out = resize_normalize(p.buffer.cuda(), table, (128, 128))
    assert out.shape == (7, 3, 128, 128)
    for s, i in enumerate(order):
        _check(out[s], ims[i])
    assert torch.equal(out[1], out[2]) and torch.equal(out[0], out[4])


@spawned
def test_source_beyond_2_31_bytes():
    from dataset.preprocess import resize_normalize
    nbytes = 2_200_000_000
    buf = torch.zeros(nbytes, dtype=torch.uint8, device='cuda')
    lo, hi = _img(40, 50, 8), _img(120, 90, 9)
    off = (1 << 31) + 4099                                      # byte offset > 2^31 (and odd)
    buf[:lo.size] = torch.from_numpy(lo.reshape(-1)).cuda()
    buf[off:off + hi.size] = torch.from_numpy(hi.reshape(-1)).cuda()
    last = nbytes - hi.size                                      # the very end of the buffer
    buf[last:] = torch.from_numpy(hi.reshape(-1)).cuda()
    table = torch.tensor([[0, 40, 50, 150], [off, 120, 90, 270], [last, 120, 90, 270]])
    out = resize_normalize(buf, table, (64, 64))
    torch.cuda.synchronize()
    _check(out[0], lo)
    _check(out[1], hi)
    assert torch.equal(out[1], out[2])
    del buf


@spawned
def test_out_of_range_rows_give_nan_planes_and_leave_the_others_exact():
    from dataset.preprocess import pack_images, resize_normalize
    ims = [_img(30, 40, 10), _img(25, 35, 11)]
    p = pack_images(ims)
    nb = p.buffer.numel()
    bad = [[nb - 10, 5, 5, 15],           # extent past the end
           [0, 0, 5, 15],                 # zero height
           [0, 5, -3, 15],                # negative width
           [0, 5, 5, 14],                 # pitch < 3W
           [-64, 5, 5, 15],               # negative offset
           [1 << 62, 1 << 40, 1 << 40, 1 << 62]]   # products overflow int64
    rows = [p.table[0].tolist()] + bad + [p.table[1].tolist()]
    table = torch.tensor(rows, dtype=torch.int64)
    from dataset.preprocess import validate_table
    with pytest.raises(ValueError):
        validate_table(table, nb)
    out = resize_normalize(p.buffer.cuda(), table, (32, 32), validate=False)
    torch.cuda.synchronize()
    for s in range(1, 1 + len(bad)):
        assert torch.isnan(out[s]).all(), 'slot {} was read'.format(s)
    _check(out[0], ims[0])
    _check(out[-1], ims[1])
