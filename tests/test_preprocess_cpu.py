"""tools/inference.py and its input step on the host (dataset/preprocess.py): PoseAggr frame windows, slot-table
packing and validation, directory listing, PIL decoding to RGB, the two coordinate scalings, argument parsing and
the --sequence resolution. The device kernel is covered by tests/test_preprocess_gpu.py."""
import importlib.util
import os
import sys

import numpy as np
import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(REPO, 'hrnet-hand-pose-estimation_amd')
TOOLS = os.path.join(PKG, 'tools')


def _tool():
    if TOOLS not in sys.path:
        sys.path.insert(0, TOOLS)
    spec = importlib.util.spec_from_file_location('hrnet_inference_tool', os.path.join(TOOLS, 'inference.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _cfg(yaml, *opts):
    from config import get_cfg_defaults
    c = get_cfg_defaults()
    c.merge_from_file(os.path.join(PKG, 'experiments', yaml))
    c.merge_from_list(list(opts))
    return c


# ---------------------------------------------------------------- sequence_windows

def test_sequence_windows_layout_in_the_middle():
    from dataset.preprocess import sequence_windows
    w = sequence_windows(20, 5, 3)
    assert w.dtype == np.int64 and w.shape == (15,)
    # [prev2 | prev1 | current | next1 | next2], each block 3 long
    assert w.reshape(5, 3).tolist() == [[3, 4, 5], [4, 5, 6], [5, 6, 7], [6, 7, 8], [7, 8, 9]]


def test_sequence_windows_clamp_at_both_ends():
    from dataset.preprocess import sequence_windows
    assert sequence_windows(7, 0, 7).reshape(5, 7).tolist() == [
        [0, 0, 0, 1, 2, 3, 4], [0, 0, 1, 2, 3, 4, 5], [0, 1, 2, 3, 4, 5, 6], [1, 2, 3, 4, 5, 6, 6], [2, 3, 4, 5, 6, 6, 6]]
    assert sequence_windows(1, 0, 1).tolist() == [0] * 5


def test_sequence_windows_batches_cover_a_sequence_like_one_batch():
    from dataset.preprocess import sequence_windows
    whole = sequence_windows(10, 0, 10).reshape(5, 10)
    parts = [sequence_windows(10, c0, min(4, 10 - c0)).reshape(5, -1) for c0 in range(0, 10, 4)]
    # a batch boundary inside the sequence: frames 3|4 and 7|8 still see their true neighbours
    assert np.array_equal(np.concatenate(parts, axis=1), whole)
    assert parts[1].tolist() == [[2, 3, 4, 5], [3, 4, 5, 6], [4, 5, 6, 7], [5, 6, 7, 8], [6, 7, 8, 9]]


@pytest.mark.parametrize('args', [(0, 0, 1), (5, 3, 3), (5, -1, 2), (5, 0, 0)])
def test_sequence_windows_rejects_frames_outside_the_sequence(args):
    from dataset.preprocess import sequence_windows
    with pytest.raises(ValueError):
        sequence_windows(*args)


# ---------------------------------------------------------------- packing and host validation

def test_pack_images_one_buffer_and_its_table():
    from dataset.preprocess import pack_images, validate_table
    rng = np.random.default_rng(0)
    ims = [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for h, w in ((5, 7), (1, 1), (3, 64), (9, 2))]
    p = pack_images(ims, pin=False, align=64)
    assert p.buffer.dtype == torch.uint8 and p.buffer.dim() == 1
    assert p.table.dtype == torch.int64 and tuple(p.table.shape) == (4, 4)
    assert p.sizes == [(5, 7), (1, 1), (3, 64), (9, 2)]
    assert all(o % 64 == 0 for o in p.offsets) and p.table[:, 0].tolist() == p.offsets
    assert p.table[:, 3].tolist() == [3 * w for _, w in p.sizes]
    flat = p.buffer.numpy()
    for im, (off, h, w, pitch) in zip(ims, p.table.tolist()):
        got = flat[off:off + (h - 1) * pitch + 3 * w].reshape(h, w, 3)
        assert np.array_equal(got, im)
    validate_table(p.table, p.buffer.numel())
    # a reused staging buffer that is large enough is sliced, not reallocated
    q = pack_images(ims[:2], pin=False, staging=p.buffer)
    assert q.buffer.data_ptr() == p.buffer.data_ptr() and q.buffer.numel() < p.buffer.numel()


@pytest.mark.parametrize('row,msg', [([0, 4, 5, 14], 'pitch'),          # pitch < 3W
                                     ([0, 0, 5, 15], 'empty'),          # zero height
                                     ([0, 4, 0, 15], 'empty'),          # zero width
                                     ([90, 4, 5, 15], 'exceed'),        # 90 + 3*15 + 15 > 100
                                     ([-1, 1, 1, 3], 'exceed'),
                                     ([2 ** 40, 1, 1, 3], 'exceed')])
def test_validate_table_rejects_bad_rows(row, msg):
    from dataset.preprocess import validate_table
    validate_table(torch.tensor([[0, 4, 5, 15], [40, 4, 5, 15]]), 100)     # last byte 40 + 45 + 15 = 100: fits
    with pytest.raises(ValueError, match=msg):
        validate_table(torch.tensor([[0, 4, 5, 15], row]), 100)


def test_pack_images_rejects_non_rgb_u8():
    from dataset.preprocess import pack_images
    with pytest.raises(ValueError):
        pack_images([np.zeros((4, 4), np.uint8)], pin=False)
    with pytest.raises(ValueError):
        pack_images([np.zeros((4, 4, 3), np.float32)], pin=False)
    with pytest.raises(ValueError):
        pack_images([], pin=False)


def test_resize_normalize_refuses_host_tensors():
    from dataset.preprocess import pack_images, resize_normalize
    p = pack_images([np.zeros((4, 4, 3), np.uint8)], pin=False)
    with pytest.raises(RuntimeError, match='HIP device'):
        resize_normalize(p.buffer, p.table, (256, 256))


# ---------------------------------------------------------------- inputs

def _png(path, mode, size=(6, 4)):
    from PIL import Image
    rng = np.random.default_rng(len(str(path)))
    if mode == 'L':
        im = Image.fromarray(rng.integers(0, 256, size[::-1], dtype=np.uint8), 'L')
    elif mode == 'RGBA':
        im = Image.fromarray(rng.integers(0, 256, size[::-1] + (4,), dtype=np.uint8), 'RGBA')
    elif mode == 'P':
        im = Image.fromarray(rng.integers(0, 256, size[::-1] + (3,), dtype=np.uint8), 'RGB').quantize(colors=8)
    else:
        im = Image.fromarray(rng.integers(0, 256, size[::-1] + (3,), dtype=np.uint8), 'RGB')
    im.save(str(path))
    return im


def test_list_images_is_sorted_and_skips_other_entries(tmp_path):
    from dataset.preprocess import list_images
    for n in ('b.png', 'a.JPG', 'c.jpeg', 'd.bmp', '10.png', '2.png'):
        (tmp_path / n).write_bytes(b'x')
    (tmp_path / 'clip.mp4').write_bytes(b'x')
    (tmp_path / 'notes.txt').write_text('x')
    (tmp_path / 'sub.png').mkdir()
    (tmp_path / 'sub').mkdir()
    got = [os.path.basename(p) for p in list_images(str(tmp_path))]
    assert got == ['10.png', '2.png', 'a.JPG', 'b.png', 'c.jpeg', 'd.bmp']


@pytest.mark.parametrize('mode', ['L', 'RGBA', 'P', 'RGB'])
def test_read_image_rgb(tmp_path, mode):
    from dataset.preprocess import read_image_rgb
    path = tmp_path / 'im.png'
    im = _png(path, mode, size=(6, 4))
    got = read_image_rgb(str(path))
    assert got.dtype == np.uint8 and got.shape == (4, 6, 3) and got.flags['C_CONTIGUOUS']
    if mode == 'L':                                   # grey replicated to three channels
        g = np.asarray(im)
        assert all(np.array_equal(got[..., c], g) for c in range(3))
    elif mode == 'RGBA':                              # alpha dropped, not blended
        assert np.array_equal(got, np.asarray(im)[..., :3])
    elif mode == 'P':                                 # palette expanded
        assert np.array_equal(got, np.asarray(im.convert('RGB')))
    else:
        assert np.array_equal(got, np.asarray(im))


def test_collect_inputs(tmp_path):
    tool = _tool()
    (tmp_path / 'f1.png').write_bytes(b'x')
    (tmp_path / 'f0.png').write_bytes(b'x')
    (tmp_path / 'v.mp4').write_bytes(b'x')
    assert [os.path.basename(p) for p in tool.collect_inputs(str(tmp_path))] == ['f0.png', 'f1.png']
    assert tool.collect_inputs(str(tmp_path / 'f1.png')) == [str(tmp_path / 'f1.png')]
    with pytest.raises(SystemExit, match='no video decoder'):
        tool.collect_inputs(str(tmp_path / 'v.mp4'))
    empty = tmp_path / 'empty'
    empty.mkdir()
    with pytest.raises(SystemExit):
        tool.collect_inputs(str(empty))
    with pytest.raises(SystemExit):
        tool.collect_inputs(str(tmp_path / 'missing.png'))


# ---------------------------------------------------------------- coordinates

def test_coordinate_scaling_of_both_output_files():
    tool = _tool()
    c = _cfg(os.path.join('RHD', 'RHD_HRNet_w32_max_hmloss_v1.yaml'))
    assert (c.MODEL.IMAGE_SIZE[0], c.MODEL.HEATMAP_SIZE[0]) == (256, 64)
    preds = np.array([[[1.0, 2.0], [63.0, 0.5]], [[10.0, 20.0], [0.0, 64.0]]], dtype=np.float32)   # (N=2, K=2, 2)
    inp = tool.to_input_pixels(preds, c)
    assert inp.dtype == np.float64 and inp.shape == (4, 2)
    assert np.array_equal(inp, preds.reshape(-1, 2).astype(np.float64) * 4.0)
    # original image pixels: x * W / 64, y * H / 64 (the reference's HEATMAP_SIZE[0] for both axes)
    img = tool.to_image_pixels(preds, [(480, 640), (100, 30)], c)
    want = np.array([[1 * 10.0, 2 * 7.5], [63 * 10.0, 0.5 * 7.5], [10 * 30 / 64, 20 * 100 / 64], [0.0, 64 * 100 / 64]])
    np.testing.assert_allclose(img, want, rtol=0, atol=1e-12)


# ---------------------------------------------------------------- arguments

def test_argument_parsing_accepts_the_reference_flags():
    tool = _tool()
    a = tool.parse_args(['--cfg', 'x.yaml', '--gpu', '-1', '--world-size', '4', '--model_path', 'm.pth.tar',
                         '--image_path', 'imgs', 'MODEL.HEATMAP_SOFTMAX', 'True'])
    assert (a.cfg, a.gpu, a.world_size, a.model_path, a.image_path) == ('x.yaml', -1, 4, 'm.pth.tar', 'imgs')
    assert a.opts == ['MODEL.HEATMAP_SOFTMAX', 'True']
    assert (a.batch_size, a.output, a.vis, a.sequence) == (32, '.', 0, 'auto')
    b = tool.parse_args(['--cfg', 'x.yaml', '--image_path', 'i.png', '--batch_size', '4', '--output', 'o', '--vis', '1',
                         '--sequence', 'off'])
    assert (b.batch_size, b.output, b.vis, b.sequence, b.opts) == (4, 'o', 1, 'off', [])
    for bad in (['--vis', '2'], ['--sequence', 'maybe'], ['--batch_size', '0']):
        with pytest.raises(SystemExit):
            tool.parse_args(['--cfg', 'x.yaml', '--image_path', 'i.png'] + bad)


def test_sequence_auto_follows_the_config():
    tool = _tool()
    aggr = os.path.join('MHP', 'MHP_HRNet_w32_trainable_softmax_pose2dloss_PoseAggr_v1.yaml')
    plain = os.path.join('RHD', 'RHD_HRNet_w32_max_hmloss_v1.yaml')
    assert tool.resolve_sequence(_cfg(aggr), 'auto') is True
    assert tool.resolve_sequence(_cfg(aggr), 'on') is True
    assert tool.resolve_sequence(_cfg(aggr, 'MODEL.USE_WARPING_TEST', 'False'), 'auto') is False
    assert tool.resolve_sequence(_cfg(plain), 'auto') is False
    assert tool.resolve_sequence(_cfg(plain), 'off') is False
    with pytest.raises(SystemExit):
        tool.resolve_sequence(_cfg(plain), 'on')          # only PoseAggr consumes 5-frame windows
    with pytest.raises(SystemExit):
        tool.resolve_sequence(_cfg(aggr), 'off')


def test_checkpoint_load_non_strict(tmp_path):
    from core.evaluate2d import load_checkpoint_state
    m = torch.nn.Sequential(torch.nn.Linear(2, 3), torch.nn.Linear(3, 1))
    sd = {'module.' + k: torch.full_like(v, 0.5) for k, v in m.state_dict().items() if k.startswith('0.')}
    sd['module.extra'] = torch.zeros(1)
    torch.save({'state_dict': sd, 'epoch': 7}, str(tmp_path / 'c.pth.tar'))
    info = {}
    load_checkpoint_state(m, str(tmp_path / 'c.pth.tar'), strict=False, info=info)
    assert float(m[0].weight.detach()[0, 0]) == 0.5
    assert sorted(info['missing']) == ['1.bias', '1.weight'] and info['unexpected'] == ['extra'] and info['epoch'] == 7
    with pytest.raises(RuntimeError):                   # the default stays strict (tools/evaluate_2D.py)
        load_checkpoint_state(m, str(tmp_path / 'c.pth.tar'))
    torch.save({'other.weight': torch.zeros(1)}, str(tmp_path / 'none.pth.tar'))
    with pytest.raises(ValueError, match='none of'):
        load_checkpoint_state(m, str(tmp_path / 'none.pth.tar'), strict=False)
