"""The spatio-temporal LSTM cell of PredRNN (models.predrnn) between its convolutions, and the 2 x 2 max pool of the
model's ResNet tail, over the C ABI (csrc/predrnn.hip), f32 NHWC, inference only: the one home of every launch of

    hrnet_sample_stats (+ _scratch), hrnet_stlstm_gates, hrnet_stlstm_out, hrnet_maxpool2d_2x2

Two layers, as hipnet.conv_kxk (whose K x K convolution runs the cell's five convolutions):

  raw launchers: no argument checks beyond the C entry's own (anything it cannot serve is a RuntimeError)
    stats(maps, eps, out)     gates(xc, hc, mc, st, ln, c_t, c_off, m_t, m_off, mem, o_pre, nh)
    out_gate(oc, st, wo, bo, o_pre, last, h_new)     pool(x, y, c, x_off, y_off)

  checked public ops: shapes are checked before any device call, a CPU tensor is a ValueError, a required gradient a
  NotImplementedError
    pack_ln(weight_or_bias)          LayerNorm([C, H, W]) weight or bias (C, H, W) -> (H, W, C), any device
    sample_stats(maps, eps)          up to three dense (B, H, W, C) maps -> (len(maps), B, 2): mean, rstd per sample
    stlstm_gates(xc, hc, mc, stats, ln, c_t, m_t, mem, nh, c_off, m_off)   -> (mem, o_pre)
    stlstm_out(oc, stats, wo, bo, o_pre, last)                             -> h_new
    maxpool2x2(x, c, x_off, out, y_off)
    cell(p, x, x_off, h, c_map, m_map, m_off, xc)                          one cell's launches -> h_new

LAUNCHES_PER_CELL counts what cell() issues: five convolutions, two statistic entries of two kernels each, the two gate
kernels.
"""
import ctypes

import torch

from hipnet import _capi as C
from hipnet import conv_kxk as K
from hipnet import nhwc

EPS = 1e-5                      # nn.LayerNorm's default, which the reference keeps
MAX_MAPS = 3
LAUNCHES_PER_CELL = {'conv_kxk': 5, 'sample_stats': 2, 'sample_stats kernels': 4, 'stlstm_gates': 1, 'stlstm_out': 1,
                     'kernels': 11}


# --------------------------------------------------------------------------------------------------- raw launchers
def stats_scratch_bytes(B, sizes):
    n = list(sizes) + [0] * (MAX_MAPS - len(sizes))
    out = ctypes.c_int64(0)
    C.call('hrnet_sample_stats_scratch', B, n[0], n[1], n[2], ctypes.byref(out))
    return out.value


def stats(maps, eps=EPS, out=None):
    """(len(maps), B, 2) mean and rstd of every sample of each dense map (B, ...)"""
    B = maps[0].shape[0]
    sizes = [m.numel() // B for m in maps]
    nbytes = stats_scratch_bytes(B, sizes)
    scratch = torch.empty(nbytes // 8, dtype=torch.float64, device=maps[0].device)
    if out is None:
        out = torch.empty((len(maps), B, 2), dtype=torch.float32, device=maps[0].device)
    ptrs = [m.data_ptr() for m in maps] + [None] * (MAX_MAPS - len(maps))
    n = sizes + [0] * (MAX_MAPS - len(maps))
    with torch.cuda.device(maps[0].device):
        C.call('hrnet_sample_stats', ptrs[0], ptrs[1], ptrs[2], n[0], n[1], n[2], B, float(eps), scratch.data_ptr(), nbytes,
               out.data_ptr(), C.stream_ptr())
    return out


def gates(xc, hc, mc, st, ln, c_t, c_off, m_t, m_off, mem, o_pre, nh):
    """ln: (wx, bx, wh, bh, wm, bm) of pack_ln"""
    B, H, W, _ = xc.shape
    with torch.cuda.device(xc.device):
        C.call('hrnet_stlstm_gates', xc.data_ptr(), hc.data_ptr(), mc.data_ptr(), st.data_ptr(), ln[0].data_ptr(),
               ln[1].data_ptr(), ln[2].data_ptr(), ln[3].data_ptr(), ln[4].data_ptr(), ln[5].data_ptr(), c_t.data_ptr(),
               c_t.shape[3], c_off, m_t.data_ptr(), m_t.shape[3], m_off, mem.data_ptr(), mem.shape[3], o_pre.data_ptr(), B, H,
               W, nh, C.stream_ptr())
    return mem, o_pre


def out_gate(oc, st, wo, bo, o_pre, last, h_new):
    B, H, W, nh = oc.shape
    with torch.cuda.device(oc.device):
        C.call('hrnet_stlstm_out', oc.data_ptr(), st.data_ptr(), wo.data_ptr(), bo.data_ptr(), o_pre.data_ptr(),
               last.data_ptr(), h_new.data_ptr(), B, H, W, nh, C.stream_ptr())
    return h_new


def pool(x, y, c, x_off, y_off):
    B, H, W, ldx = x.shape
    with torch.cuda.device(x.device):
        C.call('hrnet_maxpool2d_2x2', x.data_ptr(), y.data_ptr(), B, H, W, c, ldx, x_off, y.shape[3], y_off, C.stream_ptr())
    return y


# ---------------------------------------------------------------------------------------------- checked public ops
def _no_grad(name, *ts):
    if nhwc.wants_grad(*ts):
        raise NotImplementedError('{}: backward is not built (this op is inference only): run under '
                                  'torch.no_grad()'.format(name))


def _map(name, key, t, c=None):
    if t.ndim != 4 or t.numel() == 0 or not t.is_contiguous() or (c is not None and t.shape[3] != c):
        raise ValueError('{}: {} {}: expected a contiguous NHWC (B, H, W, {}), nothing empty'.format(
            name, key, tuple(t.shape), 'ld' if c is None else c))


def _slice(name, key, off, c, ld):
    if off < 0 or c < 1 or off + c > ld or off % 4 or c % 4 or ld % 4:
        raise ValueError('{}: {} channels [{}, {} + {}) in a row of {}: expected multiples of 4 and a slice inside the '
                         'row'.format(name, key, off, off, c, ld))


def pack_ln(t):
    """a LayerNorm([C, H, W]) weight or bias (C, H, W) -> contiguous float32 (H, W, C): the layout of the NHWC maps, so the
    cell kernels read the affine along the channel axis. Done once at load; works on any device"""
    if not isinstance(t, torch.Tensor) or t.ndim != 3 or t.numel() == 0:
        raise ValueError('pack_ln: {}: expected a (C, H, W) tensor'.format(
            tuple(t.shape) if isinstance(t, torch.Tensor) else type(t).__name__))
    return t.detach().float().permute(1, 2, 0).contiguous()


def unpack_ln(t):
    """the inverse of pack_ln: (H, W, C) -> (C, H, W)"""
    if not isinstance(t, torch.Tensor) or t.ndim != 3 or t.numel() == 0:
        raise ValueError('unpack_ln: expected a (H, W, C) tensor')
    return t.detach().permute(2, 0, 1).contiguous()


def sample_stats(maps, eps=EPS):
    """per-sample LayerNorm statistics of one to three dense f32 maps (B, H, W, C_m) (any trailing shape whose size is a
    multiple of 4) in ONE entry: (len(maps), B, 2) with [..., 0] = mean, [..., 1] = 1 / sqrt(biased var + eps). Sums are
    double on shifted data, in a fixed order: two calls give equal bits"""
    maps = list(maps)
    if not 1 <= len(maps) <= MAX_MAPS:
        raise ValueError('sample_stats: {} maps: expected one to {}'.format(len(maps), MAX_MAPS))
    nhwc.check('sample_stats', **{'map{}'.format(i): m for i, m in enumerate(maps)})
    B = maps[0].shape[0] if maps[0].ndim else 0
    for i, m in enumerate(maps):
        if m.ndim < 2 or m.numel() == 0 or m.shape[0] != B or not m.is_contiguous() or (m.numel() // B) % 4:
            raise ValueError('sample_stats: map {} {}: expected a contiguous (B = {}, ...) map with a multiple of 4 '
                             'elements per sample'.format(i, tuple(m.shape), B))
        if m.device != maps[0].device:
            raise ValueError('sample_stats: the maps must be on one device')
    if not eps >= 0:
        raise ValueError('sample_stats: eps = {}'.format(eps))
    _no_grad('sample_stats', *maps)
    return stats([m.detach() for m in maps], eps)


def stlstm_gates(xc, hc, mc, stats3, ln, c_t, m_t, mem, nh, c_off=0, m_off=0, o_pre=None):
    """the gates of one cell (see csrc/predrnn.hip): xc (B, H, W, 7 nh), hc (.., 4 nh), mc (.., 3 nh) raw convolution
    outputs, stats3 (3, B, 2) of sample_stats([xc, hc, mc]), ln = (wx, bx, wh, bh, wm, bm) of pack_ln; c_t and m_t maps read
    at channels [c_off, c_off + nh) / [m_off, m_off + nh). Writes c_new to channels [0, nh) and m_new to [nh, 2 nh) of mem
    (B, H, W, ld >= 2 nh) and nothing else of it; c_t / m_t may be mem itself (c_off 0 / m_off nh). -> (mem, o_pre)"""
    nh = int(nh)
    ln = tuple(ln)
    if len(ln) != 6:
        raise ValueError('stlstm_gates: ln: expected (wx, bx, wh, bh, wm, bm)')
    names = ('wx', 'bx', 'wh', 'bh', 'wm', 'bm')
    nhwc.check('stlstm_gates', xc=xc, hc=hc, mc=mc, stats=stats3, c_t=c_t, m_t=m_t, mem=mem, o_pre=o_pre,
               **dict(zip(names, ln)))
    if nh < 4 or nh % 4:
        raise ValueError('stlstm_gates: nh = {}: expected a multiple of 4'.format(nh))
    _map('stlstm_gates', 'xc', xc, 7 * nh)
    B, H, W, _ = xc.shape
    for key, t, k in (('hc', hc, 4), ('mc', mc, 3)):
        _map('stlstm_gates', key, t, k * nh)
        if tuple(t.shape[:3]) != (B, H, W):
            raise ValueError('stlstm_gates: {} {}: expected ({}, {}, {}, {})'.format(key, tuple(t.shape), B, H, W, k * nh))
    if tuple(stats3.shape) != (3, B, 2) or not stats3.is_contiguous():
        raise ValueError('stlstm_gates: stats {}: expected a contiguous (3, {}, 2)'.format(tuple(stats3.shape), B))
    for key, t, k in zip(names, ln, (7, 7, 4, 4, 3, 3)):
        if tuple(t.shape) != (H, W, k * nh) or not t.is_contiguous():
            raise ValueError('stlstm_gates: {} {}: expected a contiguous ({}, {}, {}) of pack_ln'.format(
                key, tuple(t.shape), H, W, k * nh))
    for key, t, off in (('c_t', c_t, int(c_off)), ('m_t', m_t, int(m_off)), ('mem', mem, 0)):
        _map('stlstm_gates', key, t)
        if tuple(t.shape[:3]) != (B, H, W):
            raise ValueError('stlstm_gates: {} {}: expected ({}, {}, {}, ld)'.format(key, tuple(t.shape), B, H, W))
        _slice('stlstm_gates', key, off, 2 * nh if key == 'mem' else nh, t.shape[3])
    if c_t.data_ptr() == mem.data_ptr() and int(c_off) != 0:
        raise ValueError('stlstm_gates: c_t is mem: c_off must be 0, the slice c_new is written to')
    if m_t.data_ptr() == mem.data_ptr() and int(m_off) != nh:
        raise ValueError('stlstm_gates: m_t is mem: m_off must be nh, the slice m_new is written to')
    if o_pre is not None:
        _map('stlstm_gates', 'o_pre', o_pre, nh)
        if tuple(o_pre.shape[:3]) != (B, H, W):
            raise ValueError('stlstm_gates: o_pre {}: expected ({}, {}, {}, {})'.format(tuple(o_pre.shape), B, H, W, nh))
    _no_grad('stlstm_gates', xc, hc, mc, c_t, m_t, mem, *ln)
    if o_pre is None:
        o_pre = torch.empty((B, H, W, nh), dtype=torch.float32, device=xc.device)
    return gates(xc.detach(), hc.detach(), mc.detach(), stats3.detach(), [t.detach() for t in ln], c_t.detach(), int(c_off),
                 m_t.detach(), int(m_off), mem.detach(), o_pre, nh)


def stlstm_out(oc, stats1, wo, bo, o_pre, last, out=None):
    """h_new (B, H, W, nh) = sigmoid(o_pre + LN(oc)) * tanh(last): oc the raw conv_o output, stats1 (1, B, 2) or (B, 2) of
    sample_stats([oc]), wo / bo (H, W, nh) of pack_ln, last the conv_last output"""
    nhwc.check('stlstm_out', oc=oc, stats=stats1, wo=wo, bo=bo, o_pre=o_pre, last=last, out=out)
    _map('stlstm_out', 'oc', oc)
    B, H, W, nh = oc.shape
    if nh % 4:
        raise ValueError('stlstm_out: nh = {}: expected a multiple of 4'.format(nh))
    if stats1.numel() != 2 * B or not stats1.is_contiguous():
        raise ValueError('stlstm_out: stats {}: expected a contiguous ({}, 2)'.format(tuple(stats1.shape), B))
    for key, t in (('wo', wo), ('bo', bo)):
        if tuple(t.shape) != (H, W, nh) or not t.is_contiguous():
            raise ValueError('stlstm_out: {} {}: expected a contiguous ({}, {}, {}) of pack_ln'.format(
                key, tuple(t.shape), H, W, nh))
    for key, t in (('o_pre', o_pre), ('last', last), ('out', out)):
        if t is not None and (tuple(t.shape) != (B, H, W, nh) or not t.is_contiguous()):
            raise ValueError('stlstm_out: {} {}: expected a contiguous ({}, {}, {}, {})'.format(
                key, tuple(t.shape), B, H, W, nh))
    _no_grad('stlstm_out', oc, wo, bo, o_pre, last)
    if out is None:
        out = torch.empty((B, H, W, nh), dtype=torch.float32, device=oc.device)
    return out_gate(oc.detach(), stats1.detach(), wo.detach(), bo.detach(), o_pre.detach(), last.detach(), out)


def maxpool2x2(x, c=None, x_off=0, out=None, y_off=0):
    """MaxPool2d(2, 2) of channels [x_off, x_off + c) of x (B, H, W, ldx), even H and W -> channels [y_off, y_off + c) of out
    (B, H / 2, W / 2, ldy) (None: a new map of c channels); c, the row lengths and offsets multiples of 4"""
    nhwc.check('maxpool2x2', x=x, out=out)
    _map('maxpool2x2', 'x', x)
    B, H, W, ldx = x.shape
    c = ldx - x_off if c is None else int(c)
    x_off, y_off = int(x_off), int(y_off)
    if H % 2 or W % 2:
        raise ValueError('maxpool2x2: x {}: H and W must be even'.format(tuple(x.shape)))
    _slice('maxpool2x2', 'input', x_off, c, ldx)
    if out is not None:
        _map('maxpool2x2', 'out', out)
        if tuple(out.shape[:3]) != (B, H // 2, W // 2):
            raise ValueError('maxpool2x2: out {}: expected ({}, {}, {}, ld)'.format(tuple(out.shape), B, H // 2, W // 2))
        _slice('maxpool2x2', 'output', y_off, c, out.shape[3])
    elif y_off:
        raise ValueError('maxpool2x2: y_off = {} without a map to write into'.format(y_off))
    _no_grad('maxpool2x2', x, out)
    if out is None:
        out = torch.empty((B, H // 2, W // 2, c), dtype=torch.float32, device=x.device)
    return pool(x.detach(), out, c, x_off, y_off)


def cell(p, x, x_off, h, c_map, m_map, m_off, xc=None):
    """one SpatioTemporalLSTMCell step. p: a dict with nh, ks, the packed convolutions 'conv_x', 'conv_h', 'conv_m',
    'conv_o', 'conv_last' as (packed weight, bias, cin) and the six + two pack_ln tensors 'ln' and 'ln_o'.
    x (B, H, W, ldx) read at [x_off, x_off + cin of conv_x); h (B, H, W, nh) the layer's hidden map; c_map (B, H, W, 2 nh)
    the layer's memory map, whose channels [0, nh) hold c_t and which receives (c_new, m_new); m_map / m_off: where m_t is
    read (another layer's memory map at nh, or c_map itself at nh). xc: the conv_x output if it was computed ahead (layer
    0's, for all frames in one launch). Returns h_new (a new map)."""
    nh, ks = p['nh'], p['ks']
    if xc is None:
        w, b, cin = p['conv_x']
        xc = K.conv_kxk(x, w, 7 * nh, ks, bias=b, cin=cin, x_off=x_off)
    w, b, cin = p['conv_h']
    hc = K.conv_kxk(h, w, 4 * nh, ks, bias=b, cin=cin)
    w, b, cin = p['conv_m']
    mc = K.conv_kxk(m_map, w, 3 * nh, ks, bias=b, cin=cin, x_off=m_off)
    st = sample_stats((xc, hc, mc))
    _, o_pre = stlstm_gates(xc, hc, mc, st, p['ln'], c_map, m_map, c_map, nh, c_off=0, m_off=m_off)
    w, b, cin = p['conv_o']
    oc = K.conv_kxk(c_map, w, nh, ks, bias=b, cin=cin)
    w, b, cin = p['conv_last']
    last = K.conv_kxk(c_map, w, nh, 1, bias=b, cin=cin)
    return stlstm_out(oc, sample_stats((oc,)), p['ln_o'][0], p['ln_o'][1], o_pre, last)
