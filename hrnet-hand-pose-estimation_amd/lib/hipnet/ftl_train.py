"""The backward of FTLMultiviewNet's head over the C ABI, f32 NHWC (csrc/ftl_train.hip): the one home of every launch of

    hrnet_ftl_gather_bwd, hrnet_ftl_scatter_bwd, hrnet_conv2d_3x3g_wgrad_scratch, hrnet_conv2d_3x3g_wgrad

The forward ops stay in hipnet.ftl (inference only, refusals included); this module adds the gradients beside them and
the autograd node of the head (head_forward_train / head_backward / HeadFn, used by models.FTL_encoder_decoder). Every
op reads and writes channel slices (ld, off, C) of wider maps, uses no atomics and sums in a fixed order: two runs from
the same state give equal bits. Two layers, as hipnet.ftl:

  raw launchers: no argument checks beyond the C entry's own (anything it cannot serve is a RuntimeError)
    gather_bwd_raw(dcat, coef, dx, B, V, c, d_off, slice, x_off)    scatter_bwd_raw(dy, coef, df, B, V, c, y_off, f_off)
    wgrad_plan(N, Ho, Wo, cin, cout)            (scratch bytes, pixel-tile splits, tiles per split): a host query
    wgrad(x, dy, scratch, dw, cin, cin_real, x_off, cout, y_off, stride, pad_lo)

  checked public ops: shapes are checked before any device call, a CPU tensor is a ValueError
    gather_bwd(dcat, coef, V, c, d_off, slice, out, x_off)      (B, h, w, ldd) -> (B V, h, w, ldx), dx = d A^T
    scatter_bwd(dy, coef, V, c, y_off, out, f_off)              (B V, h, w, ldy) -> (B, h, w, ldf), df = sum_v d A^T
    conv3x3g_wgrad(x, dy, cout, stride, pad_lo, ...)            -> dW (cout, cin_real, 3, 3)
    pack_dgrad(weight)                          the weights with which hipnet.ftl.conv IS the data gradient of
                                                Conv2d(3, 2, 2): conv(dy, ., stride 1, pad_lo 0, z 2, Ho = H_in)
    pack_dgrad_transpose(weight)                the same for ConvTranspose2d(3, 2, 2, op): conv(dy, ., stride 2, pad_lo 2,
                                                z 1, Ho = H_in)

The two identities (tests/test_ftl_train_ops_gpu.py holds them against autograd):
  y = Conv2d(3, stride 2, padding 2)(x), weight W (Co, Ci, 3, 3):  dx[i] = sum_{o, k: 2 o + k - 2 = i} dy[o] W[k]. Read dy
    zero-stuffed by 2 (dyz[2 o] = dy[o]): dx[i] = sum_k dyz[i + 2 - k] W[k] = sum_k' dyz[i + k'] W[2 - k'], a stride-1
    convolution of the stuffed map with pad_lo 0 and the flipped, transposed weight - nhwc.conv_transpose_pack(W). Its
    size range for H_o rows is 2 H_o - 3 .. 2 H_o - 1, which holds every H_in with (H_in + 1) // 2 + 1 = H_o.
  y = ConvTranspose2d(3, 2, 2, op)(x), weight W (Ci, Co, 3, 3):  y[2 i + k - 2] += x[i] W[k], so dx[i] = sum_k
    dy[2 i + k - 2] W[k]: the stride-2, pad_lo-2 convolution of dy with W read as (Co -> Ci), nhwc.conv_pack of W
    permuted to (Ci, Co, 3, 3) = W as it stands in Conv2d's (out, in) order.
"""
import ctypes

import torch

from hipnet import _capi as C
from hipnet import conv_kxk as KX
from hipnet import ftl as FT
from hipnet import nhwc

F32 = C.HR_F32


# --------------------------------------------------------------------------------------------------- raw launchers
def gather_bwd_raw(dcat, coef, dx, B, V, c, d_off, slice_, x_off):
    _, H, W, ldd = dcat.shape
    with torch.cuda.device(dcat.device):
        C.call('hrnet_ftl_gather_bwd', dcat.data_ptr(), coef.data_ptr(), dx.data_ptr(), B, V, H, W, c, ldd, d_off, slice_,
               dx.shape[3], x_off, C.stream_ptr())
    return dx


def scatter_bwd_raw(dy, coef, df, B, V, c, y_off, f_off):
    _, H, W, ldy = dy.shape
    with torch.cuda.device(dy.device):
        C.call('hrnet_ftl_scatter_bwd', dy.data_ptr(), coef.data_ptr(), df.data_ptr(), B, V, H, W, c, ldy, y_off,
               df.shape[3], f_off, C.stream_ptr())
    return df


def wgrad_plan(N, Ho, Wo, cin, cout):
    """(bytes of scratch, pixel-tile splits, 8 x 16 output-pixel tiles per split) of hrnet_conv2d_3x3g_wgrad"""
    nbytes, nsplit, per = ctypes.c_int64(0), ctypes.c_int(0), ctypes.c_int64(0)
    C.call('hrnet_conv2d_3x3g_wgrad_scratch', F32, N, Ho, Wo, cin, cout, ctypes.byref(nbytes), ctypes.byref(nsplit),
           ctypes.byref(per))
    return nbytes.value, nsplit.value, per.value


def wgrad(x, dy, scratch, dw, cin, cin_real, x_off, cout, y_off, stride, pad_lo):
    N, H, W, ldx = x.shape
    with torch.cuda.device(x.device):
        C.call('hrnet_conv2d_3x3g_wgrad', F32, x.data_ptr(), dy.data_ptr(), scratch.data_ptr(),
               scratch.numel() * scratch.element_size(), dw.data_ptr(), N, H, W, cin, cin_real, ldx, x_off, cout,
               dy.shape[3], y_off, dy.shape[1], dy.shape[2], stride, pad_lo, C.stream_ptr())
    return dw


# ---------------------------------------------------------------------------------------------- checked public ops
def gather_bwd(dcat, coef, V, c, d_off=0, slice=None, out=None, x_off=0):
    """the backward of ftl.gather: dcat (B, h, w, ldd), the gradient of the concatenated map, view v read at channels
    [d_off + v slice, d_off + v slice + c) (slice: default c) -> (B V, h, w, ldx) in slot order b V + v, written at
    [x_off, x_off + c) (out: default a new (B V, h, w, c) map). coef: the gather coefficients of ftl.affines()"""
    name = 'ftl_train.gather_bwd'
    d_off, x_off, c, V = int(d_off), int(x_off), int(c), int(V)
    nhwc.check(name, dcat=dcat, coef=coef, out=out)
    slice_ = c if slice is None else int(slice)
    if c < 1 or slice_ < c or slice_ % 4 or V < 1:
        raise ValueError('{}: c = {}, slice = {}, V = {}: expected a slice that is a multiple of 4 and holds c'.format(
            name, c, slice_, V))
    B, _, H, W, _ = FT._transform_args(name, dcat, coef, V, (V - 1) * slice_ + c, d_off, lambda v: 1)
    if c % 4:
        raise ValueError('{}: c = {}: expected multiples of 4'.format(name, c))
    FT._transform_out(name, out, (B * V, H, W), x_off, c)
    if out is None:
        out = torch.empty((B * V, H, W, c), dtype=torch.float32, device=dcat.device)
    return gather_bwd_raw(dcat.detach(), coef.detach(), out, B, V, c, d_off, slice_, x_off)


def scatter_bwd(dy, coef, V, c=None, y_off=0, out=None, f_off=0):
    """the backward of ftl.scatter: dy (B V, h, w, ldy) in slot order, read at [y_off, y_off + c) -> (B, h, w, ldf)
    written at [f_off, f_off + c) (out: default a new (B, h, w, c) map): the views added in order. coef: the scatter
    coefficients of ftl.affines()"""
    name = 'ftl_train.scatter_bwd'
    y_off, f_off = int(y_off), int(f_off)
    nhwc.check(name, dy=dy, coef=coef, out=out)
    B, V, H, W, c = FT._transform_args(name, dy, coef, V, c, y_off, lambda v: v)
    FT._transform_out(name, out, (B, H, W), f_off, c)
    if out is None:
        out = torch.empty((B, H, W, c), dtype=torch.float32, device=dy.device)
    return scatter_bwd_raw(dy.detach(), coef.detach(), out, B, V, c, y_off, f_off)


def conv3x3g_wgrad(x, dy, cout, stride, pad_lo, cin=None, cin_real=None, x_off=0, y_off=0, scratch=None, dw=None):
    """the weight gradient of y = conv3x3g(x, ., cout, stride, pad_lo, z = 1, out_hw = dy's size): x (N, H, W, ldx) read
    at channels [x_off, x_off + cin) (cin, ldx, x_off multiples of 4; default: the whole row) of which the first cin_real
    (default cin) are real, dy (N, Ho, Wo, ldy) read at [y_off, y_off + cout). Returns dW (cout, cin_real, 3, 3), a new
    tensor unless dw is given (overwritten). scratch: a float32 tensor of at least wgrad_plan(...)[0] bytes, None for a
    new one. With x := the output gradient and dy := the input of a ConvTranspose2d(3, 2, 2, op), stride 2 and pad_lo 2,
    the result is that layer's weight gradient in its own (Cin, Cout, 3, 3) layout"""
    name = 'conv3x3g_wgrad'
    nhwc.check(name, x=x, dy=dy, scratch=scratch, dw=dw)
    KX._map(name, 'x', x)
    KX._map(name, 'dy', dy)
    N, H, W, ldx = x.shape
    stride, pad_lo, _ = FT._geometry(name, stride, pad_lo, 1)
    cout, x_off, y_off = int(cout), int(x_off), int(y_off)
    cin = ldx - x_off if cin is None else int(cin)
    cin_real = cin if cin_real is None else int(cin_real)
    KX._slice(name, 'input', x_off, cin, ldx)
    if cin % 4 or ldx % 4 or x_off % 4:
        raise ValueError('{}: cin = {}, ldx = {}, x_off = {}: expected multiples of 4'.format(name, cin, ldx, x_off))
    if not 1 <= cin_real <= cin:
        raise ValueError('{}: {} real input channels of {}'.format(name, cin_real, cin))
    if dy.shape[0] != N:
        raise ValueError('{}: dy {}: expected {} maps'.format(name, tuple(dy.shape), N))
    Ho, Wo = dy.shape[1:3]
    for key, n, o in (('Ho', H, Ho), ('Wo', W, Wo)):
        lo, hi = FT.size_range(n, stride, pad_lo, 1)
        if not lo <= o <= hi:
            raise ValueError('{}: {} = {}: {} inputs with stride = {}, pad_lo = {} give {} .. {}'.format(
                name, key, o, n, stride, pad_lo, lo, hi))
    KX._slice(name, 'gradient', y_off, cout, dy.shape[3])
    nbytes = wgrad_plan(N, Ho, Wo, cin, cout)[0]
    if scratch is None:
        scratch = torch.empty(nbytes // 4, dtype=torch.float32, device=x.device)
    elif not scratch.is_contiguous() or scratch.numel() * 4 < nbytes:
        raise ValueError('{}: scratch of {} bytes, {} needed'.format(name, scratch.numel() * 4, nbytes))
    if dw is None:
        dw = torch.empty((cout, cin_real, 3, 3), dtype=torch.float32, device=x.device)
    elif tuple(dw.shape) != (cout, cin_real, 3, 3) or not dw.is_contiguous():
        raise ValueError('{}: dw {}: expected a contiguous ({}, {}, 3, 3)'.format(name, tuple(dw.shape), cout, cin_real))
    return wgrad(x.detach(), dy.detach(), scratch, dw, cin, cin_real, x_off, cout, y_off, stride, pad_lo)


def pack_dgrad(weight, cout_pad=None):
    """the packed weights with which ftl.conv(dy, ., stride 1, pad_lo 0, z 2, Ho = H_in) is the data gradient of
    Conv2d(Ci, Co, 3, stride 2, padding 2), weight (Co, Ci, 3, 3): nhwc.conv_transpose_pack of it, [pad16(Ci)][9 flipped]
    [cout_pad]; cout_pad (default Co rounded up to 4) is the width of the dy slice read, zeros in the padding"""
    nhwc.check('ftl_train.pack_dgrad', weight=weight)
    if weight.ndim != 4 or tuple(weight.shape[2:]) != (3, 3):
        raise ValueError('ftl_train.pack_dgrad: weight {}: expected (Cout, Cin, 3, 3)'.format(tuple(weight.shape)))
    co, ci = weight.shape[:2]
    cout_pad = (co + 3) // 4 * 4 if cout_pad is None else int(cout_pad)
    # conv_transpose_pack reads (Cin_T, Cout_T, 3, 3) with Cin_T the channels of the map convolved: here dy's Co
    return nhwc.conv_transpose_pack(weight.detach().contiguous(), cout_pad, None)


def pack_dgrad_transpose(weight, cout_pad=None):
    """the packed weights with which ftl.conv(dy, ., stride 2, pad_lo 2, z 1, Ho = H_in) is the data gradient of
    ConvTranspose2d(Ci, Co, 3, stride 2, padding 2, output_padding), weight (Ci, Co, 3, 3): nhwc.conv_pack of it as it
    stands, [pad16(Ci)][9][cout_pad]; cout_pad (default Co rounded up to 4): the width of the dy slice read"""
    nhwc.check('ftl_train.pack_dgrad_transpose', weight=weight)
    if weight.ndim != 4 or tuple(weight.shape[2:]) != (3, 3):
        raise ValueError('ftl_train.pack_dgrad_transpose: weight {}: expected (Cin, Cout, 3, 3)'.format(tuple(weight.shape)))
    ci, co = weight.shape[:2]
    cout_pad = (co + 3) // 4 * 4 if cout_pad is None else int(cout_pad)
    return nhwc.conv_pack(weight.detach().contiguous(), cout_pad, None)


# ------------------------------------------------------------------------------------- the head as one autograd node
HEAD_MODULES = ('encoder_head', 'fuse_after_FTL', 'channel_expansion', 'decoder', 'final_layer')


class HeadFlat(object):
    """flat f32 parameters and gradients of a trainable FTLMultiviewNet's HEAD in parameter order (the backbone is frozen
    and stays outside): the interface hipnet.optim.FlatAdam steps. Every head parameter becomes a view of flat_p; a
    backward pass OVERWRITES flat_g and publishes its slices as the parameters' .grad"""

    def __init__(self, model):
        self.model = model
        named = [(n, p) for m in HEAD_MODULES for n, p in getattr(model, m).named_parameters(prefix=m)]
        self.names, self.params = [n for n, _ in named], [p for _, p in named]
        dev = self.params[0].device
        total = sum(p.numel() for p in self.params)
        self.trainable_count = total
        self.flat_p = torch.empty(total, dtype=torch.float32, device=dev)
        self.flat_g = torch.zeros(total, dtype=torch.float32, device=dev)
        self.offsets, off = {}, 0
        for p in self.params:
            n = p.numel()
            self.flat_p[off:off + n].copy_(p.detach().reshape(-1))
            p.data = self.flat_p[off:off + n].view(p.shape)
            self.offsets[id(p)] = (off, n)
            off += n
        # what ties the heat maps to autograd's graph: its "gradient" is never used, the real ones go to flat_g
        self.anchor = torch.zeros(1, dtype=torch.float32, device=dev, requires_grad=True)
        self._scratch = None

    def grad_of(self, p):
        off, n = self.offsets[id(p)]
        return self.flat_g[off:off + n]

    def scratch(self, nbytes, dev):
        if self._scratch is None or self._scratch.numel() * 4 < nbytes:
            self._scratch = torch.empty((nbytes + 3) // 4, dtype=torch.float32, device=dev)
        return self._scratch

    def publish(self):
        for p in self.params:
            off, n = self.offsets[id(p)]
            p.grad = self.flat_g[off:off + n].view(p.shape)

    def mark_weights_dirty(self):
        self.model._dirty += 1

    def layout(self):
        return [(name, self.offsets[id(p)][0], p.numel()) for name, p in zip(self.names, self.params)]

    def param_order(self):
        return list(self.names)


def _wide(n, h, w, c, dev):
    """a map that a batch-statistic BatchNorm reads or whose gradient it reads: the BatchNorm entries take rows of a multiple
    of 16 channels of which the first c are real, the pad channels zero on the way in (the convolutions and transforms
    write the real ones only)"""
    cp = nhwc.pad16(c)
    make = torch.empty if cp == c else torch.zeros
    return make((n, h, w, cp), dtype=torch.float32, device=dev)


def _softmax_fwd(z, temp):
    out = torch.empty_like(z)
    with torch.cuda.device(z.device):
        C.call('hrnet_spatial_softmax_fwd', z.data_ptr(), temp.data_ptr(), out.data_ptr(), z.shape[0] * z.shape[1],
               z.shape[2] * z.shape[3], C.stream_ptr())
    return out


def _softmax_bwd(z, out, gout, temp):
    dz = torch.empty_like(z)
    part = torch.empty(z.shape[0] * z.shape[1], dtype=torch.float32, device=z.device)
    with torch.cuda.device(z.device):
        C.call('hrnet_spatial_softmax_bwd', z.data_ptr(), out.data_ptr(), gout.data_ptr(), temp.data_ptr(), dz.data_ptr(),
               part.data_ptr(), z.shape[0] * z.shape[1], z.shape[2] * z.shape[3], C.stream_ptr())
    return dz


def head_forward_train(model, features, extrinsic, intrinsic):
    """the head of a trainable FTLMultiviewNet on BATCH statistics: every conv + BatchNorm + ReLU is the raw-weight
    convolution with its bias and no ReLU, then nhwc.bn_batch_forward (which updates the running statistics with the
    module's momentum). Returns the heat maps (B V, K, h, w) as the output of HeadFn; the activations stay on model.tape"""
    flat = model.hip()
    with torch.no_grad():
        BV, _, h, w = features.shape
        V, C_, C2, K = model.num_views, model.in_channel, model.mid, model.num_joints
        B = BV // V
        D = model.decoder.layer_lst[0][0].weight.shape[1]
        dev = features.device
        cin = nhwc.pad16(C_)
        new = lambda *shape: torch.empty(shape, dtype=torch.float32, device=dev)
        wide = lambda n, hh, ww, c: _wide(n, hh, ww, c, dev)
        h1, w1 = FT.out_size(h, 2, 2), FT.out_size(w, 2, 2)
        h2, w2 = FT.out_size(h1, 2, 2), FT.out_size(w1, 2, 2)
        ha, wa = FT.out_size(h2, 1, 0, 2, 0), FT.out_size(w2, 1, 0, 2, 0)
        hb, wb = FT.out_size(ha, 1, 0, 2, 1), FT.out_size(wa, 1, 0, 2, 1)
        t = {'dims': (B, V, h, w, h1, w1, h2, w2, ha, wa, hb, wb, cin)}

        def bn(name, z, seq):
            y, vec, scratch = nhwc.bn_batch_forward(z, seq[1].weight, seq[1].bias, seq[1], seq[1].num_features, True)
            t[name] = (z, y, vec, scratch)
            return y

        def conv3(name, x, seq, ci, co, out_hw):
            z = FT.conv(x, nhwc.conv_pack(seq[0].weight.detach(), ci, None), seq[0].bias.detach(), wide(BV, out_hw[0], out_hw[1], co),
                        ci, 0, co, 0, 2, 2, 1, False)
            return bn(name, z, seq)

        def conv1(name, x, seq, ci, co):
            z = KX.conv(x, nhwc.conv_pack(seq[0].weight.detach(), ci, None), seq[0].bias.detach(),
                        wide(x.shape[0], x.shape[1], x.shape[2], co), ci, 0, co, 0, 1, False)
            return bn(name, z, seq)

        def tconv(name, x, seq, ci, co, out_hw):
            z = FT.conv(x, nhwc.conv_transpose_pack(seq[0].weight.detach(), ci, None), seq[0].bias.detach(),
                        wide(BV, out_hw[0], out_hw[1], co), ci, 0, co, 0, 1, 0, 2, False)
            return bn(name, z, seq)

        x0 = t['x0'] = nhwc.to_nhwc(features.detach().float(), cin)
        y = conv3('enc0', x0, model.encoder_head.layer_lst[0], cin, C_, (h1, w1))
        y = conv3('enc1', y, model.encoder_head.layer_lst[1], C_, C2, (h2, w2))
        coef_g, coef_s = t['coef'] = FT.affines(extrinsic.to(dev), intrinsic)
        cat = t['cat'] = FT.gather_raw(y, coef_g, new(B, h2, w2, V * C2), B, V, C2, 0, 0, C2)
        y = conv1('fuse0', cat, model.fuse_after_FTL.layer_lst[0], V * C2, C2)
        y = conv1('fuse1', y, model.fuse_after_FTL.layer_lst[1], C2, C2)
        s = t['scat'] = FT.scatter_raw(y, coef_s, new(BV, h2, w2, C2), B, V, C2, 0, 0)
        y = conv1('expand', s, model.channel_expansion.layer_lst[0], C2, C_)
        y = tconv('dec0', y, model.decoder.layer_lst[0], C_, D, (ha, wa))
        y = tconv('dec1', y, model.decoder.layer_lst[1], D, D, (hb, wb))
        # decoder.layer_lst.2 and final_layer have nothing between them: one 3x3 convolution D -> K, exact in training too
        last, fin = model.decoder.layer_lst[2], model.final_layer
        wf = fin.weight.detach().reshape(K, D)
        w_out = t['w_out'] = torch.einsum('km,mcrs->kcrs', wf, last.weight.detach()).contiguous()
        b_out = (wf @ last.bias.detach() + fin.bias.detach()).contiguous()
        logits = FT.conv(y, nhwc.conv_pack(w_out, D, None), b_out, new(BV, hb, wb, nhwc.pad16(K)), D, 0, K, 0, 1, 1, 1, False)
        z = t['logits'] = nhwc.nhwc_to_nchw(logits, K)
        t['temp'] = torch.ones(1, dtype=torch.float32, device=dev)
        hm = t['hm'] = _softmax_fwd(z, t['temp'])
    model.tape = t
    model._dirty += 1               # the running statistics moved through their pointers: the folded weights are stale
    return HeadFn.apply(model, flat.anchor, hm)


def head_backward(model, ghm):
    """from the heat maps' gradient (B V, K, h, w) to flat_g of every head parameter; no torch convolution in between"""
    from hipnet import conv_kxk_train as KT
    flat, t = model.hip(), model.tape
    B, V, h, w, h1, w1, h2, w2, ha, wa, hb, wb, cin = t['dims']
    BV = B * V
    C_, C2, K = model.in_channel, model.mid, model.num_joints
    D = model.decoder.layer_lst[0][0].weight.shape[1]
    dev = ghm.device
    new = lambda *shape: torch.empty(shape, dtype=torch.float32, device=dev)
    wide = lambda n, hh, ww, c: _wide(n, hh, ww, c, dev)
    G = flat.grad_of
    K4 = (K + 3) // 4 * 4

    def bn_bwd(name, gy, seq):
        z, y, vec, scratch = t[name]
        dz, dgamma, dbeta, dbias = nhwc.bn_batch_backward(gy, z, y, vec, scratch, seq[1].num_features, True, True, True)
        G(seq[1].weight).copy_(dgamma)
        G(seq[1].bias).copy_(dbeta)
        G(seq[0].bias).copy_(dbias)
        return dz

    def kxk_wgrad(x, dy, dw, db, ci, ci_real, co, ks):
        nbytes = KT.wgrad_plan(x.shape[0], x.shape[1], x.shape[2], ci, co, ks)[0]
        KT.wgrad(x, dy, flat.scratch(nbytes, dev), dw, db, ci, ci_real, 0, co, 0, ks)

    def g3_wgrad(x, dy, dw, ci, ci_real, co):
        nbytes = wgrad_plan(dy.shape[0], dy.shape[1], dy.shape[2], ci, co)[0]
        wgrad(x, dy, flat.scratch(nbytes, dev), dw, ci, ci_real, 0, co, 0, 2, 2)

    def conv1_bwd(name, gy, seq, x, ci, co, want_dx=True):
        dz = bn_bwd(name, gy, seq)
        kxk_wgrad(x, dz, G(seq[0].weight), None, ci, ci, co, 1)
        if not want_dx:
            return None
        return KT.dgrad(dz, KT.pack_dgrad(seq[0].weight, co), wide(x.shape[0], x.shape[1], x.shape[2], ci), None, co, 0, ci,
                        0, 0, 1, False)

    # softmax, then the folded output convolution D -> K and the product rule of W_out = Wf W_last
    last, fin = model.decoder.layer_lst[2], model.final_layer
    dl = _softmax_bwd(t['logits'], t['hm'], ghm.detach().contiguous().float(), t['temp'])
    dL = nhwc.nchw_to_nhwc(dl, K4, nhwc.F32)
    y6 = t['dec1'][1]
    dw_out, db_out = new(K, D, 3, 3), new(K)
    kxk_wgrad(y6, dL, dw_out, db_out, D, D, K, 3)
    wf = fin.weight.detach().reshape(K, D)
    G(fin.weight).copy_(torch.einsum('kcrs,mcrs->km', dw_out, last.weight.detach()).reshape(-1))
    G(last.weight).copy_(torch.einsum('km,kcrs->mcrs', wf, dw_out).reshape(-1))
    G(last.bias).copy_(wf.t() @ db_out)
    G(fin.bias).copy_(db_out)
    g = KT.dgrad(dL, KT.pack_dgrad(t['w_out'], K4), wide(BV, hb, wb, D), None, K4, 0, D, 0, 0, 3, False)
    # the transposed layers: weight gradient with the roles swapped, data gradient on the forward kernel at stride 2
    for name, seq, x, ci, co, hw in (('dec1', model.decoder.layer_lst[1], t['dec0'][1], D, D, (ha, wa)),
                                     ('dec0', model.decoder.layer_lst[0], t['expand'][1], C_, D, (h2, w2))):
        dz = bn_bwd(name, g, seq)
        g3_wgrad(dz, x, G(seq[0].weight), co, co, ci)
        g = FT.conv(dz, pack_dgrad_transpose(seq[0].weight, co), None, wide(BV, hw[0], hw[1], ci), co, 0, ci, 0, 2, 2, 1, False)
    g = conv1_bwd('expand', g, model.channel_expansion.layer_lst[0], t['scat'], C2, C_)
    coef_g, coef_s = t['coef']
    g = scatter_bwd_raw(g, coef_s, wide(B, h2, w2, C2), B, V, C2, 0, 0)
    g = conv1_bwd('fuse1', g, model.fuse_after_FTL.layer_lst[1], t['fuse0'][1], C2, C2)
    g = conv1_bwd('fuse0', g, model.fuse_after_FTL.layer_lst[0], t['cat'], V * C2, C2)
    g = gather_bwd_raw(g, coef_g, wide(BV, h2, w2, C2), B, V, C2, 0, C2, 0)
    # the strided layers: data gradient on the forward kernel over the zero-stuffed gradient; the features are frozen
    seq = model.encoder_head.layer_lst[1]
    dz = bn_bwd('enc1', g, seq)
    g3_wgrad(t['enc0'][1], dz, G(seq[0].weight), C_, C_, C2)
    g = FT.conv(dz, pack_dgrad(seq[0].weight, C2), None, wide(BV, h1, w1, C_), C2, 0, C_, 0, 1, 0, 2, False)
    seq = model.encoder_head.layer_lst[0]
    dz = bn_bwd('enc0', g, seq)
    g3_wgrad(t['x0'], dz, G(seq[0].weight), cin, C_, C_)
    model.tape = None


class HeadFn(torch.autograd.Function):
    """the heat maps of a training forward; the backward runs head_backward once and publishes the gradients"""

    @staticmethod
    def forward(ctx, model, anchor, hm):
        ctx.model = model
        return hm.view_as(hm)

    @staticmethod
    def backward(ctx, ghm):
        model = ctx.model
        if model.tape is None:
            raise RuntimeError('FTLMultiviewNet: backward called twice on one forward (the saved activations are released)')
        with torch.no_grad():
            head_backward(model, ghm)
            model.hip().publish()
        return None, None, None
