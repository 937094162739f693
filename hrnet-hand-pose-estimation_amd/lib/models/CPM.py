"""Convolutional Pose Machine (MODEL.NAME CPM; reference lib/models/CPM.py:6-175), inference on the HIP K x K
convolution (hipnet.conv_kxk, csrc/conv_kxk.hip).

    model = get_pose_net(cfg, is_train=False).cuda().eval()
    with torch.no_grad():
        maps = model(image, center_map)      # six (B, k + 1, H / 8, W / 8) NCHW f32 maps, stage 1 .. stage 6

The parameters carry the reference's names (conv1_stage1.weight ... Mconv5_stage6.bias, 80 tensors, 31 770 052 values at
k = 21), so a reference checkpoint loads with strict=True. image (B, 3, H, W) and center_map (B, 1, H, W), H and W
multiples of 8.

How it runs. Everything is f32 NHWC. Stage 1 and the shared trunk (`_middle`) are conv + ReLU + MaxPool2d(3, 2, 1) three
times. Stages 2 .. 6 read ONE concatenated map `cat` (B, H/8, W/8, 56) and nobody ever copies into it:

    channels  0 .. 31   conv4_stage2 / conv1_stage{3..6} write their 32 feature channels (ReLU fused)
    channels 32 .. 53   the previous stage's last 1x1 (conv7_stage1 / Mconv5_stage{s-1}) writes its k + 1 heat maps
    channel  54         the centre map, pooled once by hrnet_avgpool2d_9s8
    channel  55         pad, zero (allocated so); Mconv1_stage{s}'s packed weights carry a zero input channel for it

which is the reference's torch.cat([x, heat, center], 1) order (CPM.py:91), so Mconv1's weight needs no permutation. The
kernel stores only the real output channels, so a 22-channel layer leaves the centre channel alone. Each stage's heat
maps are converted out to NCHW (hrnet_nhwc_to_nchw) before the next stage overwrites the 32 feature channels; the heat
channels of stage s are read by Mconv1_stage{s+1} before Mconv5_stage{s+1} overwrites them (one stream, in order).

Packed weights are built on first use and rebuilt when a parameter was written or moved (load_state_dict, .to()).

Without trainable=True nothing of training exists (NOT_BUILT): the model refuses training mode, and eval mode with a
gradient required, with NotImplementedError, as it always did.

Training: CPM(k, trainable=True) / get_pose_net(cfg, is_train, trainable=True). In .train() the forward runs the SAME
launches as inference (so the heat maps have the inference model's bits) but keeps what the backward needs: one
concatenated map per stage (stage s reads cats[s - 2]; its heat maps land in cats[s - 1]), every ReLU output and the
pools' inputs. The six maps leave through ONE torch.autograd.Function whose backward walks the 40 layers in reverse on
hipnet.conv_kxk_train: hrnet_conv2d_kxk_wgrad (weight and bias gradient, written straight into the flat gradient buffer
behind param.grad), hrnet_conv2d_kxk_dgrad (mask = the producing layer's saved ReLU output; accumulate where a map feeds
several consumers: `mid` feeds five layers, a stage's heat maps the next stage and the loss) and
hrnet_maxpool2d_3x3s2_bwd (with the ReLU mask of the convolution in front). The 1x1 layers go through the same entries.
Mconv1's data gradient is two launches: channels 0 .. 31 (features, masked) and 32 .. 53 (heat maps, accumulated onto the
loss gradient); the centre map and the image get none. The transposed packs follow the forward packs' key. In .eval()
under no_grad a trainable model runs the inference path unchanged. cpm_loss is the reference's training loss
(lib/core/function.py:29-32: HeatmapLoss on the LAST stage) with optional intermediate supervision (stage_weights).
The parameters and gradients live in flat buffers (hip(): what hipnet.optim.FlatAdam steps).
"""
import torch
import torch.nn as nn

from hipnet import conv_kxk as K
from hipnet import conv_kxk_train as T
from hipnet import nhwc

NOT_BUILT = 'training of CPM is not built'
FEAT = 32                     # feature channels of the concatenated map (conv4_stage2 / conv1_stage{s})


def layer_table(k):
    """(name, Cin, Cout, ks) of the 40 convolutions in the reference's order (CPM.py:11-66)"""
    t = [('conv1_stage1', 3, 128, 9), ('conv2_stage1', 128, 128, 9), ('conv3_stage1', 128, 128, 9),
         ('conv4_stage1', 128, 32, 5), ('conv5_stage1', 32, 512, 9), ('conv6_stage1', 512, 512, 1),
         ('conv7_stage1', 512, k + 1, 1),
         ('conv1_stage2', 3, 128, 9), ('conv2_stage2', 128, 128, 9), ('conv3_stage2', 128, 128, 9),
         ('conv4_stage2', 128, 32, 5)]
    for s in range(2, 7):
        if s > 2:
            t.append(('conv1_stage{}'.format(s), 128, 32, 5))
        t += [('Mconv1_stage{}'.format(s), FEAT + k + 2, 128, 11), ('Mconv2_stage{}'.format(s), 128, 128, 11),
              ('Mconv3_stage{}'.format(s), 128, 128, 11), ('Mconv4_stage{}'.format(s), 128, 128, 1),
              ('Mconv5_stage{}'.format(s), 128, k + 1, 1)]
    return t


class CPM(nn.Module):
    def __init__(self, k, trainable=False):
        super(CPM, self).__init__()
        self.k = int(k)
        self.trainable = bool(trainable)
        for name, ci, co, ks in layer_table(self.k):
            setattr(self, name, nn.Conv2d(ci, co, kernel_size=ks, padding=ks // 2))
        self._plan, self._plan_key = None, None
        self._tplan, self._tplan_key = None, None
        self._flat, self._dirty, self.tape = None, 0, None

    # ---- packed weights ------------------------------------------------------------------------------------------
    def cat_width(self):
        """row length of the concatenated map: 32 features, k + 1 heat maps, the centre map, padded to a multiple of 4"""
        return (FEAT + self.k + 2 + 3) // 4 * 4

    def _packed(self):
        tensors = list(self.parameters())
        key = self._key(tensors)
        if self._plan is not None and key == self._plan_key:
            return self._plan
        plan = {}
        for name, ci, co, ks in layer_table(self.k):
            conv = getattr(self, name)
            cip = self.cat_width() if name.startswith('Mconv1') else (ci + 3) // 4 * 4
            plan[name] = (K.pack(conv.weight, cip), conv.bias.detach().float().contiguous(), cip, co, ks)
        self._plan, self._plan_key = plan, key
        return plan

    def _key(self, tensors=None):
        """what the packed weights were built from: a write through the flat buffer (FlatAdam) counts as one too"""
        tensors = list(self.parameters()) if tensors is None else tensors
        return tuple((t.data_ptr(), t._version) for t in tensors) + (self._dirty,)

    def _packed_t(self):
        """the flipped, transposed packs of hrnet_conv2d_kxk_dgrad, on the forward packs' key. The image layers have no
        data gradient; Mconv1 has two: its feature channels and its heat-map channels"""
        key = self._key()
        if self._tplan is not None and key == self._tplan_key:
            return self._tplan
        k1, plan = self.k + 1, {}
        for name, ci, co, ks in layer_table(self.k):
            w = getattr(self, name).weight
            cop = (co + 3) // 4 * 4
            if ci == 3:
                continue
            if name.startswith('Mconv1'):
                plan[name] = (T.pack_dgrad(w, cop, 0, FEAT), T.pack_dgrad(w, cop, FEAT, FEAT + k1))
            else:
                plan[name] = T.pack_dgrad(w, cop)
        self._tplan, self._tplan_key = plan, key
        return plan

    def _conv(self, plan, name, x, relu, cin=None, x_off=0, out=None, y_off=0):
        w, b, cip, co, ks = plan[name]
        return K.conv_kxk(x, w, co, ks, bias=b, relu=relu, cin=cip if cin is None else cin, x_off=x_off, out=out,
                          y_off=y_off)

    # ---- the model -----------------------------------------------------------------------------------------------
    def _refuse(self, image, center_map, tape=False):
        if self.training and not tape:
            raise NotImplementedError('CPM: {} (no backward of the K x K convolution and the pools, no six-stage loss): '
                                      'call .eval() and run under torch.no_grad()'.format(NOT_BUILT))
        if not tape and torch.is_grad_enabled() and (getattr(image, 'requires_grad', False) or
                                        getattr(center_map, 'requires_grad', False) or
                                        any(p.requires_grad for p in self.parameters())):
            raise NotImplementedError('CPM: eval mode with a gradient required is refused - {}: run under '
                                      'torch.no_grad()'.format(NOT_BUILT))
        for key, t, c in (('image', image, 3), ('center_map', center_map, 1)):
            if not isinstance(t, torch.Tensor) or t.ndim != 4 or t.shape[1] != c or t.numel() == 0:
                raise ValueError('CPM: {} {}: expected (B, {}, H, W)'.format(
                    key, tuple(t.shape) if isinstance(t, torch.Tensor) else type(t).__name__, c))
        B, _, H, W = image.shape
        if H % 8 or W % 8:
            raise ValueError('CPM: image {} x {}: H and W must be multiples of 8 (the reference\'s own concatenation of the '
                             'stride-8 maps fails otherwise)'.format(H, W))
        if tuple(center_map.shape) != (B, 1, H, W):
            raise ValueError('CPM: center_map {} for an image {}: expected ({}, 1, {}, {})'.format(
                tuple(center_map.shape), tuple(image.shape), B, H, W))
        if not image.is_cuda or not center_map.is_cuda or image.device != center_map.device:
            raise ValueError('CPM: expected HIP-device tensors on one device (there is no CPU path in this build)')
        if image.dtype != torch.float32 or center_map.dtype != torch.float32:
            raise ValueError('CPM: image {} / center_map {}: float32 only'.format(image.dtype, center_map.dtype))

    def _trunk(self, plan, x, names):
        """three times conv 9x9 + ReLU + MaxPool2d(3, 2, 1)"""
        for name in names:
            x = K.maxpool3x3s2(self._conv(plan, name, x, True))
        return x

    def forward(self, image, center_map):
        if self.trainable and self.training:
            self._refuse(image, center_map, tape=True)
            return self._forward_train(image, center_map)
        self._refuse(image, center_map)
        return tuple(self._infer(image, center_map)[0])

    def _infer(self, image, center_map, keep=None, last_heat=True):
        """the inference launches -> (the NCHW heat maps of stages 1 .. 6 (1 .. 5 without last_heat), the concatenated
        map as stage 6 leaves it: its features, ITS heat maps, the centre map). keep: a dict that receives stage 6's four
        ReLU outputs as m1 .. m4 (models.CPM_volumetric trains its last layers from them)"""
        with torch.no_grad():
            plan = self._packed()
            k1 = self.k + 1
            B, _, H, W = image.shape
            x = nhwc.nchw_to_nhwc(image.detach().contiguous(), 4, nhwc.F32)
            cat = torch.zeros((B, H // 8, W // 8, self.cat_width()), dtype=torch.float32, device=image.device)
            K.avgpool9s8(center_map.detach(), out=cat, y_off=FEAT + k1)
            # stage 1
            y = self._trunk(plan, x, ('conv1_stage1', 'conv2_stage1', 'conv3_stage1'))
            y = self._conv(plan, 'conv4_stage1', y, True)
            y = self._conv(plan, 'conv5_stage1', y, True)
            y = self._conv(plan, 'conv6_stage1', y, True)
            self._conv(plan, 'conv7_stage1', y, False, out=cat, y_off=FEAT)
            outs = [self._heat(cat)]
            # the trunk shared by stages 2 .. 6
            mid = self._trunk(plan, x, ('conv1_stage2', 'conv2_stage2', 'conv3_stage2'))
            for s in range(2, 7):
                self._conv(plan, 'conv4_stage2' if s == 2 else 'conv1_stage{}'.format(s), mid, True, out=cat, y_off=0)
                y = cat
                for i in (1, 2, 3, 4):
                    y = self._conv(plan, 'Mconv{}_stage{}'.format(i, s), y, True)
                    if keep is not None and s == 6:
                        keep['m{}'.format(i)] = y
                self._conv(plan, 'Mconv5_stage{}'.format(s), y, False, out=cat, y_off=FEAT)
                if s < 6 or last_heat:
                    outs.append(self._heat(cat))
        return outs, cat

    def _heat(self, cat):
        """the k + 1 heat-map channels of the concatenated map as an NCHW tensor"""
        k1 = self.k + 1
        return nhwc.nhwc_to_nchw(cat, FEAT + k1)[:, FEAT:].contiguous()


    # ---- training ------------------------------------------------------------------------------------------------
    def hip(self):
        """the flat f32 parameter and gradient buffers (what hipnet.optim.FlatAdam steps): built on first use on the
        parameters' device; every parameter becomes a view of flat_p and its .grad a view of flat_g"""
        if not self.trainable:
            raise NotImplementedError('CPM: {}: build the model with trainable=True'.format(NOT_BUILT))
        prm = list(self.parameters())
        if self._flat is None or self._flat.flat_p.device != prm[0].device:
            self._flat = _Flat(self)
        return self._flat

    def _forward_train(self, image, center_map):
        flat = self.hip()
        with torch.no_grad():
            plan = self._packed()
            k1 = self.k + 1
            B, _, H, W = image.shape
            tape = {'x': nhwc.nchw_to_nhwc(image.detach().contiguous(), 4, nhwc.F32)}
            cats = [torch.zeros((B, H // 8, W // 8, self.cat_width()), dtype=torch.float32, device=image.device)
                    for _ in range(6)]
            for cat in cats[:5]:
                K.avgpool9s8(center_map.detach(), out=cat, y_off=FEAT + k1)
            tape['cats'] = cats

            def trunk(stage):
                p = tape['x']
                for i in (1, 2, 3):
                    a = self._conv(plan, 'conv{}_stage{}'.format(i, stage), p, True)
                    tape['a{}_{}'.format(i, stage)] = a
                    p = K.maxpool3x3s2(a)
                    tape['p{}_{}'.format(i, stage)] = p
                return p

            y = trunk(1)
            for i in (4, 5, 6):
                y = tape['y{}'.format(i)] = self._conv(plan, 'conv{}_stage1'.format(i), y, True)
            self._conv(plan, 'conv7_stage1', y, False, out=cats[0], y_off=FEAT)
            outs = [self._heat(cats[0])]
            mid = trunk(2)
            for s in range(2, 7):
                cat = cats[s - 2]
                self._conv(plan, 'conv4_stage2' if s == 2 else 'conv1_stage{}'.format(s), mid, True, out=cat, y_off=0)
                y = cat
                for i in (1, 2, 3, 4):
                    y = tape['m{}_{}'.format(i, s)] = self._conv(plan, 'Mconv{}_stage{}'.format(i, s), y, True)
                self._conv(plan, 'Mconv5_stage{}'.format(s), y, False, out=cats[s - 1], y_off=FEAT)
                outs.append(self._heat(cats[s - 1]))
        self.tape = tape
        return _CPMFn.apply(self, flat.anchor, *outs)

    def _backward(self, gouts):
        """the 40 layers in reverse; gouts: six (B, k + 1, h, w) gradients or None. Gradients land in flat_g"""
        flat, tape, tp, k1 = self.hip(), self.tape, self._packed_t(), self.k + 1
        cats = tape['cats']
        B, h, w, _ = cats[0].shape
        dev = cats[0].device
        hp = (k1 + 3) // 4 * 4
        scratch = flat.scratch
        # the heat-map gradients: (B, h, w, hp) with zero pad channels; a stage nobody supervises starts from zeros
        G = [torch.zeros((B, h, w, hp), dtype=torch.float32, device=dev) if g is None else
             nhwc.nchw_to_nhwc(g.detach().contiguous().float(), hp, nhwc.F32) for g in gouts]

        def wgrad(name, x, dy, cin=None, real=None, cout=None):
            conv = getattr(self, name)
            co, ci, ks, _ = conv.weight.shape
            cin = x.shape[3] if cin is None else cin
            nbytes = T.wgrad_plan(x.shape[0], x.shape[1], x.shape[2], cin, co, ks)[0]
            T.wgrad(x, dy, scratch(nbytes, dev), flat.grad_of(conv.weight), flat.grad_of(conv.bias), cin, ci, 0, co, 0, ks)

        def dgrad(name, dy, cin, mask, out=None, accumulate=False, pack=None):
            ks = getattr(self, name).weight.shape[2]
            if out is None:
                out = torch.empty(dy.shape[:3] + (cin,), dtype=torch.float32, device=dev)
            return T.dgrad(dy, tp[name] if pack is None else pack, out, mask, dy.shape[3], 0, cin, 0, 0, ks, accumulate)

        dmid = None
        for s in range(6, 1, -1):
            cat = cats[s - 2]
            m = [None] + [tape['m{}_{}'.format(i, s)] for i in (1, 2, 3, 4)]
            wgrad('Mconv5_stage{}'.format(s), m[4], G[s - 1])
            d = dgrad('Mconv5_stage{}'.format(s), G[s - 1], 128, m[4])
            for i in (4, 3, 2):
                wgrad('Mconv{}_stage{}'.format(i, s), m[i - 1], d)
                d = dgrad('Mconv{}_stage{}'.format(i, s), d, 128, m[i - 1])
            name = 'Mconv1_stage{}'.format(s)
            wgrad(name, cat, d, cin=self.cat_width())
            df = dgrad(name, d, FEAT, cat, pack=tp[name][0])
            dgrad(name, d, k1, None, out=G[s - 2], accumulate=True, pack=tp[name][1])
            name = 'conv4_stage2' if s == 2 else 'conv1_stage{}'.format(s)
            wgrad(name, tape['p3_2'], df)
            dmid = dgrad(name, df, 128, None, out=dmid, accumulate=dmid is not None)
        wgrad('conv7_stage1', tape['y6'], G[0])
        d = dgrad('conv7_stage1', G[0], 512, tape['y6'])
        wgrad('conv6_stage1', tape['y5'], d)
        d = dgrad('conv6_stage1', d, 512, tape['y5'])
        wgrad('conv5_stage1', tape['y4'], d)
        d = dgrad('conv5_stage1', d, FEAT, tape['y4'])
        wgrad('conv4_stage1', tape['p3_1'], d)
        dp = {1: dgrad('conv4_stage1', d, 128, None), 2: dmid}
        for stage in (1, 2):
            d = dp[stage]
            for i in (3, 2, 1):
                a = tape['a{}_{}'.format(i, stage)]
                da = torch.empty_like(a)
                T.maxpool_bwd(a, d, da, a.shape[3], 0, 0, 0, True)
                name = 'conv{}_stage{}'.format(i, stage)
                if i == 1:
                    wgrad(name, tape['x'], da)
                else:
                    wgrad(name, tape['p{}_{}'.format(i - 1, stage)], da)
                    d = dgrad(name, da, 128, None)
        self.tape = None


class _Flat(object):
    """flat f32 parameters and gradients of a trainable CPM in parameter order: the interface hipnet.optim.FlatAdam uses"""

    def __init__(self, model):
        self.model = model
        self.params = list(model.parameters())
        self.names = [n for n, _ in model.named_parameters()]
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
        # what ties the six maps to autograd's graph: its "gradient" is never used, the real ones go to flat_g
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


class _CPMFn(torch.autograd.Function):
    """the six heat maps of a training forward; the backward runs CPM._backward once for all of them"""

    @staticmethod
    def forward(ctx, model, anchor, *outs):
        ctx.model = model
        ctx.set_materialize_grads(False)          # a stage nobody supervises hands None, not a map of zeros
        return tuple(o.view_as(o) for o in outs)

    @staticmethod
    def backward(ctx, *gouts):
        model = ctx.model
        if model.tape is None:
            raise RuntimeError('CPM: backward called twice on one forward (the saved activations are released)')
        with torch.no_grad():
            model._backward(gouts)
            model.hip().publish()
        return (None, None) + (None,) * len(gouts)


def cpm_loss(maps, target, stage_weights=(0, 0, 0, 0, 0, 1), criterion=None):
    """the reference's CPM training loss (lib/core/function.py:29-32): HeatmapLoss of the LAST stage's maps against the
    target; stage_weights (six floats) adds the other stages with their weights (intermediate supervision)"""
    from core.loss import HeatmapLoss
    if len(maps) != 6 or len(stage_weights) != 6:
        raise ValueError('cpm_loss: {} maps, {} stage weights: expected six of each'.format(len(maps), len(stage_weights)))
    criterion = HeatmapLoss('l2') if criterion is None else criterion
    loss = None
    for m, wgt in zip(maps, stage_weights):
        if float(wgt) == 0.0:
            continue
        term = criterion(m, target) if float(wgt) == 1.0 else criterion(m, target) * float(wgt)
        loss = term if loss is None else loss + term
    if loss is None:
        raise ValueError('cpm_loss: every stage weight is zero')
    return loss


def get_pose_net(cfg, is_train, trainable=False, **kwargs):
    return CPM(cfg.DATASET.NUM_JOINTS, trainable=trainable)
