"""PredRNN on HRNet features (MODEL.NAME predrnn; reference lib/models/predrnn.py:7-234, HRNet_PredRNN_ResNet): the
reference's temporal 3-D model, inference on HIP kernels.

    model = get_pose_net(cfg, is_train=False).cuda().eval()
    with torch.no_grad():
        pose = model(frames)             # frames (B, L, 3, H, W) -> (B, 21, 3)

Three parts, children named as in the reference so that a checkpoint of it loads with strict=True:

    HRNet     models.pose_hrnet, frozen: each of the B L frames -> 21 heat maps + C0 = 32 inter_feat channels
    PredRNN   len(N_HIDDEN) SpatioTemporalLSTMCell layers (cell_list.{i}.conv_x.0 / .1 ... conv_o.0 / .1, conv_last) that walk
              the L frames with the zig-zag memory, and conv_last (1x1, no bias) that predicts a frame from the top hidden map
    resnet    block1, MaxPool2d(2, 2), block2, fc1, ReLU, fc2, ReLU on the LAST predicted frame -> 63 values

How it runs. Everything behind the backbone is f32 NHWC.
  Backbone: ONE call on (L B, 3, H, W) under no_grad, frames in time-major order; in eval mode this equals the reference's
    per-sample loop. Heat maps go to channels 0 .. 20 and inter_feat to 21 .. 52 of the frame map (L B, h, w, 56) on the
    device (the reference builds it on the CPU); the three pad channels are zero and layer 0's conv_x has zero weight
    columns for them.
  Cell (hipnet.predrnn.cell, csrc/predrnn.hip): conv_x / conv_h / conv_m on hipnet.conv_kxk, one statistics entry over the
    three raw outputs, the fused gates kernel (LayerNorm applied on load; c_new and m_new written into the two halves of the
    layer's memory map (B, h, w, 2 nh), so torch.cat((c_new, m_new)) is never a copy), conv_o and conv_last (1x1) on that
    map, one statistics entry, the fused output kernel. Layer 0's conv_x does not depend on the recurrence and runs for all
    L frames in one launch. A layer reads c_t from its own memory map and m_t from the map of the layer below (layer 0:
    from the top layer's, as it stood after the previous frame): the zig-zag of predrnn.py:108-114.
  Tail: BatchNorm (eval) is folded into the packed conv weights and a bias at load; the residual add + ReLU is
    hrnet_sum_terms; fc1 and fc2 run on hipnet.transformer.linear. fc1's weight (222 MB at full size) is read in place:
    the activation is brought to the reference's (C, H, W) flatten order instead. The final ReLU on the 63 outputs stays, as
    in the reference. Only the last frame is predicted in forward(); rnn_forward() predicts all of them.

rnn_forward(frame_map (B, L, 53, h, w)) -> (B, L, 53, h, w) and pose_forward(last_frame (B, 53, h, w)) -> (B, 63) are the
reference's RNN.forward and ResNet.forward; frame_map(frames) is what the backbone hands to the RNN.

Packed weights are built on first use and rebuilt when a parameter or buffer was written or moved.

Deviations from the reference
  - the reference's predrnn.get_pose_net is only pose_hrnet's, imported, and no reference tool builds the full model; here
    get_pose_net(cfg, is_train) returns HRNet_PredRNN_ResNet, so MODEL.NAME predrnn names this model.
  - the reference constructs its HRNet with is_train=True (weights initialised, MODEL.PRETRAINED loaded); so does this one.
  - MODEL.LAYER_NORM is accepted and ignored, as the reference ignores it (the cells always normalise).
  - refused before any device work (check_predrnn_config): STRIDE != 1, an even FILTER_SIZE or one above the convolution
    kernel's largest, N_HIDDEN entries that differ (the reference's zig-zag memory only type-checks when they are equal) or
    are no multiples of 4, a non-square or odd HEATMAP_SIZE, NUM_JOINTS != 21 (fc2 has 63 outputs).
  - training (back-propagation through L x layers cells) is not built: training mode, and eval mode with a gradient
    required, are a NotImplementedError. There is no CPU path.
"""
import ctypes

import torch
import torch.nn as nn

from hipnet import _capi as C
from hipnet import conv_kxk as K
from hipnet import nhwc
from hipnet import predrnn as P
from hipnet import transformer as T
from models import pose_hrnet

NOT_BUILT = 'training of PredRNN is not built'
JOINTS = 21


def check_predrnn_config(config):
    """what the model refuses of a config, before anything is built"""
    m = config.MODEL
    if m.STRIDE != 1:
        raise ValueError('MODEL.STRIDE {}: only stride 1 is built (the reference\'s LayerNorm([C, W, W]) is sized for it '
                         'too)'.format(m.STRIDE))
    ks = m.FILTER_SIZE
    if not isinstance(ks, int) or ks < 1 or not ks % 2 or ks > K.tile()[3]:
        raise ValueError('MODEL.FILTER_SIZE {}: expected an odd size <= {} (an even one changes the map size in the '
                         'reference as well)'.format(ks, K.tile()[3]))
    nhid = list(m.N_HIDDEN)
    if not nhid or any(not isinstance(n, int) or n < 4 or n % 4 for n in nhid) or len(set(nhid)) != 1:
        raise ValueError('MODEL.N_HIDDEN {}: expected equal entries (the zig-zag memory of the reference passes one map '
                         'through every layer) that are multiples of 4'.format(nhid))
    size = list(m.HEATMAP_SIZE)
    if len(size) != 2 or size[0] != size[1] or size[0] < 2 or size[0] % 2:
        raise ValueError('MODEL.HEATMAP_SIZE {}: expected a square, even size (LayerNorm([C, W, W]), MaxPool2d(2, 2) and '
                         'fc1\'s width)'.format(size))
    if m.NUM_JOINTS != JOINTS:
        raise ValueError('MODEL.NUM_JOINTS {}: the frame map holds 21 heat maps and fc2 has 63 outputs'.format(m.NUM_JOINTS))


def _conv_ln(cin, cout, ks, width):
    return nn.Sequential(nn.Conv2d(cin, cout, kernel_size=ks, stride=1, padding=ks // 2), nn.LayerNorm([cout, width, width]))


class SpatioTemporalLSTMCell(nn.Module):
    """the parameters of one cell (predrnn.py:8-30); hipnet.predrnn.cell runs it"""

    def __init__(self, in_channel, num_hidden, width, filter_size):
        super(SpatioTemporalLSTMCell, self).__init__()
        self.num_hidden = num_hidden
        self.conv_x = _conv_ln(in_channel, num_hidden * 7, filter_size, width)
        self.conv_h = _conv_ln(num_hidden, num_hidden * 4, filter_size, width)
        self.conv_m = _conv_ln(num_hidden, num_hidden * 3, filter_size, width)
        self.conv_o = _conv_ln(num_hidden * 2, num_hidden, filter_size, width)
        self.conv_last = nn.Conv2d(num_hidden * 2, num_hidden, kernel_size=1, stride=1, padding=0)


class RNN(nn.Module):
    def __init__(self, config):
        super(RNN, self).__init__()
        self.frame_channel = config.MODEL.EXTRA.STAGE2.NUM_CHANNELS[0] + JOINTS
        self.num_hidden = list(config.MODEL.N_HIDDEN)
        self.num_layers = len(self.num_hidden)
        width = config.MODEL.HEATMAP_SIZE[0]
        self.cell_list = nn.ModuleList([
            SpatioTemporalLSTMCell(self.frame_channel if i == 0 else self.num_hidden[i - 1], self.num_hidden[i], width,
                                   config.MODEL.FILTER_SIZE) for i in range(self.num_layers)])
        self.conv_last = nn.Conv2d(self.num_hidden[-1], self.frame_channel, kernel_size=1, stride=1, padding=0, bias=False)


class BasicBlock(nn.Module):
    def __init__(self, planes):
        super(BasicBlock, self).__init__()
        self.conv1 = nn.Conv2d(planes, planes, kernel_size=3, stride=1, padding=1, bias=False)
        self.bn1 = nn.BatchNorm2d(planes)
        self.conv2 = nn.Conv2d(planes, planes, kernel_size=3, stride=1, padding=1, bias=False)
        self.bn2 = nn.BatchNorm2d(planes)


class ResNet(nn.Module):
    def __init__(self, config, in_channel):
        super(ResNet, self).__init__()
        self.out_ch = in_channel
        self.block1 = BasicBlock(in_channel)
        self.block2 = BasicBlock(in_channel)
        self.fc1 = nn.Linear(in_channel * config.MODEL.HEATMAP_SIZE[0] * config.MODEL.HEATMAP_SIZE[0] // 4, 1024)
        self.fc2 = nn.Linear(1024, 3 * JOINTS)


def _relu_(t):
    """in-place ReLU of a (rows, C) f32 tensor, C a multiple of 4, on hrnet_sum_terms (one identity term, relu_out)"""
    rows, c = t.shape
    one = ctypes.c_void_p * 1
    with torch.cuda.device(t.device):
        C.call('hrnet_sum_terms', C.HR_F32, t.data_ptr(), rows, 1, 1, c, 1, one(t.data_ptr()), one(None), one(None),
               (ctypes.c_int * 1)(0), (ctypes.c_int * 1)(0), 1, C.stream_ptr())
    return t


def _add_relu(a, b):
    """relu(a + b) of two f32 NHWC maps on hrnet_sum_terms (the residual add that closes a BasicBlock)"""
    B, H, W, c = a.shape
    out = torch.empty_like(a)
    two = ctypes.c_void_p * 2
    with torch.cuda.device(a.device):
        C.call('hrnet_sum_terms', C.HR_F32, out.data_ptr(), B, H, W, c, 2, two(a.data_ptr(), b.data_ptr()), two(None, None),
               two(None, None), (ctypes.c_int * 2)(0, 0), (ctypes.c_int * 2)(0, 0), 1, C.stream_ptr())
    return out


class HRNet_PredRNN_ResNet(nn.Module):
    def __init__(self, config):
        super(HRNet_PredRNN_ResNet, self).__init__()
        check_predrnn_config(config)
        self.config = config
        self.RNN_in_channel = config.MODEL.EXTRA.STAGE2.NUM_CHANNELS[0] + JOINTS
        self.RNN_feat_size = config.MODEL.HEATMAP_SIZE[0]
        self.filter_size = config.MODEL.FILTER_SIZE
        self.HRNet = pose_hrnet.get_pose_net(config, is_train=True)
        if config.MODEL.HRNET_PRETRAINED:
            checkpoint = torch.load(config.MODEL.HRNET_PRETRAINED, map_location='cpu')
            print("=> loading a pretrained HRNet model '{}' (Epoch: {})".format(
                config.MODEL.HRNET_PRETRAINED, checkpoint['epoch']))
            self.HRNet.load_state_dict(checkpoint['state_dict'], strict=False)
        self.PredRNN = RNN(config)
        self.resnet = ResNet(config, self.RNN_in_channel)
        self._plan, self._plan_key = None, None

    # ---- packed weights ------------------------------------------------------------------------------------------
    def frame_width(self):
        """row length of the frame map: 21 heat maps + C0 features, padded to a multiple of 4"""
        return (self.RNN_in_channel + 3) // 4 * 4

    def _head_tensors(self):
        mods = (self.PredRNN, self.resnet)
        return [t for m in mods for t in list(m.parameters()) + list(m.buffers())]

    def _packed(self):
        tensors = self._head_tensors()
        key = tuple((t.data_ptr(), t._version) for t in tensors)
        if self._plan is not None and key == self._plan_key:
            return self._plan
        fw, ks = self.frame_width(), self.filter_size
        cells = []
        for i, cell in enumerate(self.PredRNN.cell_list):
            nh = cell.num_hidden
            p = {'nh': nh, 'ks': ks}
            for name in ('conv_x', 'conv_h', 'conv_m', 'conv_o'):
                conv = getattr(cell, name)[0]
                cin = fw if (i == 0 and name == 'conv_x') else conv.weight.shape[1]
                p[name] = (K.pack(conv.weight, cin), conv.bias.detach().float().contiguous(), cin)
            p['conv_last'] = (K.pack(cell.conv_last.weight, 2 * nh), cell.conv_last.bias.detach().float().contiguous(), 2 * nh)
            p['ln'] = tuple(P.pack_ln(t) for name in ('conv_x', 'conv_h', 'conv_m')
                            for t in (getattr(cell, name)[1].weight, getattr(cell, name)[1].bias))
            p['ln_o'] = (P.pack_ln(cell.conv_o[1].weight), P.pack_ln(cell.conv_o[1].bias))
            cells.append(p)
        plan = {'cells': cells, 'last': K.pack(self.PredRNN.conv_last.weight, self.PredRNN.num_hidden[-1])}
        for bname in ('block1', 'block2'):
            block = getattr(self.resnet, bname)
            for conv, bn, name in ((block.conv1, block.bn1, bname + '.1'), (block.conv2, block.bn2, bname + '.2')):
                # eval BatchNorm folded in float64: y = scale * conv(x) + (beta - mean * scale)
                scale = bn.weight.detach().double() / torch.sqrt(bn.running_var.detach().double() + bn.eps)
                shift = bn.bias.detach().double() - bn.running_mean.detach().double() * scale
                plan[name] = (nhwc.conv_pack(conv.weight, cin_pad=fw, scale=scale), shift.float().contiguous())
        # fc2 with a zero 64th row, so that its output row is a multiple of 4 wide for the ReLU launch
        w2, b2 = self.resnet.fc2.weight.detach(), self.resnet.fc2.bias.detach()
        rows = (w2.shape[0] + 3) // 4 * 4
        plan['fc2'] = (torch.zeros((rows, w2.shape[1]), dtype=torch.float32, device=w2.device), nhwc.padded(b2, rows))
        plan['fc2'][0][:w2.shape[0]] = w2
        self._plan, self._plan_key = plan, key
        return plan

    # ---- refusals ------------------------------------------------------------------------------------------------
    def _refuse(self, what, t, shape):
        if self.training:
            raise NotImplementedError('predrnn: {} (no backward through the L x layers cells): call .eval() and run under '
                                      'torch.no_grad()'.format(NOT_BUILT))
        if torch.is_grad_enabled() and (getattr(t, 'requires_grad', False) or any(p.requires_grad for p in self.parameters())):
            raise NotImplementedError('predrnn: eval mode with a gradient required is refused - {}: run under '
                                      'torch.no_grad()'.format(NOT_BUILT))
        if not isinstance(t, torch.Tensor) or t.ndim != len(shape) or t.numel() == 0 or any(
                s is not None and d != s for d, s in zip(t.shape, shape)):
            raise ValueError('predrnn: {} {}: expected ({})'.format(
                what, tuple(t.shape) if isinstance(t, torch.Tensor) else type(t).__name__,
                ', '.join('*' if s is None else str(s) for s in shape)))
        if not t.is_cuda:
            raise ValueError('predrnn: {} must be a HIP-device tensor (there is no CPU path in this build)'.format(what))
        if t.dtype != torch.float32:
            raise ValueError('predrnn: {} is {}: float32 only'.format(what, t.dtype))
        if next(self.PredRNN.parameters()).device != t.device:
            raise ValueError('predrnn: the model is on {}, {} on {}'.format(next(self.PredRNN.parameters()).device, what, t.device))

    # ---- the three parts -----------------------------------------------------------------------------------------
    def frame_map(self, frames):
        """frames (B, L, 3, H, W) -> the frame map (L, B, h, w, 56) f32 NHWC, time-major: channels 0 .. 20 the heat maps,
        21 .. 52 inter_feat, the rest zero"""
        self._refuse('frames', frames, (None, None, 3, None, None))
        with torch.no_grad():
            return self._frame_map(frames)

    def _frame_map(self, frames):
        B, L = frames.shape[:2]
        x = frames.detach().transpose(0, 1).reshape((L * B,) + tuple(frames.shape[2:])).contiguous()
        heat, feat = self.HRNet(x)
        s = self.RNN_feat_size
        if tuple(heat.shape[1:]) != (JOINTS, s, s) or tuple(feat.shape[1:]) != (self.RNN_in_channel - JOINTS, s, s):
            raise ValueError('predrnn: the backbone gave heat maps {} and features {} for frames {}: MODEL.HEATMAP_SIZE is '
                             '{} x {}'.format(tuple(heat.shape), tuple(feat.shape), tuple(frames.shape), s, s))
        fm = nhwc.nchw_to_nhwc(torch.cat((heat.float(), feat.float()), 1).contiguous(), self.frame_width(), nhwc.F32)
        return fm.view(L, B, s, s, self.frame_width())

    def _rnn(self, fm, all_frames):
        """fm (L, B, h, w, 56) -> the predicted frames (L, B, h, w, 56), or the last one (1, B, h, w, 56)"""
        plan = self._packed()
        cells = plan['cells']
        L, B, h, w, fw = fm.shape
        nl, nh, dev = len(cells), cells[0]['nh'], fm.device
        hid = [torch.zeros((B, h, w, nh), dtype=torch.float32, device=dev) for _ in range(nl)]
        mem = [torch.zeros((B, h, w, 2 * nh), dtype=torch.float32, device=dev) for _ in range(nl)]
        wx, bx, cin = cells[0]['conv_x']
        xc_all = K.conv_kxk(fm.view(L * B, h, w, fw), wx, 7 * nh, cells[0]['ks'], bias=bx, cin=cin).view(L, B, h, w, 7 * nh)
        out = torch.zeros((L if all_frames else 1, B, h, w, fw), dtype=torch.float32, device=dev)
        for t in range(L):
            for i in range(nl):
                hid[i] = P.cell(cells[i], hid[i - 1] if i else None, 0, hid[i], mem[i], mem[i - 1] if i else mem[nl - 1], nh,
                                xc=None if i else xc_all[t])
            if all_frames or t == L - 1:
                K.conv_kxk(hid[nl - 1], plan['last'], self.RNN_in_channel, 1, out=out[t if all_frames else 0], y_off=0)
        return out

    def _block(self, plan, name, x):
        fw, c = self.frame_width(), self.RNN_in_channel
        zeros = lambda: torch.zeros(x.shape, dtype=torch.float32, device=x.device)
        w, b = plan[name + '.1']
        y = K.conv_kxk(x, w, c, 3, bias=b, relu=True, cin=fw, out=zeros())
        w, b = plan[name + '.2']
        y = K.conv_kxk(y, w, c, 3, bias=b, relu=False, cin=fw, out=zeros())
        return _add_relu(y, x)

    def _tail(self, x):
        """x (B, h, w, 56) with zero pad channels -> (B, 63)"""
        plan = self._packed()
        y = self._block(plan, 'block1', x)
        y = P.maxpool2x2(y)
        y = self._block(plan, 'block2', y)
        flat = nhwc.nhwc_to_nchw(y, self.RNN_in_channel).reshape(y.shape[0], -1)         # the reference's (C, H, W) order
        z = _relu_(T.linear(flat, self.resnet.fc1.weight, self.resnet.fc1.bias))
        w2, b2 = plan['fc2']
        return _relu_(T.linear(z, w2, b2))[:, :3 * JOINTS].contiguous()

    def rnn_forward(self, frame_map):
        """the reference's RNN.forward: frame_map (B, L, 53, h, w) -> the predicted frames (B, L, 53, h, w)"""
        s, c = self.RNN_feat_size, self.RNN_in_channel
        self._refuse('frame_map', frame_map, (None, None, c, s, s))
        with torch.no_grad():
            B, L = frame_map.shape[:2]
            x = frame_map.detach().transpose(0, 1).reshape(L * B, c, s, s).contiguous()
            fm = nhwc.nchw_to_nhwc(x, self.frame_width(), nhwc.F32).view(L, B, s, s, self.frame_width())
            out = self._rnn(fm, True)
            y = nhwc.nhwc_to_nchw(out.view(L * B, s, s, self.frame_width()), c)
            return y.view(L, B, c, s, s).transpose(0, 1).contiguous()

    def pose_forward(self, last_frame):
        """the reference's ResNet.forward: last_frame (B, 53, h, w) -> (B, 63)"""
        s, c = self.RNN_feat_size, self.RNN_in_channel
        self._refuse('last_frame', last_frame, (None, c, s, s))
        with torch.no_grad():
            return self._tail(nhwc.nchw_to_nhwc(last_frame.detach().contiguous(), self.frame_width(), nhwc.F32))

    def forward(self, frames):
        self._refuse('frames', frames, (None, None, 3, None, None))
        with torch.no_grad():
            last = self._rnn(self._frame_map(frames), False)[0]
            return self._tail(last).view(-1, JOINTS, 3)


def get_pose_net(cfg, is_train, **kwargs):
    return HRNet_PredRNN_ResNet(cfg)
