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

Not built (NOT_BUILT): training - there is no backward of the K x K convolution or the pools, no six-stage loss. The
model refuses training mode, and eval mode with a gradient required, with NotImplementedError.
"""
import torch
import torch.nn as nn

from hipnet import conv_kxk as K
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
    def __init__(self, k):
        super(CPM, self).__init__()
        self.k = int(k)
        for name, ci, co, ks in layer_table(self.k):
            setattr(self, name, nn.Conv2d(ci, co, kernel_size=ks, padding=ks // 2))
        self._plan, self._plan_key = None, None

    # ---- packed weights ------------------------------------------------------------------------------------------
    def cat_width(self):
        """row length of the concatenated map: 32 features, k + 1 heat maps, the centre map, padded to a multiple of 4"""
        return (FEAT + self.k + 2 + 3) // 4 * 4

    def _packed(self):
        tensors = list(self.parameters())
        key = tuple((t.data_ptr(), t._version) for t in tensors)
        if self._plan is not None and key == self._plan_key:
            return self._plan
        plan = {}
        for name, ci, co, ks in layer_table(self.k):
            conv = getattr(self, name)
            cip = self.cat_width() if name.startswith('Mconv1') else (ci + 3) // 4 * 4
            plan[name] = (K.pack(conv.weight, cip), conv.bias.detach().float().contiguous(), cip, co, ks)
        self._plan, self._plan_key = plan, key
        return plan

    def _conv(self, plan, name, x, relu, cin=None, x_off=0, out=None, y_off=0):
        w, b, cip, co, ks = plan[name]
        return K.conv_kxk(x, w, co, ks, bias=b, relu=relu, cin=cip if cin is None else cin, x_off=x_off, out=out,
                          y_off=y_off)

    # ---- the model -----------------------------------------------------------------------------------------------
    def _refuse(self, image, center_map):
        if self.training:
            raise NotImplementedError('CPM: {} (no backward of the K x K convolution and the pools, no six-stage loss): '
                                      'call .eval() and run under torch.no_grad()'.format(NOT_BUILT))
        if torch.is_grad_enabled() and (getattr(image, 'requires_grad', False) or
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
        self._refuse(image, center_map)
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
                y = self._conv(plan, 'Mconv1_stage{}'.format(s), cat, True)
                y = self._conv(plan, 'Mconv2_stage{}'.format(s), y, True)
                y = self._conv(plan, 'Mconv3_stage{}'.format(s), y, True)
                y = self._conv(plan, 'Mconv4_stage{}'.format(s), y, True)
                self._conv(plan, 'Mconv5_stage{}'.format(s), y, False, out=cat, y_off=FEAT)
                outs.append(self._heat(cat))
        return tuple(outs)

    def _heat(self, cat):
        """the k + 1 heat-map channels of the concatenated map as an NCHW tensor"""
        k1 = self.k + 1
        return nhwc.nhwc_to_nchw(cat, FEAT + k1)[:, FEAT:].contiguous()


def get_pose_net(cfg, is_train, **kwargs):
    return CPM(cfg.DATASET.NUM_JOINTS)
