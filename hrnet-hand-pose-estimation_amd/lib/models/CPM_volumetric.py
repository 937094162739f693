"""CPM_volumetric - the backbone of the volumetric triangulation model on the CPM family (MODEL.NAME vol_CPM; reference
lib/models/CPM_volumetric.py:44-227), on the HIP K x K convolution of models.CPM and the slice up-sampling of
hipnet.upsample_slice.

It IS a models.CPM.CPM (same 80 parameters under the reference's names, same launches) with three differences:

  * forward(image, center_map) returns the reference's 8-tuple (:222): the five stride-8 heat maps of stages 1 .. 5
    (B, k + 1, H / 8, W / 8), stage 6's heat maps at MODEL.HEATMAP_SIZE, inter_feat, None. Stage 6's maps are lifted
    straight out of the concatenated map (channels 32 .. 32 + k of 56) by ONE hrnet_upsample_slice_nchw launch: no
    NHWC -> NCHW copy at stride 8 comes first.
  * inter_feat is the f32 NHWC ReLU output of Mconv4_stage6, (B, H / 8, W / 8, 128), read through `inter_feat(outputs)`.
    The reference up-samples it to 128 NCHW channels (:217); models.triangulation runs process_features first, at
    stride 8, and up-samples 32 channels, so that tensor is never made (models/triangulation.py says why that is the
    same function).
  * with MODEL.VOL_CONFIDENCES the parameters and buffers of GlobalAveragePoolingHead(128, 32) (:7-41, :107-108) exist
    under `vol_confidences.*` after Mconv5_stage6, so a reference checkpoint loads with strict=True. No launch reads
    the head and the eighth slot is None: the reference uses it only under the conf* aggregations, which
    models.triangulation refuses (the decision of models/pose_hrnet_volumetric.py).

MODEL.HEATMAP_SIZE is (width, height) as everywhere in this project; the reference reads its first entry for both axes
(:47, :220), which is the same for its square yamls.

Training (trainable=True, .train()): only Mconv3/4/5_stage6 train (reference lib/models/triangulation.py:512-527), so the
40-layer backward of models.CPM is not used. The forward runs the inference launches (the outputs have the inference
forward's bits) and keeps the ReLU outputs of Mconv2/3/4_stage6 and stage 6's concatenated map; the backward is

    G  = up-sample transpose of the heat-map gradient          hrnet_upsample_slice_nchw_bwd into (B, h, w, 24), pad zero
    Mconv5_stage6: weight and bias gradient from (m4, G); d = mask_m4(W5^T G) + g_feat       dgrad, mask, accumulate
    Mconv4_stage6: weight and bias gradient from (m3, d); d3 = mask_m3(W4^T d)
    Mconv3_stage6: weight and bias gradient from (m2, d3); stop.

hrnet_conv2d_kxk_dgrad with mask and accumulate computes mask(acc) + what-was-there: the mask covers the convolution's
term only. The mask is a 0/1 factor, so mask(a + b) = mask(a) + mask(b) exactly, and g_feat arrives ALREADY masked: its
producer is process_features' data gradient, conv_kxk_dgrad with mask = inter_feat itself (the ReLU output it read).
That is the contract of `inter_feat`: whoever differentiates through it returns the gradient with respect to the ReLU's
INPUT, as every dgrad of models.CPM does. Everything below Mconv3_stage6 has requires_grad False, gets no launch and
keeps its bits. The gradients are returned to autograd (one torch.autograd.Function over the six trainable tensors), so
.grad accumulates as usual and torch.optim.Adam steps them; there is no flat buffer (hip() refuses).
"""
import torch
import torch.nn as nn

from hipnet import conv_kxk_train as T
from hipnet import upsample_slice as S
from models import CPM as _cpm
from models.pose_hrnet_volumetric import GlobalAveragePoolingHead

FEAT = _cpm.FEAT
INTER = 128                   # channels of inter_feat (Mconv4_stage6)
TRAINED = ('Mconv3_stage6', 'Mconv4_stage6', 'Mconv5_stage6')


class CPM(_cpm.CPM):
    def __init__(self, cfg, trainable=False):
        if cfg.MODEL.get('ALG_CONFIDENCES', False):
            raise NotImplementedError('CPM_volumetric: MODEL.ALG_CONFIDENCES is not built')
        hm = cfg.MODEL.HEATMAP_SIZE
        if len(hm) != 2 or min(int(v) for v in hm) < 1:
            raise ValueError('CPM_volumetric: MODEL.HEATMAP_SIZE {}: expected (width, height)'.format(list(hm)))
        super(CPM, self).__init__(cfg.DATASET.NUM_JOINTS, trainable=trainable)
        self.hm_size = (int(hm[1]), int(hm[0]))                 # (H, W) of the lifted maps
        if cfg.MODEL.get('VOL_CONFIDENCES', False):
            self.vol_confidences = GlobalAveragePoolingHead(INTER, 32)
        self._tpacks = {}

    # ---- packed weights: per layer, so an optimiser step repacks three layers and not forty ------------------------
    def _packed(self):
        plan = self._plan if self._plan is not None else {}
        keys = self._plan_key if isinstance(self._plan_key, dict) else {}
        for name, ci, co, ks in _cpm.layer_table(self.k):
            conv = getattr(self, name)
            key = self._layer_key(conv)
            if keys.get(name) != key:
                cip = self.cat_width() if name.startswith('Mconv1') else (ci + 3) // 4 * 4
                plan[name] = (_cpm.K.pack(conv.weight, cip), conv.bias.detach().float().contiguous(), cip, co, ks)
                keys[name] = key
        self._plan, self._plan_key = plan, keys
        return plan

    @staticmethod
    def _layer_key(conv):
        return (conv.weight.data_ptr(), conv.weight._version, conv.bias.data_ptr(), conv.bias._version)

    def _packed_t(self, name):
        """the flipped, transposed pack of hrnet_conv2d_kxk_dgrad for one of the trained layers"""
        conv = getattr(self, name)
        key = self._layer_key(conv)
        if self._tpacks.get(name, (None,))[0] != key:
            self._tpacks[name] = (key, T.pack_dgrad(conv.weight, (conv.out_channels + 3) // 4 * 4))
        return self._tpacks[name][1]

    def hip(self):
        raise NotImplementedError('CPM_volumetric: there is no flat parameter buffer - the three trained layers get their '
                                  'gradients through autograd (.grad) and torch.optim.Adam steps them')

    # ---- the model ---------------------------------------------------------------------------------------------------
    @staticmethod
    def inter_feat(outputs):
        """the seventh output: Mconv4_stage6's ReLU output, f32 NHWC (B, H / 8, W / 8, 128). A gradient sent back through it
        must be the one with respect to the ReLU's INPUT (masked where the tensor is <= 0): conv_kxk_dgrad(..., mask=this
        tensor) returns exactly that"""
        return outputs[6]

    def forward(self, image, center_map):
        tape = self.trainable and self.training
        self._refuse(image, center_map, tape=tape)
        if tape and torch.is_grad_enabled():
            trained = [p for name in TRAINED for p in (getattr(self, name).weight, getattr(self, name).bias)]
            if any(p.requires_grad for p in trained):
                return _ShortFn.apply(self, image, center_map, *trained) + (None,)
        return self._run(image, center_map, {}) + (None,)

    def _run(self, image, center_map, keep):
        """the seven tensors of the 8-tuple; keep receives stage 6's ReLU outputs m1 .. m4"""
        outs, cat = self._infer(image, center_map, keep=keep, last_heat=False)
        return tuple(outs) + (S.upsample_slice(cat, FEAT, self.k + 1, self.hm_size), keep['m4'])

    def _backward(self, keep, g_heat, g_feat):
        """the short walk of the module docstring -> the gradients of (w3, b3, w4, b4, w5, b5), None where nothing arrives"""
        m2, m3, m4 = keep['m2'], keep['m3'], keep['m4']
        B, h, w, _ = m4.shape
        k1 = self.k + 1
        hp = (k1 + 3) // 4 * 4
        dw5 = db5 = None
        d = None if g_feat is None else g_feat.detach().contiguous().float().clone()
        if g_heat is not None:
            G = S.upsample_slice_bwd(g_heat.detach().contiguous().float(), (h, w), hp, 0, k1)
            dw5, db5 = T.conv_kxk_wgrad(m4, G, k1, 1)
            d = T.conv_kxk_dgrad(G, self._packed_t('Mconv5_stage6'), INTER, 1, out=d, mask=m4, accumulate=d is not None)
        if d is None:
            return (None,) * 6
        dw4, db4 = T.conv_kxk_wgrad(m3, d, INTER, 1)
        d3 = T.conv_kxk_dgrad(d, self._packed_t('Mconv4_stage6'), INTER, 1, mask=m3)
        dw3, db3 = T.conv_kxk_wgrad(m2, d3, INTER, 11)
        return dw3, db3, dw4, db4, dw5, db5


class _ShortFn(torch.autograd.Function):
    """the training forward of CPM_volumetric: the inference launches, and a backward that reaches the last three layers"""

    @staticmethod
    def forward(ctx, model, image, center_map, *trained):
        keep = {}
        outs = model._run(image, center_map, keep)
        ctx.model, ctx.keep = model, keep
        model.tape = keep                   # the saved activations of the latest training forward, until its backward
        ctx.set_materialize_grads(False)
        ctx.mark_non_differentiable(*outs[:5])
        return outs

    @staticmethod
    def backward(ctx, *g):
        if ctx.keep is None:
            raise RuntimeError('CPM_volumetric: backward called twice on one forward (the saved activations are released)')
        with torch.no_grad():
            grads = ctx.model._backward(ctx.keep, g[5], g[6])
        if ctx.model.tape is ctx.keep:
            ctx.model.tape = None
        ctx.keep = None
        need = ctx.needs_input_grad[3:]
        return (None, None, None) + tuple(gr if nd else None for gr, nd in zip(grads, need))


def get_pose_net(cfg, is_train, trainable=False, **kwargs):
    return CPM(cfg, trainable=trainable)
