"""The project's own restatement of V2V's eval-mode forward (reference lib/models/v2v.py) from torch.nn.functional
calls on the CPU, in float64 unless told otherwise: the five block types and the network, driven by a state dict with
the reference's keys. tests/test_v2v_cpu.py holds it to the reference's own float64 output (tests/golden/v2v.npz);
the device tests use it where a fixture would be too large. Also the recipe that fills a state dict from a seed, shared
by the fixture's generator and the tests (the fixture does not store 11.8 M weights)."""
import numpy as np
import torch
import torch.nn.functional as F

EPS = 1e-5                                   # nn.BatchNorm3d's default


def fill_state_dict(keys_and_shapes, seed):
    """every entry from numpy.random.default_rng(seed), drawn in sorted key order, as float64 numpy arrays:
      conv / deconv weight     normal(0, 1.4 / sqrt(fan_in)), fan_in = in-channels * kernel volume as the forward sees
                               it (a ConvTranspose3d(2, 2) output voxel sums in-channels products, one tap each)
      conv / deconv bias       normal(0, 0.1)
      BatchNorm weight (gamma) uniform(0.5, 1.0)       BatchNorm bias (beta) normal(0, 0.2); the last BatchNorm of a
                               residual branch normal(-0.35, 0.2): its output is added to a skip that is >= 0 (it
                               comes out of a ReLU), and with a centred beta the chain of identity-skip blocks at
                               the 1^3 .. 4^3 levels drifts until every output of their ReLUs is positive
      running_mean             normal(0, 0.2)          running_var           uniform(0.5, 1.5)
      num_batches_tracked      7
    He scaling with gammas near 1 blew the output up to 1e4 in a probe; these gains keep the activations of the 60-odd
    layers O(1) and the ReLUs about half on, which the generator asserts."""
    rng = np.random.default_rng(seed)
    shapes = dict(keys_and_shapes)
    out = {}
    for k in sorted(shapes):
        shp = tuple(int(s) for s in shapes[k])
        leaf = k.rsplit('.', 1)[1]
        if leaf == 'num_batches_tracked':
            out[k] = np.array(7, dtype=np.int64)
        elif leaf == 'running_mean':
            out[k] = rng.normal(0.0, 0.2, shp)
        elif leaf == 'running_var':
            out[k] = rng.uniform(0.5, 1.5, shp)
        elif len(shp) == 5:
            transposed = 'upsample' in k
            fan_in = shp[0] if transposed else shp[1] * shp[2] * shp[3] * shp[4]
            out[k] = rng.normal(0.0, 1.4 / np.sqrt(fan_in), shp)
        elif leaf == 'weight':
            out[k] = rng.uniform(0.5, 1.0, shp)
        elif shapes.get(k.rsplit('.', 1)[0] + '.running_mean') is not None:
            out[k] = rng.normal(-0.35 if k.endswith('res_branch.4.bias') else 0.0, 0.2, shp)
        else:
            out[k] = rng.normal(0.0, 0.1, shp)
    return out


class Net:
    """sd: state dict (numpy or torch values) with the reference's keys; dtype: the precision everything runs in.
    relu_on collects, per ReLU in execution order, the fraction of its outputs that are nonzero."""

    def __init__(self, sd, dtype=torch.float64, device='cpu'):
        self.sd = {k: torch.as_tensor(np.asarray(v) if not isinstance(v, torch.Tensor) else v).to(device)
                   for k, v in sd.items()}
        self.sd = {k: (v.to(dtype) if v.is_floating_point() else v) for k, v in self.sd.items()}
        self.relu_on = []

    def _relu(self, x):
        y = F.relu(x)
        self.relu_on.append(float((y != 0).double().mean()))
        return y

    def _bn(self, x, p):
        g = self.sd
        return F.batch_norm(x, g[p + '.running_mean'], g[p + '.running_var'], g[p + '.weight'], g[p + '.bias'], False,
                            0.0, EPS)

    def _conv(self, x, p):
        w = self.sd[p + '.weight']
        return F.conv3d(x, w, self.sd[p + '.bias'], 1, (w.shape[2] - 1) // 2)

    def basic(self, x, p):
        return self._relu(self._bn(self._conv(x, p + '.block.0'), p + '.block.1'))

    def res(self, x, p):
        r = self._relu(self._bn(self._conv(x, p + '.res_branch.0'), p + '.res_branch.1'))
        r = self._bn(self._conv(r, p + '.res_branch.3'), p + '.res_branch.4')
        s = x
        if p + '.skip_con.0.weight' in self.sd:
            s = self._bn(self._conv(x, p + '.skip_con.0'), p + '.skip_con.1')
        return self._relu(r + s)

    @staticmethod
    def pool(x):
        return F.max_pool3d(x, 2, 2)

    def upsample(self, x, p):
        y = F.conv_transpose3d(x, self.sd[p + '.block.0.weight'], self.sd[p + '.block.0.bias'], 2, 0)
        return self._relu(self._bn(y, p + '.block.1'))

    def encoder_decoder(self, x, p='encoder_decoder'):
        skips = []
        for k in range(1, 6):
            skips.append(self.res(x, '{}.skip_res{}'.format(p, k)))
            x = self.res(self.pool(x), '{}.encoder_res{}'.format(p, k))
        x = self.res(x, p + '.mid_res')
        for k in range(5, 0, -1):
            x = self.res(x, '{}.decoder_res{}'.format(p, k))
            x = self.upsample(x, '{}.decoder_upsample{}'.format(p, k)) + skips[k - 1]
        return x

    def __call__(self, x):
        self.relu_on = []
        x = torch.as_tensor(x).to(next(iter(self.sd.values())).device)
        x = x.to(self.sd['output_layer.weight'].dtype)
        x = self.basic(x, 'front_layers.0')
        for k in (1, 2, 3):
            x = self.res(x, 'front_layers.{}'.format(k))
        x = self.encoder_decoder(x)
        x = self.res(x, 'back_layers.0')
        x = self.basic(x, 'back_layers.1')
        x = self.basic(x, 'back_layers.2')
        return self._conv(x, 'output_layer')


def forward(sd, x, dtype=torch.float64, device='cpu'):
    """-> numpy output of the eval-mode network in `dtype`"""
    with torch.no_grad():
        return Net(sd, dtype, device)(x).cpu().numpy()
