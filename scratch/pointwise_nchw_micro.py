"""Timing of hrnet_pointwise_nchw / hrnet_pointwise_nchw_bwd (csrc/pointwise.hip) at the volumetric model's size,
(N, Cin, Cout, P) = (12, 480, 32, 4096), next to PyTorch-ROCm's F.conv2d and its autograd on the same device tensors:
the table of DESIGN.md, "The vol model". 20 warm-up and 100 timed launches each between device events; prints one JSON
line with the median, the 10th and the 90th percentile in microseconds and the GB/s of the algorithmic bytes.

    python scratch/pointwise_nchw_micro.py [N Cin Cout H W]

PyTorch's backward is timed alone: the graph of one forward is kept (retain_graph) and only backward() sits between
the events."""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(HERE), 'hrnet-hand-pose-estimation_amd', 'lib'))

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from hipnet import _capi as C  # noqa: E402


def main(N=12, Cin=480, Cout=32, H=64, W=64):
    P = H * W
    x = torch.randn(N, Cin, H, W, device='cuda')
    w = torch.randn(Cout, Cin, 1, 1, device='cuda') * 0.05
    b = torch.randn(Cout, device='cuda')
    dy = torch.randn(N, Cout, H, W, device='cuda')
    y, dx, dw, db = torch.empty_like(dy), torch.empty_like(x), torch.empty_like(w), torch.empty_like(b)
    parts = C.call('hrnet_pointwise_nchw_parts', N, P)
    floats = parts * (Cout * Cin + Cout)
    scratch = torch.empty(floats, device='cuda')
    s = C.stream_ptr()

    def fwd():
        C.call('hrnet_pointwise_nchw', C.HR_F32, x.data_ptr(), w.data_ptr(), b.data_ptr(), y.data_ptr(), N, Cin, Cout, P, s)

    def bwd(want_dx=True, want_dw=True):
        C.call('hrnet_pointwise_nchw_bwd', C.HR_F32, x.data_ptr(), w.data_ptr(), dy.data_ptr(),
               dx.data_ptr() if want_dx else None, dw.data_ptr() if want_dw else None, db.data_ptr() if want_dw else None,
               scratch.data_ptr() if want_dw else None, floats if want_dw else 0, N, Cin, Cout, P, s)
    xr, wr, br = x.clone().requires_grad_(True), w.clone().requires_grad_(True), b.clone().requires_grad_(True)
    yr = F.conv2d(xr, wr, br)

    def torch_fwd():
        with torch.no_grad():
            F.conv2d(x, w, b)

    def torch_bwd():
        xr.grad = wr.grad = br.grad = None
        yr.backward(dy, retain_graph=True)

    def timed(fn, warm=20, iters=100):
        for _ in range(warm):
            fn()
        torch.cuda.synchronize()
        ts = []
        for _ in range(iters):
            a, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            e.record()
            e.synchronize()
            ts.append(a.elapsed_time(e) * 1e3)
        ts.sort()
        return ts[iters // 2], ts[iters // 10], ts[-(iters // 10)]
    fbytes = 4 * N * P * (Cin + Cout)
    out = {'shape': [N, Cin, Cout, P], 'parts': parts}
    for name, fn, nbytes in (('forward', fwd, fbytes), ('backward', bwd, 2 * fbytes),
                             ('backward_dx', lambda: bwd(True, False), fbytes),
                             ('backward_dw_db', lambda: bwd(False, True), fbytes),
                             ('torch_forward', torch_fwd, fbytes), ('torch_backward', torch_bwd, 2 * fbytes)):
        m, lo, hi = timed(fn)
        out[name] = {'us_median': round(m, 1), 'us_p10': round(lo, 1), 'us_p90': round(hi, 1),
                     'GBps': round(nbytes / m / 1e3, 1)}
    print(json.dumps(out))


if __name__ == '__main__':
    main(*[int(v) for v in sys.argv[1:6]])
