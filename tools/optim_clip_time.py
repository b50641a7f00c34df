"""usage (GPU box): python tools/optim_clip_time.py
Kernel time of what gradient clipping adds to a step, at the generator's arena size, 1 and 8 pairs: the two norm launches
(splice_grad_norm_pairs) and the clipped update against the plain update, each as back-to-back launches between two events (the
launches queue up, so the interval is the kernels' own time plus dispatch gaps)."""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from splice_amd import _lib
from splice_amd.generator import GeneratorEngine

L = _lib.lib()
n1 = GeneratorEngine(device="cuda").numel
stride = (n1 + 63) // 64 * 64
out = []
for P in (1, 8):
    n = n1 if P == 1 else P * stride
    p, g, g2, m, v = (torch.randn(n, device="cuda") * 0.01 for _ in range(5))
    v.abs_()
    lrs = torch.full((P,), 2e-3, device="cuda")
    step = torch.ones(1, dtype=torch.int32, device="cuda")
    part = torch.zeros(P * ((n1 + 4095) // 4096), device="cuda")
    state = torch.zeros(P, 6, dtype=torch.int32, device="cuda")
    s = _lib.current_stream()
    def plain():
        if P == 1:
            return L.splice_optim_step_ex(0, _lib.ptr(p), _lib.ptr(g), _lib.ptr(g2), _lib.ptr(m), _lib.ptr(v), n, 2e-3, None, 0.0, 0.99, 1e-8, 5, 0, s)
        return L.splice_optim_step_pairs(0, _lib.ptr(p), _lib.ptr(g), _lib.ptr(g2), _lib.ptr(m), _lib.ptr(v), P, stride, n1, _lib.ptr(lrs), 0.0, 0.99, 1e-8, 5, 0, s)
    def norm():
        return L.splice_grad_norm_pairs(_lib.ptr(g), _lib.ptr(g2), P, stride, n1, 1e-3, _lib.ptr(part), _lib.ptr(state), None, None, s)
    def clipped():
        return L.splice_optim_step_pairs_clip(0, _lib.ptr(p), _lib.ptr(g), _lib.ptr(g2), _lib.ptr(m), _lib.ptr(v), None, P, stride, n1, _lib.ptr(lrs), 0.0, 0.99, 1e-8,
                                              _lib.ptr(step), None, 0, 0.0, 0, _lib.ptr(state), s)
    res = {}
    for rep in range(5):
        for name, fn in (("plain update", plain), ("norm (2 launches)", norm), ("clipped update", clipped)):
            for _ in range(20):
                assert fn() == 0
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(300):
                fn()
            b.record()
            torch.cuda.synchronize()
            res.setdefault(name, []).append(a.elapsed_time(b) / 300 * 1e3)
    for name in res:
        xs = sorted(res[name])
        out.append(f"P={P} n={n} floats {name}: median {xs[2]:.2f} us per call (min {xs[0]:.2f}, max {xs[-1]:.2f}; 5 x 300 back-to-back calls)")
print("\n".join(out))
