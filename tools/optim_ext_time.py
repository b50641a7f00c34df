"""usage (GPU box): python tools/optim_ext_time.py            (event timing)
       rocprofv3 --kernel-trace --stats -d DIR -o optim_ext --output-format csv -- python tools/optim_ext_time.py   (the kernels' own time)
Kernel time of the fused update under the extended rules against the plain rule of the same kind, at the
generator's arena size, 1 and 8 pairs: sgd + momentum, rmsprop + momentum + centered, adamw + amsgrad.  Each as back-to-back launches
between two events (the launches queue up, so the interval is the kernels' own time plus dispatch gaps); under rocprofv3 the stats
table names every instance (the rule and PAIR_LR are template arguments)."""
import ctypes as C
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from splice_amd import _lib
from splice_amd.generator import GeneratorEngine

L = _lib.lib()
n1 = GeneratorEngine(device="cuda").numel
stride = (n1 + 63) // 64 * 64
HP = {0: (0.9, 0.99, 1e-8), 1: (0.99, 0.0, 1e-8), 2: (0.0, 0.0, 0.0)}
RULES = [("adam", 0, None), ("adamw + amsgrad", 0, dict(weight_decay=0.01, decoupled=True, amsgrad=True)),
         ("rmsprop", 1, None), ("rmsprop + momentum + centered", 1, dict(momentum=0.9, centered=True)),
         ("sgd", 2, None), ("sgd + momentum", 2, dict(momentum=0.9))]
out = []
for P in (1, 8):
    n = n1 if P == 1 else P * stride
    p, g, g2, m, v, w = (torch.randn(n, device="cuda") * 0.01 for _ in range(6))
    v.abs_().add_(1e-3)
    w.mul_(0.1)          # (v > w^2: the centred rule stays real)
    lrs = torch.full((P,), 2e-3, device="cuda")
    s = _lib.current_stream()
    res = {}
    for rep in range(5):
        for name, kind, ext in RULES:
            rec = None if ext is None else _lib.optim_ext(ext)

            def fn():
                if rec is not None:
                    return L.splice_optim_step_pairs_ext(kind, _lib.ptr(p), _lib.ptr(g), _lib.ptr(g2), _lib.ptr(m), _lib.ptr(v), _lib.ptr(w), None, P, stride, n1,
                                                         _lib.ptr(lrs), *HP[kind], 5, None, None, 0, 0.0, 0, None, None, None, None, C.byref(rec), s)
                if P == 1:
                    return L.splice_optim_step_ex(kind, _lib.ptr(p), _lib.ptr(g), _lib.ptr(g2), _lib.ptr(m), _lib.ptr(v), n, 2e-3, None, *HP[kind], 5, 0, s)
                return L.splice_optim_step_pairs(kind, _lib.ptr(p), _lib.ptr(g), _lib.ptr(g2), _lib.ptr(m), _lib.ptr(v), P, stride, n1, _lib.ptr(lrs), *HP[kind], 5, 0, s)
            for _ in range(20):
                assert fn() == 0, L.splice_last_error()
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
