"""usage (GPU box): python tools/optim_best_time.py
Kernel time of the optimiser launch without and with the keep-best snapshot, at the generator's arena size, 1 and 8 pairs: the masked
update (the stop rule on, the option off) against the snapshot instance on a step that does not take (one record load per slot) and on a
step that takes (one store stream more), each as back-to-back launches between two events (the launches queue up, so the interval is the
kernels' own time plus dispatch gaps)."""
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
    p, g, g2, m, v, bp = (torch.randn(n, device="cuda") * 0.01 for _ in range(6))
    v.abs_()
    lrs = torch.full((P,), 2e-3, device="cuda")
    step = torch.full((1,), 5, dtype=torch.int32, device="cuda")              # step index 4
    stop = torch.zeros(P, 6, dtype=torch.int32, device="cuda")
    stop[:, 5] = -1
    ones = torch.zeros(P, 6, dtype=torch.int32, device="cuda")                # clip records with coef 1: the masked update without the option
    ones[:, 2] = torch.tensor(1.0).view(torch.int32)
    idle = torch.tensor([[3, 0]] * P, dtype=torch.int32, device="cuda")       # best_step 3: no slot takes at step index 4
    take = torch.tensor([[4, 1]] * P, dtype=torch.int32, device="cuda")       # every slot takes
    s = _lib.current_stream()
    head = (0, _lib.ptr(p), _lib.ptr(g), _lib.ptr(g2), _lib.ptr(m), _lib.ptr(v), None, P, stride, n1, _lib.ptr(lrs), 0.0, 0.99, 1e-8, _lib.ptr(step), _lib.ptr(stop),
            0, 0.0, 0)
    def masked():
        return L.splice_optim_step_pairs_clip(*head, _lib.ptr(ones), s)
    def best(rec):
        return lambda: L.splice_optim_step_pairs_best(*head, _lib.ptr(ones), _lib.ptr(rec), _lib.ptr(bp), None, s)
    res = {}
    names = (("masked clipped update, option off", masked), ("snapshot instance, no slot takes", best(idle)), ("snapshot instance, every slot takes", best(take)))
    for rep in range(5):
        for name, fn in names:
            for _ in range(20):
                assert fn() == 0
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(300):
                fn()
            b.record()
            torch.cuda.synchronize()
            res.setdefault(name, []).append(a.elapsed_time(b) / 300 * 1e3)
    for name, _ in names:
        xs = sorted(res[name])
        out.append(f"P={P} n={n} floats {name}: median {xs[2]:.2f} us per launch (min {xs[0]:.2f}, max {xs[-1]:.2f}; 5 x 300 back-to-back launches)")
print("\n".join(out))
