"""usage (GPU box): python tools/key_nn_ab.py [--pairs 1] [--rounds 4] [--steps 80] [--warmup 15] [--layer 11] [--lam 1.0] [--only off|on]
The step without the nearest-neighbour key appearance term (`off`: the keys absent) and with it on block `--layer` (`on`:
`lambda_global_key_nn`, `dino_nn_layer`), alternating on one box: engines as bench.py builds them (synthetic weights, 224 x 224 pairs,
ViT-B/8, every step with the entire image handed over, `cls_warmup` 0 so that the term runs from the first step), `--steps` steps timed
between two events behind `--warmup` steps, `--rounds` rounds.  `--only` runs one arm alone (one arm per process; also for a rocprofv3
--kernel-trace --stats run of one arm: the launches' own time)."""
import argparse
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from splice_amd.engine import synthetic_engine

ARMS = ("off", "on")
ap = argparse.ArgumentParser()
ap.add_argument("--pairs", type=int, default=1)
ap.add_argument("--rounds", type=int, default=4)
ap.add_argument("--steps", type=int, default=80)
ap.add_argument("--warmup", type=int, default=15)
ap.add_argument("--layer", type=int, default=11)
ap.add_argument("--lam", type=float, default=1.0)
ap.add_argument("--only", choices=ARMS, default=None)
a = ap.parse_args()

on_keys = {"lambda_global_key_nn": a.lam, "dino_nn_layer": a.layer}
vit = None
for rnd in range(1, a.rounds + 1):
    for arm in (ARMS if rnd % 2 else ARMS[::-1]):   # (the order swapped every round)
        if a.only and arm != a.only:
            continue
        cfg = dict(n_epochs=10000, cls_warmup=0, **(on_keys if arm == "on" else {}))
        eng, A, B = synthetic_engine(cfg, pairs=a.pairs, vit_engine=vit)
        vit = eng.vit
        for _ in range(a.warmup):
            eng.step(A, B, A)
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        e0.record()
        for _ in range(a.steps):
            eng.step(A, B, A)
        e1.record()
        torch.cuda.synchronize()
        wall = time.perf_counter() - t0
        ms = e0.elapsed_time(e1) / a.steps
        rows = eng.losses_dev.cpu()
        note = f" loss {[round(float(r[0]), 5) for r in rows]}"
        if arm == "on":
            vals = eng.key_nn_value()
            note += f" key_nn {[round(float(v), 6) for v in (vals if isinstance(vals, list) else [vals])]}"
        print(f"round {rnd} key_nn={'off' if arm == 'off' else 'block %d' % a.layer:8s} P={a.pairs} steps/s {1e3 / ms:.3f} ms/step {ms:.4f} wall steps/s {a.steps / wall:.3f}{note}", flush=True)
        del eng
