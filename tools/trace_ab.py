"""usage (GPU box): python tools/trace_ab.py [--pairs 1] [--rounds 3] [--steps 80] [--warmup 15] [--clip 0.0] [--only on|off] [--first off|on]
The step with the loss trace (`loss_trace`) off and on, alternating on one box: engines as bench.py builds them (synthetic weights, 224 x 224
pairs, ViT-B/8, every step with the entire image handed over), `--steps` steps timed between two events behind `--warmup` steps, `--rounds`
rounds of off / on.  `--clip c` runs both arms with `grad_clip_norm = c`, so the norm launch's trace instance is in the timed step too.
`--only` runs one arm alone (a rocprofv3 --kernel-trace --stats run of one arm: the two instances' own time)."""
import argparse
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from splice_amd.engine import synthetic_engine

ap = argparse.ArgumentParser()
ap.add_argument("--pairs", type=int, default=1)
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--steps", type=int, default=80)
ap.add_argument("--warmup", type=int, default=15)
ap.add_argument("--clip", type=float, default=0.0)
ap.add_argument("--only", choices=("on", "off"), default=None)
ap.add_argument("--first", choices=("on", "off"), default="off", help="the arm that runs first in every round")
a = ap.parse_args()

vit = None
for rnd in range(1, a.rounds + 1):
    for arm in (("off", "on") if a.first == "off" else ("on", "off")):
        if a.only and arm != a.only:
            continue
        cfg = dict(loss_trace=arm == "on", grad_clip_norm=a.clip, n_epochs=10000)
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
        rows = len(eng.loss_trace(0)) if arm == "on" else 0
        print(f"round {rnd} trace={arm:3s} P={a.pairs} clip={a.clip:g} steps/s {1e3 / ms:.3f} ms/step {ms:.4f} wall steps/s {a.steps / wall:.3f} trace rows {rows}", flush=True)
        del eng
