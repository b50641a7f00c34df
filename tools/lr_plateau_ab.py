"""usage (GPU box): python tools/lr_plateau_ab.py [--pairs 1] [--rounds 3] [--steps 80] [--warmup 15] [--only on|off] [--first off|on]
The step with the plateau lr rule (`lr_plateau_factor`) off and on, alternating on one box: engines as bench.py builds them (synthetic
weights, 224 x 224 pairs, ViT-B/8, every step with the entire image handed over), `--steps` steps timed between two events behind
`--warmup` steps, `--rounds` rounds of off / on.  Both arms run the stop rule the lr rule needs (windows of 5 counted steps, a patience
no run reaches), so the off arm launches the loss kernel's instance with the stop rule alone and the scalar-lr optimiser instance, the on
arm the instance with both rules and, at several pairs, the per-pair-lr optimiser instance.  `--only` runs one arm alone (a rocprofv3
--kernel-trace --stats run of one arm: the instances' own time, and the kernel launches per step)."""
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
ap.add_argument("--only", choices=("on", "off"), default=None)
ap.add_argument("--first", choices=("on", "off"), default="off", help="the arm that runs first in every round")
a = ap.parse_args()

vit = None
for rnd in range(1, a.rounds + 1):
    for arm in (("off", "on") if a.first == "off" else ("on", "off")):
        if a.only and arm != a.only:
            continue
        cfg = dict(stop_window=5, stop_rel=0.01, stop_patience=10 ** 6, lr_plateau_factor=0.5 if arm == "on" else 0.0, lr_plateau_patience=2,
                   lr_plateau_min_scale=0.5)
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
        cuts = [d["cuts"] for d in eng.lr_state()] if arm == "on" and a.pairs > 1 else [eng.lr_state()["cuts"]] if arm == "on" else []
        print(f"round {rnd} lr_plateau={arm:3s} P={a.pairs} steps/s {1e3 / ms:.3f} ms/step {ms:.4f} wall steps/s {a.steps / wall:.3f} cuts {cuts}", flush=True)
        del eng
