"""usage (GPU box): python tools/clip_auto_ab.py [--pairs 1] [--rounds 4] [--steps 80] [--warmup 15] [--clip 1.0] [--k 2.0] [--only off|fixed|auto]
The step without clipping (`off`), with fixed clipping (`fixed`: `grad_clip_norm = --clip`) and with clipping against the pair's running
norm (`auto`: `grad_clip_auto = --k`, warm-up 8, no cap), alternating on one box: engines as bench.py builds them (synthetic weights,
224 x 224 pairs, ViT-B/8, every step with the entire image handed over), `--steps` steps timed between two events behind `--warmup`
steps, `--rounds` rounds.  `--only` runs one arm alone (a rocprofv3 --kernel-trace --stats run of one arm: the instance's own time)."""
import argparse
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from splice_amd.engine import synthetic_engine

ARMS = ("off", "fixed", "auto")
ap = argparse.ArgumentParser()
ap.add_argument("--pairs", type=int, default=1)
ap.add_argument("--rounds", type=int, default=4)
ap.add_argument("--steps", type=int, default=80)
ap.add_argument("--warmup", type=int, default=15)
ap.add_argument("--clip", type=float, default=1.0)
ap.add_argument("--k", type=float, default=2.0)
ap.add_argument("--only", choices=ARMS, default=None)
a = ap.parse_args()

vit = None
for rnd in range(1, a.rounds + 1):
    for arm in ARMS:
        if a.only and arm != a.only:
            continue
        cfg = dict(grad_clip_norm=a.clip if arm == "fixed" else 0.0, grad_clip_auto=a.k if arm == "auto" else 0.0, n_epochs=10000)
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
        note = ""
        if arm != "off":
            recs = eng.clip_state() if a.pairs > 1 else [eng.clip_state()]
            note = f" clipped {[r['clipped'] for r in recs]}"
        if arm == "auto":
            autos = eng.clip_auto_state() if a.pairs > 1 else [eng.clip_auto_state()]
            note += f" ref {[[round(float(x), 4) for x in r['ref']] for r in autos]}"
        print(f"round {rnd} clip={arm:5s} P={a.pairs} steps/s {1e3 / ms:.3f} ms/step {ms:.4f} wall steps/s {a.steps / wall:.3f}{note}", flush=True)
        del eng
