"""usage (GPU box): python tools/image_terms_ab.py [--pairs 1] [--rounds 4] [--steps 80] [--warmup 15] [--tv 0.1] [--pix 1.0] [--only off|tv|pix|both]
The step without the image-space loss terms (`off`), with the total variation of x' (`tv`: `lambda_global_tv = --tv`), with the pixel
identity of y' (`pix`: `lambda_global_pixel_identity = --pix`) and with both, alternating on one box: engines as bench.py builds them
(synthetic weights, 224 x 224 pairs, ViT-B/8, every step with the entire image handed over), `--steps` steps timed between two events behind
`--warmup` steps, `--rounds` rounds.  `--only` runs one arm alone (a rocprofv3 --kernel-trace --stats run of one arm: the launches' own time)."""
import argparse
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from splice_amd.engine import synthetic_engine

ARMS = ("off", "tv", "pix", "both")
ap = argparse.ArgumentParser()
ap.add_argument("--pairs", type=int, default=1)
ap.add_argument("--rounds", type=int, default=4)
ap.add_argument("--steps", type=int, default=80)
ap.add_argument("--warmup", type=int, default=15)
ap.add_argument("--tv", type=float, default=0.1)
ap.add_argument("--pix", type=float, default=1.0)
ap.add_argument("--only", choices=ARMS, default=None)
a = ap.parse_args()

vit = None
for rnd in range(1, a.rounds + 1):
    for arm in ARMS:
        if a.only and arm != a.only:
            continue
        cfg = dict(lambda_global_tv=a.tv if arm in ("tv", "both") else 0.0, lambda_global_pixel_identity=a.pix if arm in ("pix", "both") else 0.0,
                   n_epochs=10000)
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
        note = f" loss {[round(float(r[0]), 5) for r in rows]} tv {[round(float(r[6]), 6) for r in rows]} pix {[round(float(r[7]), 6) for r in rows]}"
        print(f"round {rnd} terms={arm:4s} P={a.pairs} steps/s {1e3 / ms:.3f} ms/step {ms:.4f} wall steps/s {a.steps / wall:.3f}{note}", flush=True)
        del eng
