"""Timing of a hyper-parameter sweep of ONE 224 x 224 pair against the two things it replaces or rides on:
uniform K pairs in one MultiPairEngine (same launches, one config), and K serial single-pair runs (SpliceEngine).
Legs alternate within one process (uniform, sweep, single, uniform, sweep, single, ...) so that they share the box state.
Prints one JSON line: pair-steps/s of every leg per round and the medians.

    python tools/sweep_bench.py [--variants 8] [--steps 300] [--warmup 30] [--rounds 3] [--legs uniform,sweep,single]
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from splice_amd import synth  # noqa: E402
from splice_amd.engine import DEFAULT_CFG, MultiPairEngine, SpliceEngine  # noqa: E402
from splice_amd.vit import VitEngine  # noqa: E402

VARIANT_AXES = [dict(lambda_global_ssim=s, lr=lr, scheduler_policy=pol) for s in (1.0, 0.5) for lr in (0.002, 0.004) for pol in ("none", "cosine")]


def _time(eng, A, B, E, steps, warmup):
    for _ in range(warmup):
        eng.step(A, B, E)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        eng.step(A, B, E)
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--variants", type=int, default=8)
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--warmup", type=int, default=30)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--legs", default="uniform,sweep,single", help="legs to run (e.g. uniform,sweep under a kernel profiler: the single leg's "
                                                                 "one-pair launches would mix into the per-kernel statistics)")
    args = ap.parse_args(argv)
    K = args.variants
    cfg = dict(DEFAULT_CFG, dino_model_name="dino_vitb8", dino_global_patch_size=224, n_epochs=args.steps + args.warmup)
    variants = [VARIANT_AXES[k % len(VARIANT_AXES)] for k in range(K)]
    vit = VitEngine("dino_vitb8", device="cuda").load_state_dict(synth.vit_params(1234, "dino_vitb8", img_size=224))
    a, b = synth.image_pair(1234, 0, 224, 224)
    A1, B1 = torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda()
    AK, BK = A1[None].expand(K, -1, -1, -1).contiguous(), B1[None].expand(K, -1, -1, -1).contiguous()
    gens = [synth.generator_params(1235 + k, cfg["init_gain"]) for k in range(K)]
    legs = {k: [] for k in args.legs.split(",")}
    for _ in range(args.rounds):
        if "uniform" in legs:
            eng = MultiPairEngine(cfg, None, gens, (224, 224), (224, 224), vit_engine=vit)
            legs["uniform"].append(K * args.steps / _time(eng, AK, BK, AK, args.steps, args.warmup))
            del eng
        if "sweep" in legs:
            eng = MultiPairEngine(cfg, None, [gens[0]] * K, (224, 224), (224, 224), vit_engine=vit, pair_cfgs=variants)
            legs["sweep"].append(K * args.steps / _time(eng, AK, BK, AK, args.steps, args.warmup))
            del eng
        if "single" in legs:
            eng = SpliceEngine(cfg, None, gens[0], (224, 224), (224, 224), vit_engine=vit)
            legs["single"].append(args.steps / _time(eng, A1, B1, A1, args.steps, args.warmup))
            del eng
    med = {k: round(statistics.median(v), 1) for k, v in legs.items()}
    out = {"variants": K, "steps": args.steps, "rounds": args.rounds, "pair_steps_per_s": {k: [round(x, 1) for x in v] for k, v in legs.items()}, "median": med}
    if "sweep" in med and "uniform" in med:
        out["sweep_vs_uniform"] = round(med["sweep"] / med["uniform"], 4)
    if "sweep" in med and "single" in med:
        out["sweep_time_vs_serial"] = round(med["single"] / med["sweep"], 4)   # wall time of the sweep / K serial single-pair runs
    print(json.dumps(out))


if __name__ == "__main__":
    main()
