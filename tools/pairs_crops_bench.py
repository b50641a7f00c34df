"""Timing of several 224 x 224 pairs with n_crops = 2 global crops each in ONE MultiPairEngine (one netG call per pair's crops,
every launch shared) against one pair with n_crops = 2 and the serial equivalent (single-pair n_crops = 2 engines stepped in
turn).  Fixed crops, so every leg replays a captured graph.  Legs alternate within one process (one pair, P = 2, 4, 8, serial,
one pair, ...) so that they share the box state.  Prints one JSON line: pair-steps/s of every leg per round, the medians and the
ratio of every leg to serial.

    python tools/pairs_crops_bench.py [--pairs 2,4,8] [--n-crops 2] [--steps 200] [--warmup 20] [--rounds 3] [--serial-engines 4]
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


def _time(engs, inputs, steps, warmup):
    """seconds for `steps` steps of every engine, stepped in turn"""
    for _ in range(warmup):
        for eng, (A, B, E) in zip(engs, inputs):
            eng.step(A, B, E)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        for eng, (A, B, E) in zip(engs, inputs):
            eng.step(A, B, E)
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--pairs", default="2,4,8")
    ap.add_argument("--n-crops", type=int, default=2)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--serial-engines", type=int, default=4, help="single-pair engines stepped in turn by the serial leg")
    ap.add_argument("--legs", default="one,pairs,serial", help="legs to run (e.g. pairs alone under a kernel profiler)")
    args = ap.parse_args(argv)
    n = args.n_crops
    Ps = [int(p) for p in args.pairs.split(",")]
    cfg = dict(DEFAULT_CFG, dino_model_name="dino_vitb8", dino_global_patch_size=224, n_epochs=args.steps + args.warmup)
    vit = VitEngine("dino_vitb8", device="cuda").load_state_dict(synth.vit_params(1234, "dino_vitb8", img_size=224))
    a, b = synth.image_pair(1234, 0, 224, 224)
    A1, B1 = torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda()
    Pmax = max(Ps + [args.serial_engines])
    gens = [synth.generator_params(1235 + k, cfg["init_gain"]) for k in range(Pmax)]

    def crops(P):   # [P*n,3,224,224] crops (the full image, fixed) and [P,3,224,224] entire images
        return (A1[None].expand(P * n, -1, -1, -1).contiguous(), B1[None].expand(P * n, -1, -1, -1).contiguous(),
                A1[None].expand(P, -1, -1, -1).contiguous())

    want = args.legs.split(",")
    legs = {}
    if "one" in want:
        legs["one"] = []
    if "pairs" in want:
        legs.update({f"P{P}": [] for P in Ps})
    if "serial" in want:
        legs["serial"] = []
    for _ in range(args.rounds):
        if "one" in legs:
            eng = SpliceEngine(cfg, None, gens[0], (224, 224), (224, 224), vit_engine=vit, n_crops=n)
            A, B, E = crops(1)
            legs["one"].append(args.steps / _time([eng], [(A, B, E[0])], args.steps, args.warmup))
            del eng
        for P in Ps if "pairs" in want else []:
            eng = MultiPairEngine(cfg, None, gens[:P], (224, 224), (224, 224), vit_engine=vit, n_crops=n)
            legs[f"P{P}"].append(P * args.steps / _time([eng], [crops(P)], args.steps, args.warmup))
            del eng
        if "serial" in legs:
            S = args.serial_engines
            engs = [SpliceEngine(cfg, None, gens[k], (224, 224), (224, 224), vit_engine=vit, n_crops=n) for k in range(S)]
            A, B, E = crops(1)
            legs["serial"].append(S * args.steps / _time(engs, [(A, B, E[0])] * S, args.steps, args.warmup))
            del engs
    med = {k: round(statistics.median(v), 1) for k, v in legs.items()}
    out = {"n_crops": n, "steps": args.steps, "rounds": args.rounds, "pair_steps_per_s": {k: [round(x, 1) for x in v] for k, v in legs.items()},
           "median": med}
    if "serial" in med:
        out["vs_serial"] = {k: round(v / med["serial"], 3) for k, v in med.items()}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
