"""usage (GPU box): python tools/compact_measure.py --mode compact|staging|checkpoint|train_pairs [...]
The measurements of pair snapshots, engines as bench.py builds them (synthetic weights, 224 x 224 pairs, ViT-B/8).

--mode compact [--steps 30]: an 8-pair engine under a stop rule no slot reaches.  Times `--steps` steps at 8 pairs, then compact()
    8 -> 4 -- the rebuild alone (waits for the device on both sides), every step behind it one by one until a graph replays again, and
    `--steps` steps at 4 pairs -- then 4 -> 1 alike.  Which slots leave is set on the host's copy of the stop steps: what compact() costs does
    not depend on why a slot left.  Prints the per-step saving and the number of steps after which a compaction has paid for itself.
--mode staging --form flat|gather --pairs P: P pairs, `--steps` steps; gather: the handle picks its P pairs out of 8-pair batches (rows
    0, 2, ..).  One form per process: what a `rocprofv3 --kernel-trace --stats` run of the staging launch takes.
--mode checkpoint --pairs P: the stall of train.save_checkpoint (host snapshots of every slot under every rule, written and moved into
    place), three times, and the file's size.
--mode train_pairs --compact on|off [--pairs 8] [--epochs 240] [--window 5] [--rel 0.02]: wall time of one train_pairs run on synthetic pairs whose slots stop at
    different windows, and the stop steps.  One arm per process, alternate the arms."""
import argparse
import os
import sys
import tempfile
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from splice_amd import _lib, synth
from splice_amd.engine import synthetic_engine

ap = argparse.ArgumentParser()
ap.add_argument("--mode", choices=("compact", "staging", "checkpoint", "train_pairs"), required=True)
ap.add_argument("--pairs", type=int, default=8)
ap.add_argument("--steps", type=int, default=30)
ap.add_argument("--form", choices=("flat", "gather"), default="flat")
ap.add_argument("--compact", choices=("on", "off"), default="off")
ap.add_argument("--epochs", type=int, default=240)
ap.add_argument("--rel", type=float, default=0.02)
ap.add_argument("--window", type=int, default=5)
a = ap.parse_args()
RULES = dict(stop_window=5, stop_rel=0.01, stop_patience=10 ** 6)


def timed_steps(eng, inputs, n):
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        eng.step(*inputs)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n


if a.mode == "compact":
    eng, A, B = synthetic_engine(RULES, pairs=8)
    inputs = (A, B, A)
    for _ in range(15):
        eng.step(*inputs)
    step_ms = {8: timed_steps(eng, inputs, a.steps)}
    print(f"P=8 ms/step {step_ms[8]:.3f}", flush=True)
    for leave, left in (([4, 5, 6, 7], 4), ([1, 2, 3], 1)):
        before = len(eng.live)
        eng._stops()
        for p in leave:
            eng._stopped[p] = eng.step_idx
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        assert eng.compact() and len(eng.live) == left
        torch.cuda.synchronize()
        rebuild = (time.perf_counter() - t0) * 1e3
        firsts = []
        for _ in range(6):                      # eager steps, the captures, the first replays: wall time of each, the device drained
            t0 = time.perf_counter()
            eng.step(*inputs)
            torch.cuda.synchronize()
            firsts.append((time.perf_counter() - t0) * 1e3)
        step_ms[left] = timed_steps(eng, inputs, a.steps)
        saving = step_ms[before] - step_ms[left]
        extra = rebuild + sum(t - step_ms[left] for t in firsts)
        print(f"compact {before} -> {left}: rebuild {rebuild:.1f} ms, first steps behind it {' '.join(f'{t:.1f}' for t in firsts)} ms, then P={left} ms/step {step_ms[left]:.3f}; "
              f"saving {saving:.3f} ms/step, cost {extra:.1f} ms = {extra / saving:.0f} steps to pay for itself", flush=True)
elif a.mode == "staging":
    eng, A, B = synthetic_engine({}, pairs=a.pairs)
    if a.pairs == 1:
        A, B = A[None], B[None]
    if a.form == "gather":
        rows = [2 * p for p in range(a.pairs)] if a.pairs <= 4 else list(range(a.pairs))
        n_in = 8
        big_a, big_b = torch.rand(n_in, *A.shape[1:], device=A.device), torch.rand(n_in, *B.shape[1:], device=B.device)
        for p, r in enumerate(rows):
            big_a[r], big_b[r] = A[p], B[p]
        _lib.check(_lib.lib().splice_step_set_input_rows(eng.handle, n_in, (_lib.C.c_int * a.pairs)(*rows)), "set_input_rows")
        eng.P_in, A, B = n_in, big_a, big_b
    inputs = (A, B, A)
    for _ in range(10):
        eng.step(*inputs)
    print(f"staging form={a.form} P={a.pairs} ms/step {timed_steps(eng, inputs, a.steps):.3f} loss {eng.losses_dev[0, 0].item():.6f}", flush=True)
elif a.mode == "checkpoint":
    from splice_amd.train import save_checkpoint
    rules = dict(RULES, stop_keep_best=True, ema_decay=0.99, grad_clip_norm=1.0, loss_trace=True, lr_plateau_factor=0.5, n_epochs=2000)
    eng, A, B = synthetic_engine(rules, pairs=a.pairs)
    for _ in range(20):
        eng.step(A, B, A)
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "checkpoint.pt")
        stalls = []
        for _ in range(3):
            for _ in range(5):
                eng.step(A, B, A)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            save_checkpoint(path, eng, None, eng.step_idx + 1)
            stalls.append((time.perf_counter() - t0) * 1e3)
        print(f"checkpoint P={a.pairs}: stall {' '.join(f'{t:.1f}' for t in stalls)} ms, file {os.path.getsize(path) / 2 ** 20:.1f} MiB (every rule on, trace of 2000 rows)", flush=True)
else:
    from PIL import Image
    from splice_amd.train import train_pairs
    os.environ.setdefault("SPLICE_SYNTHETIC_WEIGHTS", "1")
    with tempfile.TemporaryDirectory() as d:
        roots = []
        for p in range(a.pairs):
            A, B = synth.smooth_image_pair(60, p, 224, 224)
            for side, img in (("A", A), ("B", B)):
                os.makedirs(os.path.join(d, f"p{p}", side))
                Image.fromarray((img.transpose(1, 2, 0) * 255).astype(np.uint8)).save(os.path.join(d, f"p{p}", side, "img.png"))
            roots.append(os.path.join(d, f"p{p}"))
        over = dict(seed=3, n_epochs=a.epochs, log_images_freq=50, use_augmentations=True, stop_window=a.window, stop_patience=2, stop_rel=a.rel, entire_A_every=75,
                    stop_compact=a.compact == "on")
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        eng = train_pairs(roots, cfg_overrides=over, progress=False)
        torch.cuda.synchronize()
        wall = time.perf_counter() - t0
        print(f"train_pairs P={a.pairs} stop_compact={a.compact} stop_window {a.window} stop_rel {a.rel}: wall {wall:.2f} s, {eng.step_idx + 1} steps, stop steps {eng.stopped_at}, live at the end {eng.live}", flush=True)
