"""Device time per call, forward + backward, of the deep-supervision loss (ft.DeepSupervisionLoss, the level reader of csrc/loss.hip) against
what the package offered before it (profiles/deep_supervision.md), at the head sizes of the two bundles:

    brats   B = 2,  C = 3, levels 128^3 / 64^3 / 32^3, uint8 target at 128^3
    fives   B = 16, C = 1, levels 512^2 / 256^2,       uint8 target at 512^2

Variants, alternating round by round in ONE process after a warm-up of each:

    native        ft.DeepSupervisionLoss(ft.DiceCELoss()) on the list: level 0 through the dense kernels, the coarse levels
                  through the index map
    composed      per level: target.float() (F.interpolate takes no bool, the dense kernels no uint8), F.interpolate
                  nearest-exact, ft.DiceCELoss; the weighted sum — the user's work-around
    single        ft.DiceCELoss on level 0 alone (what a run without deep supervision pays)
    native_again  the first once more: the spread of a repeated baseline

A round is enough calls to fill --window-ms between two HIP events; the time per call is that window over the calls, launch
overhead included.  Also counted, per variant: the native launches, and the bytes the caching allocator hands out during one
call (the down-sampled and converted targets of the composed form show up there).  A run without a GPU fails.

    python tools/bench_deep_supervision.py [--rounds 10] [--window-ms 20] [--only brats] [--out deep_supervision.json]
"""
from __future__ import annotations

import argparse
import json
import math
import os
import statistics
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import factorizer_amd as ft  # noqa: E402
from factorizer_amd import _native, losses  # noqa: E402

SHAPES = {"brats": (2, 3, [(128,) * 3, (64,) * 3, (32,) * 3]),
          "fives": (16, 1, [(512,) * 2, (256,) * 2])}


def window(fn, iters):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    s.record()
    for _ in range(iters):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / iters


def alternate(variants, rounds, window_ms):
    """ms per call of every variant: [per round]; the calls per round come from a first timing of the slowest variant"""
    for fn in variants.values():
        for _ in range(3):
            fn()
    est = max(window(fn, 3) for fn in variants.values())
    iters = max(3, math.ceil(window_ms / max(est, 1e-3)))
    times = {k: [] for k in variants}
    for _ in range(rounds):
        for k, fn in variants.items():
            times[k].append(window(fn, iters))
    return times, iters


def counted(fn):
    """(native launches, bytes allocated) of one call"""
    torch.cuda.synchronize()
    n0, a0 = _native.launch_count(), torch.cuda.memory_stats()["allocated_bytes.all.allocated"]
    fn()
    torch.cuda.synchronize()
    return _native.launch_count() - n0, torch.cuda.memory_stats()["allocated_bytes.all.allocated"] - a0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--window-ms", type=float, default=20.0)
    ap.add_argument("--only", default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_deep_supervision.py measures device time: no GPU found")
    dev = torch.device("cuda:0")
    res = {"device": torch.cuda.get_device_name(0), "rounds": a.rounds, "window_ms": a.window_ms, "rows": []}
    base = ft.DiceCELoss()
    crit = ft.DeepSupervisionLoss(base)
    for bundle, (B, C, levels) in SHAPES.items():
        if a.only and bundle != a.only:
            continue
        torch.manual_seed(0)
        zs = [torch.randn(B, C, *S, device=dev) for S in levels]
        t = (torch.rand(B, C, *levels[0], device=dev) > 0.5).to(torch.uint8)
        w = losses.ds_weights(len(zs), "exp")

        def step(loss_of, n=len(zs)):
            zr = [z.detach().requires_grad_(True) for z in zs[:n]]
            return torch.autograd.grad(loss_of(zr), zr)

        def composed(zr):
            total = 0.0
            for wl, z in zip(w, zr):
                tf = t.float()
                tl = tf if z.shape[2:] == t.shape[2:] else F.interpolate(tf, size=z.shape[2:], mode="nearest-exact")
                total = total + wl * base(z, tl)
            return total

        variants = {"native": lambda: step(lambda zr: crit(zr, t)), "composed": lambda: step(composed),
                    "single": lambda: step(lambda zr: base(zr[0], t), 1),
                    "native_again": lambda: step(lambda zr: crit(zr, t))}
        counts = {k: counted(fn) for k, fn in variants.items()}
        times, iters = alternate(variants, a.rounds, a.window_ms)
        ms = {k: {"median": statistics.median(v), "min": min(v), "max": max(v)} for k, v in times.items()}
        row = {"bundle": bundle, "B": B, "C": C, "levels": [list(S) for S in levels], "target": "uint8", "weights": w,
               "calls_per_round": iters, "ms_per_call": ms,
               "baseline_repeat_rel_diff_median": statistics.median(abs(p - q) / p for p, q in zip(times["native"], times["native_again"])),
               "native_launches": {k: c[0] for k, c in counts.items()}, "allocated_bytes_per_call": {k: c[1] for k, c in counts.items()},
               "native_over_composed": ms["native"]["median"] / ms["composed"]["median"],
               "native_over_single": ms["native"]["median"] / ms["single"]["median"]}
        print(json.dumps(row), flush=True)
        res["rows"].append(row)
        del zs, t
        torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
