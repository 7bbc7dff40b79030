"""Device time per call, forward + backward, of the class-index DiceCE (ft.DiceCELoss(softmax=True, to_onehot_y=True), the
dice_sce_* kernels of csrc/loss.hip) against the composed framework form on the same device in the same process, and of the
multi-class metrics pass (fz_seg_argmax) against composed argmax + one-hot + counts (profiles/softmax_loss.md):

    amos     B = 2,  C = 16, 128^3, uint8 labels      (AMOS22-like: 16 classes)
    three    B = 2,  C = 3,  128^3, uint8 labels      + the sigmoid ft.dice_ce_loss kernels at this shape as the yardstick
    slices   B = 16, C = 2,  512^2, uint8 labels

Variants, alternating round by round after a warm-up of each (tools/bench_deep_supervision.py has the scheme):

    native        ft.dice_ce_softmax_loss: sums pass, finish (B <= 8), gradient pass
    composed      softmax -> masked one-hot -> Dice -> F.cross_entropy(ignore_index) in framework ops
    native_again  the first once more: the spread of a repeated baseline
    sigmoid       (three only) ft.dice_ce_loss on a float multi-label target of the same shape

Per native pass: its event-timed device time (functional.KernelTimer) and its algorithmic bytes — sums 4·numel + label
bytes, gradient 8·numel + label bytes — over that time, as a fraction of the device-copy rate measured in the same process
(a 1 GiB fp32 tensor copied to another: 2 bytes moved per byte copied).  Per variant: the native launches and the bytes the
caching allocator hands out during one call.  A run without a GPU fails.

    python tools/bench_softmax_loss.py [--rounds 10] [--window-ms 100] [--only amos] [--out softmax_loss.json]
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import factorizer_amd as ft  # noqa: E402
from factorizer_amd import functional as Fn  # noqa: E402
from bench_deep_supervision import alternate, counted, window  # noqa: E402

SHAPES = {"amos": (2, 16, (128,) * 3), "three": (2, 3, (128,) * 3), "slices": (16, 2, (512,) * 2)}


def composed_loss(z, y, smooth=1e-5):
    """the framework form a user writes without the package: every intermediate is a full tensor"""
    C = z.shape[1]
    idx = y[:, 0].long()
    ok = (idx >= 0) & (idx < C)
    t = (F.one_hot(torch.where(ok, idx, torch.zeros_like(idx)), C).movedim(-1, 1) * ok.unsqueeze(1)).to(z.dtype)
    p = torch.softmax(z, dim=1)
    dims = tuple(range(2, z.ndim))
    dice = (1.0 - (2.0 * (p * t).sum(dims) + smooth) / (p.sum(dims) + t.sum(dims) + smooth)).mean()
    ce = F.cross_entropy(z, torch.where(ok, idx, torch.full_like(idx, -100)), ignore_index=-100, reduction="sum") / ok.numel()
    return dice + ce


def composed_counts(x, y):
    C = x.shape[1]
    m = x.amax(1, keepdim=True)
    cls = torch.arange(C, device=x.device).view(1, C, *([1] * (x.dim() - 2)))
    p = torch.where(x == m, cls, C).amin(1)
    P = F.one_hot(p, C).movedim(-1, 1).bool()
    Y = F.one_hot(y[:, 0].long(), C).movedim(-1, 1).bool()
    dims = tuple(range(2, x.dim()))
    return torch.stack([(P & Y).sum(dims), P.sum(dims), Y.sum(dims)], dim=-1)


def copy_rate():
    """bytes per second moved by a device copy of 1 GiB (read + write), median of 10 windows of 5"""
    a = torch.empty(1 << 28, dtype=torch.float32, device="cuda:0")
    b = torch.empty_like(a)
    for _ in range(3):
        b.copy_(a)
    ms = statistics.median(window(lambda: b.copy_(a), 5) for _ in range(10))
    return 2 * a.numel() * 4 / (ms * 1e-3)


def passes(fn, reps=10):
    """per native kernel name: (median ms per launch, algorithmic bytes per launch) over `reps` timed calls"""
    per = {}
    for _ in range(reps):
        timer = Fn.KernelTimer()
        Fn.set_timer(timer)
        try:
            fn()
        finally:
            Fn.set_timer(None)
        for k, v in timer.summary().items():
            per.setdefault(k, []).append((v["ms"] / v["calls"], v["bytes"] // v["calls"]))
    return {k: {"ms": statistics.median(t for t, _ in v), "bytes": v[0][1]} for k, v in per.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--window-ms", type=float, default=100.0)
    ap.add_argument("--only", default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_softmax_loss.py measures device time: no GPU found")
    dev = torch.device("cuda:0")
    rate = copy_rate()
    res = {"device": torch.cuda.get_device_name(0), "rounds": a.rounds, "window_ms": a.window_ms,
           "copy_rate_GBps": rate / 1e9, "rows": []}
    print(json.dumps({"copy_rate_GBps": rate / 1e9}), flush=True)
    for name, (B, C, S) in SHAPES.items():
        if a.only and name != a.only:
            continue
        torch.manual_seed(0)
        z = torch.randn(B, C, *S, device=dev)
        y = torch.randint(0, C, (B, 1, *S), device=dev).to(torch.uint8)

        def step(loss_of, zz=z):
            zr = zz.detach().requires_grad_(True)
            return torch.autograd.grad(loss_of(zr), zr)

        variants = {"native": lambda: step(lambda zr: ft.dice_ce_softmax_loss(zr, y)),
                    "composed": lambda: step(lambda zr: composed_loss(zr, y)),
                    "native_again": lambda: step(lambda zr: ft.dice_ce_softmax_loss(zr, y))}
        if name == "three":
            t = (torch.rand(B, C, *S, device=dev) > 0.5).float()
            variants["sigmoid"] = lambda: step(lambda zr: ft.dice_ce_loss(zr, t))
        counts = {k: counted(fn) for k, fn in variants.items()}
        times, iters = alternate(variants, a.rounds, a.window_ms)
        ms = {k: {"median": statistics.median(v), "min": min(v), "max": max(v)} for k, v in times.items()}
        per = passes(variants["native"])
        if name == "three":
            per.update(passes(variants["sigmoid"]))
        for v in per.values():
            v["GBps"] = v["bytes"] / (v["ms"] * 1e-3) / 1e9
            v["of_copy_rate"] = v["GBps"] * 1e9 / rate
        row = {"shape": name, "B": B, "C": C, "spatial": list(S), "labels": "uint8", "calls_per_round": iters, "ms_per_call": ms,
               "baseline_repeat_rel_diff_median": statistics.median(abs(p - q) / p for p, q in zip(times["native"], times["native_again"])),
               "native_launches": {k: c[0] for k, c in counts.items()}, "allocated_bytes_per_call": {k: c[1] for k, c in counts.items()},
               "native_over_composed": ms["native"]["median"] / ms["composed"]["median"], "passes": per}
        if name == "amos":
            mv = {"native": lambda: ft.multiclass_counts(z, y), "composed": lambda: composed_counts(z, y),
                  "native_again": lambda: ft.multiclass_counts(z, y)}
            assert torch.equal(mv["native"](), mv["composed"]())
            mc = {k: counted(fn) for k, fn in mv.items()}
            mt, mi = alternate(mv, a.rounds, a.window_ms)
            mm = {k: {"median": statistics.median(v), "min": min(v), "max": max(v)} for k, v in mt.items()}
            mp = passes(mv["native"])
            for v in mp.values():
                v["GBps"] = v["bytes"] / (v["ms"] * 1e-3) / 1e9
                v["of_copy_rate"] = v["GBps"] * 1e9 / rate
            row["metrics"] = {"calls_per_round": mi, "ms_per_call": mm, "native_over_composed": mm["native"]["median"] / mm["composed"]["median"],
                              "allocated_bytes_per_call": {k: c[1] for k, c in mc.items()}, "passes": mp}
        print(json.dumps(row), flush=True)
        res["rows"].append(row)
        del z, y
        torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
