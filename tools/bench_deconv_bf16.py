"""Device time of the Deconver mixer (ft.Deconv forward + backward) on bf16 against fp32 activation storage
(profiles/deconv_bf16.md), on the recipes' stage-0 shapes:

    brats   C = 32, groups = -1 (depthwise), ratio 1, kernel 3^3, 128^3, B = 2     (model_zoo/deconver_brats23, num_iters 1)
    fives   C = 32, groups = -1,             ratio 1, kernel 7^2, 512^2, B = 16    (model_zoo/deconver_fives,   num_iters 1)

Variants, alternating round by round in ONE process after a warm-up of each:
    fp32            this library on float32 activations
    bf16            this library on bfloat16 activations (native kernels, functional.GCorrMuFn for the update)
    bf16_framework  what a bfloat16 input met before the native bf16 kernels: the same layer evaluated with framework grouped
                    convolutions and three elementwise ops under torch.autocast("cuda", bfloat16) (the linear stays native)
    fp32_again      the first variant once more: the spread of a repeated baseline
A round is --iters forward + backward passes between two HIP events.  The launches of the grouped-correlation family alone
come from the library's KernelTimer (a separate pass): ms per launch, bytes per launch from the shapes (what _timed records:
every activation tensor read or written once, filters ignored), and the achieved rate against a device-to-device copy of
the same process.  With --fp32-only the tool times the fp32 variant alone through the public entry points that every revision
of the package has (to compare two checkouts run it once in each).  A run without a GPU fails.

    python tools/bench_deconv_bf16.py [--rounds 10] [--iters 5] [--only brats] [--out deconv_bf16_bench.json]
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import factorizer_amd as ft  # noqa: E402
from factorizer_amd import functional as Fn  # noqa: E402

BF = torch.bfloat16
SHAPES = {
    "brats": dict(B=2, C=32, kernel=(3, 3, 3), S=(128, 128, 128)),
    "fives": dict(B=16, C=32, kernel=(7, 7), S=(512, 512)),
}


def framework_layer(m, x):
    """ft.Deconv(groups=-1, ratio=1, num_iters=1) with framework grouped convolutions under bf16 autocast"""
    conv = F.conv3d if len(m.kernel_size) == 3 else F.conv2d
    C = m.channels
    with torch.autocast("cuda", dtype=BF):
        s = F.relu(m.init.linear(x))
        h = F.relu(m.init.h0)                                        # (C, 1, *k): depthwise
        hT = torch.flip(h, dims=tuple(range(2, h.ndim)))
        num = conv(x, hT, padding=m.padding, groups=C) + m.eps
        r = conv(s, h, padding=m.padding, groups=C)
        return s * num / (conv(r, hT, padding=m.padding, groups=C) + m.eps)


def copy_rate(dev):
    """bytes/s moved by a device-to-device copy of 1 GiB (read + write counted)"""
    a = torch.empty(1 << 28, dtype=torch.float32, device=dev)
    b = torch.empty_like(a)
    for _ in range(3):
        b.copy_(a)
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(10):
        b.copy_(a)
    e.record()
    torch.cuda.synchronize()
    return 2 * a.numel() * 4 * 10 / (s.elapsed_time(e) * 1e-3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--only", default=None)
    ap.add_argument("--fp32-only", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_deconv_bf16.py measures device time: no GPU found")
    dev = torch.device("cuda:0")
    res = {"device": torch.cuda.get_device_name(0), "rounds": a.rounds, "iters": a.iters, "copy_bytes_per_s": copy_rate(dev),
           "cases": {}}
    for name, sh in SHAPES.items():
        if a.only and name != a.only:
            continue
        torch.manual_seed(0)
        m = ft.Deconv(channels=sh["C"], groups=-1, ratio=1, kernel_size=sh["kernel"], num_iters=1).to(dev)
        x32 = torch.rand(sh["B"], sh["C"], *sh["S"], device=dev)
        g32 = torch.rand_like(x32)
        params = list(m.parameters())

        def step(x, g, layer):
            x = x.detach().requires_grad_(True)
            y = layer(x)
            return torch.autograd.grad(y, [x] + params, g)

        variants = {"fp32": lambda: step(x32, g32, m)}
        if not a.fp32_only:
            x16, g16 = x32.to(BF), g32.to(BF)
            variants["bf16"] = lambda: step(x16, g16, m)
            variants["bf16_framework"] = lambda: step(x16, g16, lambda x: framework_layer(m, x))
        variants["fp32_again"] = variants["fp32"]
        for fn in variants.values():                                   # warm-up: every kernel loaded, allocator settled
            for _ in range(3):
                fn()
        times = {k: [] for k in variants}
        for _ in range(a.rounds):
            for k, fn in variants.items():
                s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()
                s.record()
                for _ in range(a.iters):
                    fn()
                e.record()
                torch.cuda.synchronize()
                times[k].append(s.elapsed_time(e) / a.iters)
        case = {"shape": {k: (list(v) if isinstance(v, tuple) else v) for k, v in sh.items()},
                "ms_per_fwd_bwd_median": {k: statistics.median(v) for k, v in times.items()},
                "ms_per_fwd_bwd_min": {k: min(v) for k, v in times.items()},
                "baseline_repeat_rel_diff_median": statistics.median(abs(p - q) / p for p, q in zip(times["fp32"], times["fp32_again"]))}
        # the launches of the family alone
        launches = {}
        for k in [v for v in ("fp32", "bf16") if v in variants]:
            timer = Fn.KernelTimer()
            Fn.set_timer(timer)
            for _ in range(a.iters):
                variants[k]()
            Fn.set_timer(None)
            agg = timer.summary()
            launches[k] = {n: {"calls_per_pass": v["calls"] / a.iters, "ms_per_launch": v["ms"] / v["calls"],
                               "bytes_per_launch": v["bytes"] / v["calls"],
                               "bytes_per_s": v["bytes"] / (v["ms"] * 1e-3),
                               "of_copy_rate": v["bytes"] / (v["ms"] * 1e-3) / res["copy_bytes_per_s"]}
                           for n, v in agg.items() if n.startswith("gcorr")}
        case["gcorr_launches"] = launches
        print(name, json.dumps(case), flush=True)
        res["cases"][name] = case
        del m, x32, g32, variants
        torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
