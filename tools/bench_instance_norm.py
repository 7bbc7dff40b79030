"""Device time per call of the native instance norm (ft.InstanceNorm*d, csrc/inorm.hip) against nn.InstanceNorm*d on the same
device (profiles/instance_norm.md), on the ten block-norm shapes of the Deconver bundles:

    brats   B = 2,  (C, 128^3 / 64^3 / 32^3 / 16^3 / 8^3)  for C = 32 / 64 / 128 / 256 / 512   (model_zoo/deconver_brats23)
    fives   B = 16, (C, 512^2 / 256^2 / 128^2 / 64^2 / 32^2) for the same widths                (model_zoo/deconver_fives)

Per shape, in fp32 and bf16: the forward alone (no graph kept) and forward + backward (input gradient), default arguments
(affine=False).  Variants alternate round by round in ONE process after a warm-up of each: native, framework, native_again (the
spread of a repeated baseline).  A round is enough calls to fill --window-ms between two HIP events; the time per call is that
window over the calls, launch overhead included.  Next to each time: the bytes the native kernels move, from the shapes (a
plane of V <= fz_inorm_one_pass_max() is read once per direction and tensor, a larger one twice; one write), over the time,
against a device-to-device copy of 1 GiB in the same process.  One more row: forward + backward of the BraTS-size ft.Deconver
(4 -> 3 channels, 2 x 128^3) with norm=nn.InstanceNorm3d against the same model through ft.convert_instance_norm.  A run without
a GPU fails.

    python tools/bench_instance_norm.py [--rounds 10] [--window-ms 20] [--only brats] [--no-network] [--out instance_norm.json]
"""
from __future__ import annotations

import argparse
import copy
import json
import math
import os
import statistics
import sys

import torch
from torch import nn

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import factorizer_amd as ft  # noqa: E402
from factorizer_amd import _native  # noqa: E402

WIDTHS = (32, 64, 128, 256, 512)
SHAPES = {"brats": [(2, c, (128 >> i,) * 3) for i, c in enumerate(WIDTHS)],
          "fives": [(16, c, (512 >> i,) * 2) for i, c in enumerate(WIDTHS)]}


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


def summary(times):
    out = {k: {"median": statistics.median(v), "min": min(v), "max": max(v)} for k, v in times.items()}
    out["baseline_repeat_rel_diff_median"] = statistics.median(abs(p - q) / p for p, q in zip(times["native"], times["native_again"]))
    return out


def native_bytes(numel, esize, V, backward):
    reads = 1 if V <= _native.lib().fz_inorm_one_pass_max() else 2
    n = reads + 1                      # forward: x (once or twice), y
    if backward:
        n += 2 * reads + 1             # x and g (once or twice each), gx
    return n * numel * esize


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--window-ms", type=float, default=20.0)
    ap.add_argument("--only", default=None)
    ap.add_argument("--no-network", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_instance_norm.py measures device time: no GPU found")
    dev = torch.device("cuda:0")
    res = {"device": torch.cuda.get_device_name(0), "rounds": a.rounds, "window_ms": a.window_ms,
           "copy_bytes_per_s": copy_rate(dev), "one_pass_max": _native.lib().fz_inorm_one_pass_max(), "rows": []}
    for bundle, shapes in SHAPES.items():
        if a.only and bundle != a.only:
            continue
        for B, C, S in shapes:
            mine = getattr(ft, f"InstanceNorm{len(S)}d")(C).to(dev)
            theirs = getattr(nn, f"InstanceNorm{len(S)}d")(C).to(dev)
            for dtype in (torch.float32, torch.bfloat16):
                torch.manual_seed(0)
                x = torch.randn(B, C, *S, device=dev).to(dtype)
                g = torch.randn(B, C, *S, device=dev).to(dtype)
                V = x[0, 0].numel()

                def fwd(m):
                    with torch.no_grad():
                        return m(x)

                def fwd_bwd(m):
                    xr = x.detach().requires_grad_(True)
                    return torch.autograd.grad(m(xr), xr, g)

                for mode, step in (("fwd", fwd), ("fwd_bwd", fwd_bwd)):
                    variants = {"native": lambda: step(mine), "framework": lambda: step(theirs), "native_again": lambda: step(mine)}
                    n0 = _native.launch_count()
                    step(mine)
                    launches = _native.launch_count() - n0
                    times, iters = alternate(variants, a.rounds, a.window_ms)
                    nbytes = native_bytes(x.numel(), x.element_size(), V, mode == "fwd_bwd")
                    ms = summary(times)
                    row = {"bundle": bundle, "B": B, "C": C, "spatial": list(S), "V": V, "dtype": str(dtype).replace("torch.", ""),
                           "mode": mode, "calls_per_round": iters, "native_launches": launches, "ms_per_call": ms,
                           "native_over_framework": ms["native"]["median"] / ms["framework"]["median"],
                           "native_bytes": nbytes, "native_bytes_per_s": nbytes / (ms["native"]["median"] * 1e-3)}
                    row["native_of_copy_rate"] = row["native_bytes_per_s"] / res["copy_bytes_per_s"]
                    print(json.dumps(row), flush=True)
                    res["rows"].append(row)
                del x, g
                torch.cuda.empty_cache()
    if not a.no_network and (not a.only or a.only == "brats"):
        torch.manual_seed(0)
        plain = ft.Deconver(in_channels=4, out_channels=3, spatial_dims=3, norm=nn.InstanceNorm3d, act=nn.ReLU, groups=-1, ratio=1,
                            kernel_size=(3, 3, 3), num_iters=1, mlp_ratio=4).to(dev)
        conv = ft.convert_instance_norm(copy.deepcopy(plain))
        x = torch.rand(2, 4, 128, 128, 128, device=dev)
        gy = torch.rand(2, 3, 128, 128, 128, device=dev)

        def step(m):
            return torch.autograd.grad(m(x), list(m.parameters()), gy, allow_unused=True)

        variants = {"native": lambda: step(conv), "framework": lambda: step(plain), "native_again": lambda: step(conv)}
        times, iters = alternate(variants, max(3, a.rounds // 2), a.window_ms)
        ms = summary(times)
        res["network"] = {"model": "Deconver 4 -> 3, widths 32..512, depthwise k3, num_iters 1, 2 x 128^3, fp32, forward + backward",
                          "calls_per_round": iters, "ms_per_step": ms,
                          "native_over_framework": ms["native"]["median"] / ms["framework"]["median"]}
        print(json.dumps(res["network"]), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
