"""Device time of the U-shape convolutions of the FIVES 2-D Deconver (widths 32..512, strides (1, 2, 2, 2, 2), 512^2 RGB):
native (convs.Conv2d / convs.ConvTranspose2d on the 2-D tap geometries of the GEMM family) against the framework path
(F.conv2d / F.conv_transpose2d on the same tensors), forward and forward + backward, HIP events, warm-up, median of --iters.

  python tools/time_conv2d.py [--batch 16] [--iters 20] [--out profiles/conv2d_unet.json]

Algorithmic bytes: fp32 tensors read / written once (forward: x, w, y; backward adds gy read twice, x once, gx written).
Roofs (MI355X_MICROARCH.md): HBM 6.29 TB/s measured, fp32 matrix 155 TFLOP/s measured; `roof_frac` = achieved / the binding one.
Timings are reported, never gated.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import warnings

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from factorizer_amd import convs  # noqa: E402

DEV = "cuda:0"
HBM, MFMA = 6.29e12, 155e12
WIDTHS = (32, 64, 128, 256, 512)


def layers(S=512):
    out = [("stem k3 3->32", "k3", 3, 32, S)]
    s = S
    for i in range(4):
        out.append((f"down{i} k2s2 {WIDTHS[i]}->{WIDTHS[i + 1]}", "k2s2", WIDTHS[i], WIDTHS[i + 1], s))
        s //= 2
    for i in range(4, 0, -1):
        out.append((f"up{4 - i} tk2s2 {WIDTHS[i]}->{WIDTHS[i - 1]}", "t2", WIDTHS[i], WIDTHS[i - 1], s))
        s *= 2
    out.append(("head k1 32->1", "k1", 32, 1, S))
    return out


def module(kind, cin, cout):
    if kind == "t2":
        return convs.ConvTranspose2d(cin, cout, kernel_size=2, stride=2)
    k, st, p = {"k3": (3, 1, 1), "k2s2": (2, 2, 0), "k1": (1, 1, 0)}[kind]
    return convs.Conv2d(cin, cout, kernel_size=k, stride=st, padding=p, bias=(kind != "k3"))


def framework(m, x):
    if isinstance(m, torch.nn.ConvTranspose2d):
        return F.conv_transpose2d(x, m.weight, m.bias, stride=2)
    return F.conv2d(x, m.weight, m.bias, stride=m.stride, padding=m.padding)


def median_ms(fn, warmup, iters):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(iters):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        fn()
        e.record()
        torch.cuda.synchronize()
        ts.append(s.elapsed_time(e))
    return statistics.median(ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default="profiles/conv2d_unet.json")
    a = ap.parse_args()
    warnings.simplefilter("error", RuntimeWarning)      # the native rows must be native
    B, rows = a.batch, []
    for name, kind, cin, cout, s in layers(a.size):
        torch.manual_seed(0)
        m = module(kind, cin, cout).to(DEV)
        x = torch.randn(B, cin, s, s, device=DEV, requires_grad=True)
        y = m(x)
        gy = torch.randn_like(y)
        params = [x] + list(m.parameters())
        K = {"k3": 9 * cin, "k2s2": 4 * cin, "t2": cin, "k1": cin}[kind]
        M = {"t2": 4 * cout}.get(kind, cout)
        flops = 2.0 * B * (x[0, 0].numel() if kind != "k2s2" else y[0, 0].numel()) * M * K
        fb = 4.0 * (x.numel() + y.numel() + sum(p.numel() for p in m.parameters()))
        bb = fb + 4.0 * (2 * y.numel() + 2 * x.numel())
        row = {"layer": name, "B": B, "in": list(x.shape), "out": list(y.shape), "gflop_fwd": flops / 1e9, "mb_fwd": fb / 1e6,
               "mb_fwd_bwd": bb / 1e6}
        for path, f in (("native", lambda: m(x)), ("framework", lambda: framework(m, x))):
            row[f"{path}_fwd_ms"] = median_ms(lambda: f(), a.warmup, a.iters)
            row[f"{path}_fwd_bwd_ms"] = median_ms(lambda: torch.autograd.grad(f(), params, gy), a.warmup, a.iters)
        for what, ms, byts, fl in (("fwd", row["native_fwd_ms"], fb, flops), ("fwd_bwd", row["native_fwd_bwd_ms"], bb, 3 * flops)):
            t_hbm, t_mfma = byts / HBM, fl / MFMA
            row[f"native_{what}_bound"] = "HBM" if t_hbm >= t_mfma else "MFMA"
            row[f"native_{what}_roof_frac"] = max(t_hbm, t_mfma) / (ms * 1e-3)
        row["speedup_fwd_bwd"] = row["framework_fwd_bwd_ms"] / row["native_fwd_bwd_ms"]
        rows.append(row)
        print(json.dumps(row), flush=True)
        del m, x, y, gy, params
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump({"device": torch.cuda.get_device_name(0), "batch": B, "size": a.size, "iters": a.iters, "rows": rows}, fh, indent=1)


if __name__ == "__main__":
    main()
