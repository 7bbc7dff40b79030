"""Device time of ft.augment_batch per batch (profiles/augment.md): the native kernels against the framework path
(affine_grid / grid_sample, conv, elementwise ops) on the recipe's shapes — BraTS B = 2, 4 x 128^3 image + 3 x 128^3 uint8
label; FIVES B = 16, 3 x 512^2 + 1 x 512^2 — with every step drawn on every sample, with nothing drawn (pure streaming), and
with the recipe's probabilities averaged over 200 drawn batches.  Times are HIP events around the calls of one batch, after
warm-up; a run without a GPU fails.

    python tools/bench_augment.py [--batches 200] [--out augment_bench.json]
"""
from __future__ import annotations

import argparse
import json
import math
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import factorizer_amd as ft  # noqa: E402
from factorizer_amd import augment as AG  # noqa: E402

SHAPES = {"brats": ((2, 4, 128, 128, 128), 3), "fives": ((16, 3, 512, 512), 1)}


def framework_path(image, label, p):
    """the same six transforms with framework ops on device (linear interpolation through grid_sample, so a comparison of
    cost, not of bits): one affine_grid + two grid_sample, randn noise, one grouped conv per axis, elementwise intensity"""
    B, nd = image.shape[0], image.dim() - 2
    dev = image.device
    sp = image.shape[2:]
    theta = torch.zeros(B, nd, nd + 1)
    for b in range(B):                     # voxel-space A (z, y, x) -> normalised (x, y, z) coordinates of affine_grid
        A = p.affine[b].double()
        n = torch.tensor([s - 1 for s in sp], dtype=torch.float64)
        M = (A * n[None, :] / n[:, None]).flip(0, 1)
        sign = torch.where(p.flip[b].flip(0), -1.0, 1.0).double()
        theta[b, :, :nd] = (M * sign[None, :]).float()
    grid = F.affine_grid(theta.to(dev), image.shape, align_corners=True)
    x = F.grid_sample(image, grid, mode="bilinear", padding_mode="border", align_corners=True)
    lab = F.grid_sample(label.float(), grid, mode="nearest", padding_mode="border", align_corners=True).to(label.dtype)
    std = p.noise_std.to(dev).reshape(B, *([1] * (nd + 1)))
    x = x + std * torch.randn_like(x)
    conv = F.conv3d if nd == 3 else F.conv2d
    for b in range(B):
        if not bool((p.sigma[b] > 0).any()):
            continue
        xb = x[b:b + 1].transpose(0, 1)    # channels as batch: one filter
        for k in range(nd):
            s = float(p.sigma[b, k])
            if s <= 0:
                continue
            w = AG.gaussian_taps(s).to(dev)
            shape = [1, 1] + [1] * nd
            shape[2 + k] = w.numel()
            pad = [0] * nd
            pad[k] = (w.numel() - 1) // 2
            xb = conv(xb, w.reshape(shape), padding=pad)
        x[b] = xb.transpose(0, 1)[0]
    g = p.gain.to(dev).reshape(B, *([1] * (nd + 1)))
    o = p.offset.to(dev).reshape(B, *([1] * (nd + 1)))
    return x * g + o, lab


def all_drawn(B, nd):
    g = torch.Generator().manual_seed(1)
    return ft.draw_augment_params(B, nd, generator=g, affine_prob=1, noise_prob=1, smooth_prob=1, scale_intensity_prob=1,
                                  shift_intensity_prob=1)


def time_ms(fn, reps):
    for _ in range(3):
        fn(0)
    torch.cuda.synchronize()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for i in range(reps):
        fn(i)
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, default=200)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_augment.py measures device time: no GPU found")
    dev = torch.device("cuda:0")
    res = {"device": torch.cuda.get_device_name(0), "batches": a.batches, "cases": {}}
    for name, (shape, L) in SHAPES.items():
        B, C, nd = shape[0], shape[1], len(shape) - 2
        V = math.prod(shape[2:])
        img = torch.rand(shape, device=dev)
        lab = torch.randint(0, 4, (B, L, *shape[2:]), device=dev, dtype=torch.uint8)
        stream_bytes = B * V * (2 * 4 * C + 2 * L)          # every voxel read once and written once
        g = torch.Generator().manual_seed(2)
        drawn = [ft.draw_augment_params(B, nd, generator=g) for _ in range(a.batches)]
        sets = {"identity": [ft.AugmentParams.identity(B, nd)], "all_steps": [all_drawn(B, nd)], "recipe": drawn}
        case = {"shape": list(shape), "label_channels": L, "stream_bytes": stream_bytes}
        for key, ps in sets.items():
            reps = len(ps) if key == "recipe" else 50
            nat = time_ms(lambda i: ft.augment_batch(img, lab, ps[i % len(ps)]), reps)
            fw = time_ms(lambda i: framework_path(img, lab, ps[i % len(ps)]), min(reps, 50))
            ns = sum(int((p.sigma > 0).any(1).sum()) for p in ps) / len(ps)
            nbytes = stream_bytes + ns * C * V * (4 + 4 + 4)   # smoothing samples: fp32 workspace written, read, final store
            nbytes -= ns * C * V * 4                            # ... instead of the direct store
            case[key] = {"native_ms": nat, "framework_ms": fw, "ratio": fw / nat, "bytes": nbytes,
                         "native_GBps": nbytes / nat / 1e6, "smoothing_samples_per_batch": ns}
            print(name, key, json.dumps(case[key]), flush=True)
        # the resample launch alone on the all-identity batch (kernel time through the library's timer)
        from factorizer_amd import functional as Fn
        timer = Fn.KernelTimer()
        Fn.set_timer(timer)
        for _ in range(20):
            ft.augment_batch(img, lab, sets["identity"][0])
        Fn.set_timer(None)
        agg = timer.summary()["aug_resample"]
        case["identity_resample_launch_ms"] = agg["ms"] / agg["calls"]
        case["identity_resample_GBps"] = stream_bytes / (agg["ms"] / agg["calls"]) / 1e6
        print(name, "identity resample launch", case["identity_resample_launch_ms"], "ms", case["identity_resample_GBps"], "GB/s",
              flush=True)
        res["cases"][name] = case
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
