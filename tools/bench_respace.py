"""Device time of ft.resample_volume and ft.restore_spaced_prediction at an ISLES-like shape (profiles/respace.md): a
(2, 112, 112, 73) volume with a one-channel uint8 label, at 2 x 2 x 2 mm (pixdim 2: the copy path) and at 0.9 x 0.9 x 6 mm
brought to pixdim 2; restore with K = 5 one-channel logit tensors.  The native kernels against (a) the same chain in framework
ops on the same device — the composed path of factorizer_amd/respace.py fed device tensors — and (b) the device copy rate,
measured here on a buffer of the call's algorithmic bytes.  Also the gather with the axes in place against the same size with
the axes permuted, which decides whether a tile-staging variant is worth having.  Every repetition is timed on its own with
HIP events after warm-up (ten calls between two events, so that the host side of a call hides behind the device work of
the one before); medians with the 10th / 90th percentile.  A run without a GPU fails.

    python tools/bench_respace.py [--reps 50] [--out respace_bench.json]
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import factorizer_amd as ft  # noqa: E402
from factorizer_amd import respace as RS  # noqa: E402

SIZE = (112, 112, 73)
C, FOLDS = 2, 5
WORLD = {"L": (0, -1), "R": (0, 1), "P": (1, -1), "A": (1, 1), "I": (2, -1), "S": (2, 1)}


def affine(code, zooms):
    A = np.eye(4)
    A[:3, :3] = 0.0
    for i, c in enumerate(code):
        w, s = WORLD[c]
        A[w, i] = s * zooms[i]
    return A


INNER = 10   # calls between two events: the host side of a call (about 20 us) hides behind the device work of the one before


def times_us(fn, reps):
    for _ in range(5):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(INNER):
            fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b) * 1e3 / INNER)
    q = np.percentile(out, [50, 10, 90])
    return dict(median_us=round(float(q[0]), 2), p10_us=round(float(q[1]), 2), p90_us=round(float(q[2]), 2))


def copy_us(nbytes, reps, dev):
    src = torch.empty(nbytes // 8, dtype=torch.float32, device=dev).normal_()
    dst = torch.empty_like(src)
    return times_us(lambda: dst.copy_(src), reps)


def with_rates(rec, nbytes, reps, dev):
    rec["algorithmic_MB"] = round(nbytes / 1e6, 3)
    rec["copy_same_bytes"] = copy_us(nbytes, reps, dev)
    rec["fraction_of_copy_rate"] = round(rec["copy_same_bytes"]["median_us"] / rec["native"]["median_us"], 3)
    rec["speedup_over_framework"] = round(rec["framework"]["median_us"] / rec["native"]["median_us"], 2)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = "cuda:0"
    gen = torch.Generator().manual_seed(0)
    x = torch.randn((C,) + SIZE, generator=gen).to(dev)
    lab = (torch.rand((1,) + SIZE, generator=gen) > 0.9).to(torch.uint8).to(dev)
    res = {"size": [C, *SIZE], "folds": FOLDS, "reps": a.reps, "device": torch.cuda.get_device_name(0)}
    for name, zooms in (("2x2x2_to_2", (2.0, 2.0, 2.0)), ("0.9x0.9x6_to_2", (0.9, 0.9, 6.0))):
        g = ft.spacing_geometry(SIZE, affine("LPS", zooms), 2.0, roi_size=(64, 64, 64))
        nearest = all(abs(s) == 1.0 for s in g.scale)
        out_vox = int(np.prod(g.out_size))
        fwd = dict(res_size=list(g.res_size), out_size=list(g.out_size))
        fwd["native"] = times_us(lambda: ft.resample_volume(x, g, label=lab), a.reps)
        fwd["framework"] = times_us(lambda: (RS._pad(RS._resample_composed(x, g, nearest), g.pad_before, g.out_size),
                                             RS._pad(RS._resample_composed(lab, g, True), g.pad_before, g.out_size)), a.reps)
        with_rates(fwd, (C * 4 + 1) * (x[0].numel() + out_vox), a.reps, dev)
        ls = [torch.randn((1, 1) + g.out_size, generator=gen).mul_(4).to(dev) for _ in range(FOLDS)]
        for dtype in (torch.float32, torch.bfloat16):
            lt = [t.to(dtype) for t in ls]
            inv = {}
            inv["native"] = times_us(lambda: ft.restore_spaced_prediction(lt, g), a.reps)
            inv["framework"] = times_us(lambda: RS._unspace_composed(lt, g, True, 0.5), a.reps)
            with_rates(inv, FOLDS * int(np.prod(g.res_size)) * lt[0].element_size() + x[0].numel(), a.reps, dev)
            fwd["restore_" + str(dtype).split(".")[1]] = inv
        res[name] = fwd
    # the gather with the axes in place, mirrored, and permuted, on one size and scale (image only, bilinear); large enough
    # that the kernel, not the call, is what is timed
    cube = torch.randn((2, 256, 256, 256), generator=gen).to(dev)
    perm = {}
    for code in ("RAS", "LPI", "ARS", "SAR", "ASR"):
        g = ft.spacing_geometry((256, 256, 256), affine(code, (1.5, 1.5, 1.5)), 2.0)
        r = times_us(lambda: ft.resample_volume(cube, g), a.reps)
        r["src_axis"], r["res_size"] = list(g.src_axis), list(g.res_size)
        r["GB_per_s"] = round((cube.numel() + 2 * int(np.prod(g.out_size))) * 4 / r["median_us"] / 1e3, 1)
        perm[code] = r
    res["axes_256cubed_1.5_to_2"] = perm
    text = json.dumps(res, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
