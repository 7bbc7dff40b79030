"""Device time of ft.prepare_volume and ft.restore_prediction at the recipe's shape (profiles/vol_prep.md): a
(4, 240, 240, 155) volume, int16 and fp32, roi 128^3, class-map label with the BraTS sets; restore with K = 5 fold models.
The native kernels against (a) the same chain in framework ops on the same device — the composed path of
factorizer_amd/volume.py, what a user would write today — and (b) the algorithmic bytes of each pass over the copy rate.
Whole calls: HIP events around them after warm-up (prepare_volume includes its one host read of the box); single passes: the
library's KernelTimer.  A run without a GPU fails.

    python tools/bench_vol_prep.py [--reps 30] [--out vol_prep_bench.json]
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import factorizer_amd as ft  # noqa: E402
from factorizer_amd import _native as N  # noqa: E402
from factorizer_amd import functional as Fn  # noqa: E402
from factorizer_amd import volume as V  # noqa: E402

SHAPE = (4, 240, 240, 155)
HEAD = ((28, 204), (22, 218), (6, 146))   # the non-zero part of a skull-stripped BraTS volume, roughly
ROI = (128, 128, 128)
MARGIN = 10
FOLDS = 5
COPY_TBPS = 5.65                           # bare 16-byte-per-lane 1 : 1 stream on this chip (5.4-5.9 TB/s)


def synthetic(dtype, dev):
    g = torch.Generator().manual_seed(0)
    x = torch.zeros(SHAPE, dtype=torch.float32)
    inner = (slice(None),) + tuple(slice(a, b) for a, b in HEAD)
    x[inner] = torch.randn(x[inner].shape, generator=g).abs() * 300 + 20
    lab = torch.zeros(SHAPE[1:], dtype=torch.uint8)
    lab[tuple(slice(a + 40, b - 60) for a, b in HEAD)] = torch.randint(0, 4, [b - a - 100 for a, b in HEAD], generator=g,
                                                                      dtype=torch.uint8)
    x = x.round().to(torch.int16) if dtype == torch.int16 else x / 7
    return x.to(dev), lab.to(dev)


def framework_prepare(x, lab):
    """the composed chain on device, box included"""
    size = tuple(x.shape[1:])
    fl = V._first_last_composed(x)
    start = tuple(max(f - MARGIN, 0) for f in fl[0])
    end = tuple(min(l + 1 + MARGIN, n) for l, n in zip(fl[1], size))
    bsize = tuple(e - s for s, e in zip(start, end))
    out = tuple(max(b, r) for b, r in zip(bsize, ROI))
    before = tuple((o - b) // 2 for o, b in zip(out, bsize))
    return V._prepare_composed(x, lab, start, end, before, out, True, True, ft.BRATS_CLASSES, torch.float32)


def time_ms(fn, reps):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(reps):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / reps


def kernel_table(fn, reps):
    """per pass: launches per call, average ms per call, algorithmic bytes per call, through the library's timer"""
    timer = Fn.KernelTimer()
    Fn.set_timer(timer)
    n0 = N.launch_count()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    launches = (N.launch_count() - n0) / reps
    Fn.set_timer(None)
    out = {}
    for name, a in timer.summary().items():
        ms, nb = a["ms"] / reps, a["bytes"] / reps
        out[name] = {"ms": ms, "bytes": nb, "GBps": nb / ms / 1e6, "floor_ms": nb / (COPY_TBPS * 1e9),
                     "fraction_of_copy_rate": nb / ms / 1e6 / (COPY_TBPS * 1e3)}
    return launches, out


def framework_launches(fn):
    """device kernels of one call of the framework path, counted by the framework's profiler; None if it is unavailable"""
    try:
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        return sum(1 for ev in prof.events() if str(ev.device_type).endswith("CUDA"))
    except Exception as exc:  # noqa: BLE001
        print("framework launch count not available:", exc, flush=True)
        return None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_vol_prep.py measures device time: no GPU found")
    dev = torch.device("cuda:0")
    res = {"device": torch.cuda.get_device_name(0), "shape": list(SHAPE), "roi": list(ROI), "reps": a.reps,
           "copy_rate_TBps": COPY_TBPS, "cases": {}}

    def save():
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as f:
                json.dump(res, f, indent=1)

    for dtype in (torch.int16, torch.float32):
        x, lab = synthetic(dtype, dev)
        nat = lambda: ft.prepare_volume(x, lab, margin=MARGIN, roi_size=ROI, classes=ft.BRATS_CLASSES)   # noqa: E731
        fw = lambda: framework_prepare(x, lab)                                                            # noqa: E731
        p = nat()
        q = fw()
        same = bool(torch.equal(p.image[0], q[0]) and torch.equal(p.label[0], q[1]))
        case = {"box": [list(p.box_start), list(p.box_end)], "prepared": list(p.image.shape), "equal_to_framework_path": same}
        # alternate the two paths: other work shares the host
        nat_ms, fw_ms = [], []
        for _ in range(3):
            nat_ms.append(time_ms(nat, a.reps))
            fw_ms.append(time_ms(fw, max(3, a.reps // 3)))
        launches, passes = kernel_table(nat, a.reps)
        floor = sum(v["floor_ms"] for v in passes.values())
        case.update({"native_ms": nat_ms, "framework_ms": fw_ms, "ratio_framework_over_native": min(fw_ms) / min(nat_ms),
                     "native_launches": launches, "passes": passes, "kernel_ms": sum(v["ms"] for v in passes.values()),
                     "floor_ms": floor, "ratio_native_over_floor": min(nat_ms) / floor})
        res["cases"]["prepare_" + str(dtype).split(".")[-1]] = case
        print("prepare", dtype, json.dumps(case), flush=True)
        save()
    # restore: K = 5 logit tensors of the prepared shape
    g = torch.Generator().manual_seed(1)
    for dtype in (torch.float32, torch.bfloat16):
        ls = [torch.randn((1, 3) + tuple(p.image.shape[2:]), generator=g).to(dtype).to(dev) for _ in range(FOLDS)]
        geo = (p.box_start, p.box_end, p.pad_before, p.orig_size)
        bound = V._bound(True, 0.5)
        for form, vals in (("label_map", ft.BRATS_LABEL_VALUES), ("mask", None)):
            nat = lambda: ft.restore_prediction(ls, p, label_values=vals)                                  # noqa: E731
            fw = lambda: V._restore_composed(ls, *geo, bound, vals)                                        # noqa: E731
            same = bool(torch.equal(nat(), fw()))
            nat_ms, fw_ms = [], []
            for _ in range(3):
                nat_ms.append(time_ms(nat, a.reps))
                fw_ms.append(time_ms(fw, max(3, a.reps // 3)))
            launches, passes = kernel_table(nat, a.reps)
            floor = sum(v["floor_ms"] for v in passes.values())
            case = {"equal_to_framework_path": same, "native_ms": nat_ms, "framework_ms": fw_ms,
                    "ratio_framework_over_native": min(fw_ms) / min(nat_ms), "native_launches": launches, "passes": passes,
                    "floor_ms": floor, "ratio_native_over_floor": min(nat_ms) / floor}
            res["cases"][f"restore_{form}_" + str(dtype).split(".")[-1]] = case
            print("restore", form, dtype, json.dumps(case), flush=True)
            save()
    x, lab = synthetic(torch.int16, dev)
    res["framework_launches_prepare"] = framework_launches(lambda: framework_prepare(x, lab))
    res["framework_launches_restore_label_map"] = framework_launches(
        lambda: V._restore_composed(ls, *geo, bound, ft.BRATS_LABEL_VALUES))
    save()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
