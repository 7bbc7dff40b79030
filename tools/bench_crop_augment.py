"""Device time per batch of ft.crop_augment_batch (profiles/crop_augment.md): the crop cut inside the augmentation gather
against the two ways there were to feed ft.augment_batch from prepared volumes before it existed —
  (a) device slices of the resident sources + torch.stack + ft.augment_batch,
  (b) host slices into a pinned buffer + one host-to-device copy + ft.augment_batch
— on the recipe's geometries: BraTS B = 2, 4 x fp32 + 3 x uint8, roi 128^3 from 155 x 240 x 240 sources and a ragged smaller
one; FIVES B = 16, 3 x fp32 + 1 x uint8, roi 512^2 from 2048^2 sources.  Each with identity records (a pure batched crop) and
with the recipe's probabilities over --batches drawn batches (sources, origins and records from a seeded generator).

How the time is taken.  One process, every shape warmed up.  A WINDOW is --window consecutive batches between two HIP events.
The host needs longer to issue a batch than the device to run it, so a window is queued behind a blocker (matrix products that
keep the device busy until the whole window is enqueued; `queued` in the result says whether that held, and only such windows
count): the events then bracket device work alone.  The paths alternate window by window over the same batches — (a), fused,
(b), (a) again — and the spread is the difference of the two (a) windows of a round.  Path (b)'s host slicing runs before its
window and is reported separately as host wall time; its window holds the pinned copy and the augmentation.  The free-running
time per batch of a plain loop (host-bound where the host is slower) is reported beside it.  The resample launches alone come
from the library's KernelTimer.  A run without a GPU fails.

    python tools/bench_crop_augment.py [--batches 200] [--window 8] [--out crop_augment_bench.json]
"""
from __future__ import annotations

import argparse
import json
import math
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import factorizer_amd as ft  # noqa: E402
from factorizer_amd import _native  # noqa: E402
from factorizer_amd import augment as AG  # noqa: E402
from factorizer_amd import functional as Fn  # noqa: E402

GEOMS = {
    "brats": dict(B=2, C=4, L=3, roi=(128, 128, 128), sources=[(155, 240, 240)] * 3 + [(141, 173, 190)]),
    "fives": dict(B=16, C=3, L=1, roi=(512, 512), sources=[(2048, 2048)] * 8),
}
HOST_ROUNDS = 8          # path (b) is timed in the first rounds only: its host slicing takes tens of ms per batch


def box(t, g, roi):
    return t[(slice(None),) + tuple(slice(o, o + r) for o, r in zip(g, roi))]


class Batch:
    def __init__(self, idx, org, params):
        self.idx, self.org, self.params = idx, org, params


def draw_batches(n, geom, recipe, gen, dev):
    """n batches: source indices, origins and records from `gen`; the noise seed is put on the device here (a Python int would
    be uploaded by a synchronous copy inside every call that adds noise)"""
    nd = len(geom["roi"])
    out = []
    for _ in range(n):
        idx = torch.randint(0, len(geom["sources"]), (geom["B"],), generator=gen).tolist()
        org = ft.draw_crop_origins([geom["sources"][i] for i in idx], geom["roi"], gen)
        params = ft.draw_augment_params(geom["B"], nd, generator=gen) if recipe else ft.AugmentParams.identity(geom["B"], nd)
        params.seed = torch.tensor([params.seed], dtype=torch.int64, device=dev)
        out.append(Batch(idx, org.tolist(), params))
    return out


class Blocker:
    """keeps the device busy for about `ms` milliseconds"""

    def __init__(self, dev):
        self.a = torch.rand(4096, 4096, device=dev)
        for _ in range(3):
            self.a @ self.a
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        s.record()
        for _ in range(10):
            self.a @ self.a
        e.record()
        torch.cuda.synchronize()
        self.one_ms = s.elapsed_time(e) / 10

    def run(self, ms):
        for _ in range(max(1, int(math.ceil(ms / self.one_ms)))):
            self.a @ self.a


def window_ms(fn, batches, blocker, block_ms):
    """(device ms per batch, queued?) of fn over `batches`, the window queued behind the blocker"""
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    blocker.run(block_ms)
    s.record()
    for k, bt in enumerate(batches):
        fn(bt, k)
    e.record()
    queued = not s.query()              # the blocker was still running when the last batch had been issued
    torch.cuda.synchronize()
    return s.elapsed_time(e) / len(batches), queued


def free_running_ms(fn, batches):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for k, bt in enumerate(batches):
        fn(bt, 0)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / len(batches)


def device():
    if not torch.cuda.is_available():
        raise SystemExit("bench_crop_augment.py measures device time: no GPU found")
    return torch.device("cuda:0")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, default=200)
    ap.add_argument("--window", type=int, default=8)
    ap.add_argument("--only", default=None, help="one geometry")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = device()
    blocker = Blocker(dev)
    res = {"device": torch.cuda.get_device_name(0) if dev.type == "cuda" else "none", "batches": a.batches, "window": a.window,
           "blocker_ms": blocker.one_ms, "cases": {}}
    for name, geom in GEOMS.items():
        if a.only and name != a.only:
            continue
        B, C, L, roi = geom["B"], geom["C"], geom["L"], geom["roi"]
        nd, V = len(roi), math.prod(roi)
        gen = torch.Generator().manual_seed(7)
        hx = [torch.rand((C,) + s, generator=gen) for s in geom["sources"]]
        hl = [torch.randint(0, 4, (L,) + s, generator=gen, dtype=torch.uint8) for s in geom["sources"]]
        xs, ls = [t.to(dev) for t in hx], [t.to(dev) for t in hl]
        W = a.window
        pin_x = [torch.empty((B, C) + roi, pin_memory=dev.type == "cuda") for _ in range(W)]
        pin_l = [torch.empty((B, L) + roi, dtype=torch.uint8, pin_memory=dev.type == "cuda") for _ in range(W)]
        batch_bytes = B * V * (4 * C + L)                    # one batch of image + label
        case = {"B": B, "C": C, "L": L, "roi": list(roi), "sources": [list(s) for s in geom["sources"]],
                "batch_bytes": batch_bytes, "resident_source_bytes": sum(t.numel() * 4 for t in hx) + sum(t.numel() for t in hl)}

        def fused(bt, k):
            return ft.crop_augment_batch([xs[i] for i in bt.idx], [ls[i] for i in bt.idx], bt.org, roi, bt.params)

        def device_slices(bt, k):
            x = torch.stack([box(xs[i], g, roi) for i, g in zip(bt.idx, bt.org)])
            l = torch.stack([box(ls[i], g, roi) for i, g in zip(bt.idx, bt.org)])
            return ft.augment_batch(x, l, bt.params)

        def host_stage(bt, k):
            for b, (i, g) in enumerate(zip(bt.idx, bt.org)):
                pin_x[k][b].copy_(box(hx[i], g, roi))
                pin_l[k][b].copy_(box(hl[i], g, roi))

        def host_copy(bt, k):
            return ft.augment_batch(pin_x[k].to(dev, non_blocking=True), pin_l[k].to(dev, non_blocking=True), bt.params)

        for key, recipe in (("identity", False), ("recipe", True)):
            batches = draw_batches(a.batches, geom, recipe, torch.Generator().manual_seed(11), dev)
            # the three paths give the same bits at the sizes timed
            bt = batches[0]
            host_stage(bt, 0)
            ref = device_slices(bt, 0)
            for other in (fused(bt, 0), host_copy(bt, 0)):
                assert torch.equal(ref[0], other[0]) and torch.equal(ref[1], other[1])
            n0 = _native.launch_count()
            for bt in batches:
                fused(bt, 0)
            launches = (_native.launch_count() - n0) / len(batches)
            # how long the host needs to issue a window, per path (warm-up of every shape as well): sizes the blocker
            issue = {}
            for pname, fn in (("device_slices", device_slices), ("fused", fused), ("host_copy", host_copy)):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for k, bt in enumerate(batches[:W]):
                    fn(bt, k)
                issue[pname] = (time.perf_counter() - t0) * 1e3
                torch.cuda.synchronize()
            block_ms = 2.0 * max(issue.values()) + 5.0
            t = {"device_slices": [], "device_slices_again": [], "fused": [], "host_copy": []}
            not_queued, stage_ms = 0, []
            for r in range(len(batches) // W):
                win = batches[r * W:(r + 1) * W]
                order = [("device_slices", device_slices), ("fused", fused)]
                if r < HOST_ROUNDS:
                    t0 = time.perf_counter()
                    for k, bt in enumerate(win):
                        host_stage(bt, k)
                    stage_ms.append((time.perf_counter() - t0) * 1e3 / W)
                    order.append(("host_copy", host_copy))
                order.append(("device_slices_again", device_slices))
                for pname, fn in order:
                    ms, queued = window_ms(fn, win, blocker, block_ms)
                    if queued:
                        t[pname].append((r, ms))
                    else:
                        not_queued += 1
            mean = {p: statistics.fmean(ms for _, ms in v) if v else None for p, v in t.items()}
            again = dict(t["device_slices_again"])
            rel = [abs(ms - again[r]) / ms for r, ms in t["device_slices"] if r in again]
            both = dict(t["fused"])
            gain = [ms / both[r] for r, ms in t["device_slices"] if r in both]
            ns = sum(int((bt.params.sigma > 0).any(1).sum()) for bt in batches) / len(batches)
            smooth_bytes = ns * C * V * 8                       # fp32 workspace written and read instead of the direct store
            case[key] = {
                "device_ms_per_batch": mean, "windows_counted": {p: len(v) for p, v in t.items()}, "windows_not_queued": not_queued,
                "baseline_repeat_rel_diff_median": statistics.median(rel) if rel else None,
                "baseline_repeat_rel_diff_max": max(rel) if rel else None,
                "device_slices_over_fused_per_window_median": statistics.median(gain) if gain else None,
                "device_slices_over_fused_per_window_min": min(gain) if gain else None,
                "host_slicing_wall_ms_per_batch": statistics.fmean(stage_ms) if stage_ms else None,
                "host_issue_ms_per_window": issue,
                "free_running_ms_per_batch": {"device_slices": free_running_ms(device_slices, batches[:40]),
                                              "fused": free_running_ms(fused, batches[:40])},
                "native_launches_per_batch_fused": launches, "smoothing_samples_per_batch": ns,
                "bytes_from_shapes": {"fused": 2 * batch_bytes + smooth_bytes,
                                      "device_slices_at_least": 4 * batch_bytes + smooth_bytes,
                                      "host_copy_over_pcie": batch_bytes},
            }
            print(name, key, json.dumps(case[key]), flush=True)
        # the resample launches alone on identity batches: the crop gather against the dense gather at the same output
        batches = draw_batches(24, geom, False, torch.Generator().manual_seed(13), dev)
        table = AG._crop_table([xs[i] for i in batches[0].idx], [ls[i] for i in batches[0].idx], batches[0].org, roi)
        case["first_batch_vector_source_loads"] = AG.source_vector_loads(table, roi, 4).tolist()
        timer = Fn.KernelTimer(only=("aug_crop_resample", "aug_resample"))
        Fn.set_timer(timer)
        for bt in batches:
            fused(bt, 0)
            device_slices(bt, 0)
        Fn.set_timer(None)
        agg = timer.summary()
        for k in ("aug_crop_resample", "aug_resample"):
            ms = agg[k]["ms"] / agg[k]["calls"]
            case[k + "_launch_ms"] = ms
            case[k + "_GBps"] = 2 * batch_bytes / ms / 1e6
        print(name, "launches alone", case["aug_crop_resample_launch_ms"], case["aug_resample_launch_ms"], flush=True)
        res["cases"][name] = case
        del xs, ls, hx, hl, pin_x, pin_l
        torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
