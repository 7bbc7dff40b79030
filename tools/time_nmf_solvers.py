"""Device time of the native cd / smu solvers against native hals / mu and against the composed path (HIP events after warm-up).

  python tools/time_nmf_solvers.py [--out FILE.json]

Workloads: 32 768 matrices of 8 x 512, rank 2, 5 iterations (BASELINE configs[1]'s matrix count), forward and forward + backward;
a FactorizerBlock at C = 32 on a 64^3 volume (patch 8: the 8^3 fused core), forward and forward + backward.  The composed path is
the same module with the solver's native id hidden (the package's ATen update rules on device).  Timings are reported, never gated.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import warnings

import torch
from torch import nn

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import factorizer_amd as ft  # noqa: E402

DEV = "cuda:0"


def _composed(module):
    """hide the native id of every solver inside `module`: the composed path runs instead"""
    for m in module.modules():
        if isinstance(m, ft.MatrixFactorization):
            s = m.solver
            s.__class__ = type("Composed" + type(s).__name__, (type(s),), {"native_id": None})
    return module


def _time(fn, warmup=3, iters=10):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(iters):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / iters


def nmf_case(solver, native, bwd):
    torch.manual_seed(0)
    mf = ft.MatrixFactorization((8, 512), rank=2, num_iters=5, init="uniform", solver=solver).to(DEV)
    if not native:
        _composed(mf)
    x = torch.rand(32768, 8, 512, device=DEV, requires_grad=bwd)
    gy = torch.rand_like(x)

    def run():
        y = mf(x)
        if bwd:
            torch.autograd.grad(y, x, gy)
    return _time(run, iters=5 if native else 2)


def block_case(solver, native, bwd):
    torch.manual_seed(0)
    blk = ft.FactorizerBlock(channels=32, spatial_size=(64, 64, 64), norm=ft.LayerNorm,
                             reshape=(ft.SWMatricize, {"head_dim": 8, "patch_size": 8}), act=nn.ReLU, factorize=ft.NMF,
                             rank=1, num_iters=5, init="uniform", solver=solver, mlp_ratio=2, dropout=0.0).to(DEV)
    if not native:
        _composed(blk)
    x = torch.randn(1, 32, 64, 64, 64, device=DEV, requires_grad=bwd)
    gy = torch.rand_like(x)

    def run():
        y = blk(x)
        if bwd:
            torch.autograd.grad(y, [x] + list(blk.parameters()), gy)
    return _time(run, iters=5 if native else 2)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    warnings.simplefilter("ignore", RuntimeWarning)   # the composed rows warn that they are composed
    res = {}
    for wl, fn in (("nmf_32768x8x512_r2_t5", nmf_case), ("block_c32_64cubed_r1_t5", block_case)):
        for bwd in (False, True):
            for solver in ("hals", "cd", "mu", "smu"):
                for native in (True, False):
                    key = f"{wl}:{'fwd+bwd' if bwd else 'fwd'}:{solver}:{'native' if native else 'composed'}"
                    res[key] = round(fn(solver, native, bwd), 4)
                    print(f"{key}: {res[key]:.4f} ms", flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump({"device": torch.cuda.get_device_name(0), "ms": res}, f, indent=1)


if __name__ == "__main__":
    main()
