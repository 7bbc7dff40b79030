"""Inputs and CPU references shared by tests/test_wide_nmf_bf16_cpu.py and tests/test_gpu_wide_nmf_bf16.py: the two
split-N NMF families (csrc/nmf_global.hip, csrc/nmf_global_rank.hip) on bf16 activation storage.

The inputs of the bf16 path are the fp32 inputs of tests/wide_rank_cases.py rounded to bf16 (`rb`), so the bf16 tensors
hold them exactly; every reference is computed from those same values.  As there, a (case, solver) pair is usable only if
the fp32 oracle is within W.GUARD of the float64 oracle on THESE inputs (`guard`: asserted, never skipped).  References
are computed once per process and handed out read-only."""
import functools

import torch

import parity as P
import wide_rank_cases as W
from oracle import cpu_ref as O

BF = torch.bfloat16
U = 2.0 ** -8   # bf16 unit roundoff (8 significand bits, RNE)


def rb(t):
    """round to bf16 and come back: the value a bf16 tensor in HBM actually holds"""
    return t.to(BF).float()


def close(what, got, ref, n_stores, extra=0.0):
    """max|got − ref| ≤ n_stores · u · max|ref| (+ extra)"""
    assert got.dtype in (BF, torch.float32)
    return P.close(what, got.float(), ref, rel=n_stores * U, floor=1e-6, extra=extra,
                   why=f"bf16 storage: {n_stores} stored tensor(s) x u = 2^-8 between input and this result")


def bits(t):
    """a bf16 tensor as integers (non-finite values compare too)"""
    assert t.dtype == BF
    return t.detach().contiguous().view(torch.int16).cpu()


@functools.lru_cache(maxsize=None)
def inputs(M, N, R):
    """(x, u0, v0, gy) of W.inputs with x and gy rounded to bf16 (fp32 tensors holding bf16 values); never modified"""
    x, u0, v0, gy = W.inputs(M, N, R)
    return rb(x), u0, v0, rb(gy)


@functools.lru_cache(maxsize=None)
def reference(M, N, R, T, G, solver):
    """as W.reference, on the rounded inputs"""
    x, u0, v0, gy = inputs(M, N, R)
    d = lambda t: t.double()
    y32 = O.nmf_forward(x, u0, v0, T, solver, G)
    gx32 = O.nmf_backward(x, u0, v0, gy, T, solver, G)
    y64 = O.nmf_forward(d(x), d(u0), d(v0), T, solver, G)
    gx64 = O.nmf_backward(d(x), d(u0), d(v0), d(gy), T, solver, G)
    yk = (y32.double() - y64).abs().max().item()
    gk = (gx32.double() - gx64).abs().max().item()
    return {"y64": y64.float(), "gx64": gx64.float(), "y_kink": yk, "gx_kink": gk,
            "y_guard": yk / y64.abs().max().item(), "gx_guard": gk / gx64.abs().max().item()}


def guard(M, N, R, T, G, solver):
    """the conditioning guard of one (case, solver) pair on the rounded inputs: a property of the inputs"""
    ref = reference(M, N, R, T, G, solver)
    print(f"guard (bf16 inputs) {M}x{N} R{R} T{T} G{G} {solver}: y {ref['y_guard']:.2e} gx {ref['gx_guard']:.2e}")
    assert ref["y_guard"] <= W.GUARD and ref["gx_guard"] <= W.GUARD, (M, N, R, T, G, solver, ref["y_guard"], ref["gx_guard"])
    return ref
