"""Inputs and CPU references shared by tests/test_wide_nmf_rank_cpu.py and tests/test_gpu_wide_nmf_rank.py: the
split-N NMF family for ranks up to 32 (csrc/nmf_global_rank.hip).

HALS at these ranks is chaotic in fp32 on unstructured data in the reference's own arithmetic (torch.rand inputs at
R >= 7: the fp32 oracle differs from the float64 oracle by 40-55 % in y, its gradient is NaN or ~1e13: components die,
b[r][r] + eps becomes ~eps and gate decisions flip), so parity is tested on a planted, well-separated family: component r
owns a block of rows and a block of columns, the initial factors start near the planted ones.

A (case, solver) pair is usable only if the fp32 oracle is within GUARD * max|ref| of the float64 oracle, for y and for
gx: a condition on the INPUTS, asserted on the CPU by both test files (`guard`).  The references are computed once per
process and handed out read-only."""
import functools

import torch

from oracle import cpu_ref as O

GUARD = 3e-5
L = 2

# (M, N, R, T, G (None: all iterations), solvers)
CASES = [
    (16, 777, 5, 4, None, ("mu", "hals")),      # smallest M, N % 4 = 1, ragged single slab
    (24, 2048, 8, 4, None, ("mu", "hals")),     # M <= 64 taken for R alone
    (64, 1024, 7, 4, None, ("mu", "hals")),     # stage-1 family, exactly one 1024-column slab
    (64, 1024, 7, 3, 1, ("mu", "hals")),
    (65, 1030, 1, 4, None, ("mu", "hals")),     # M just past the old cap, R = 1 shortcut, N % 4 = 2
    (128, 2052, 13, 4, None, ("mu", "hals")),   # three slabs, the last one 4 columns
    (256, 300, 25, 3, 1, ("mu", "hals")),       # N below one slab, truncated gradient
    (256, 520, 25, 4, None, ("mu", "hals")),    # stage 3
    (512, 520, 26, 4, None, ("mu", "hals")),    # M at the cap
    (512, 512, 26, 4, None, ("mu",)),           # stage 4 exactly (HALS gx 2.2e-5: too close to the guard)
    (512, 64, 6, 4, None, ("mu", "hals")),      # N below the thread count (64^3 input, stage 4)
    (40, 4100, 32, 4, None, ("mu",)),           # R at the cap, five slabs (HALS at R = 32 is chaotic even here: excluded)
    # past the V-update's 8192-column switch: one thread per column, nine slabs.  MU only: the HALS guard of this shape
    # depends on the host's BLAS (7.7e-7 / 1.3e-6 on one CPU, 1.9e-5 / 3.7e-5 on another): too close to the guard
    (64, 8200, 7, 4, None, ("mu",)),
]
PAIRS = [(M, N, R, T, G, s) for (M, N, R, T, G, solvers) in CASES for s in solvers]
IDS = [f"{M}x{N}-R{R}-T{T}-G{'all' if G is None else G}-{s}" for (M, N, R, T, G, s) in PAIRS]


@functools.lru_cache(maxsize=None)
def inputs(M, N, R):
    """(x, u0, v0, gy): x (L, M, N) planted rank-R plus 2 % noise; fp32, never modified by a caller"""
    torch.manual_seed(M * 1000 + N + R)
    ut, vt = torch.zeros(L, M, R), torch.zeros(L, N, R)
    for r in range(R):
        rows = slice(r * M // R, (r + 1) * M // R)
        cols = slice(r * N // R, (r + 1) * N // R)
        ut[:, rows, r] = 0.5 + torch.rand(L, rows.stop - rows.start)
        vt[:, cols, r] = 0.5 + torch.rand(L, cols.stop - cols.start)
    x = ut @ vt.mT + 0.02 * torch.rand(L, M, N)
    u0 = 0.8 * ut[0] + 0.1 * torch.rand(M, R) + 0.05
    v0 = 0.8 * vt[0] + 0.1 * torch.rand(N, R) + 0.05
    gy = torch.rand_like(x)
    return x, u0, v0, gy


@functools.lru_cache(maxsize=None)
def reference(M, N, R, T, G, solver):
    """dict: y64, gx64 (float64 oracle, as fp32 tensors), y_kink, gx_kink (max|fp32 oracle - fp64 oracle|),
    y_guard, gx_guard (the same relative to max|fp64|)"""
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
    """the conditioning guard of one (case, solver) pair: a property of the inputs, not of any kernel"""
    ref = reference(M, N, R, T, G, solver)
    print(f"guard {M}x{N} R{R} T{T} G{G} {solver}: y {ref['y_guard']:.2e} gx {ref['gx_guard']:.2e}")
    assert ref["y_guard"] <= GUARD and ref["gx_guard"] <= GUARD, (M, N, R, T, G, solver, ref["y_guard"], ref["gx_guard"])
    return ref
