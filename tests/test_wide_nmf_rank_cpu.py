"""No GPU: the split-N NMF family for ranks up to 32 and matrices up to 512 rows (csrc/nmf_global_rank.hip) — its gate
on both sides of every bound, the host-side refusals of its entry points, its workspace sizes and launch counts, the
reference's rank rule planned onto the three native families, the conditioning guard of every parity case
(tests/wide_rank_cases.py), and the composed paths it leaves alone."""
import ctypes
import warnings

import pytest
import torch

import factorizer_amd as ft
import parity as P
import wide_rank_cases as W
from factorizer_amd import _native
from factorizer_amd import functional as Fn
from oracle import cpu_ref as O


@pytest.fixture(scope="module")
def lib():
    from factorizer_amd import build
    build.build(verbose=False)
    return _native.lib()


@pytest.mark.parametrize("M,N,R,want", [
    (15, 4096, 5, 0), (16, 4096, 5, 1),          # M floor
    (512, 512, 26, 1), (513, 512, 26, 0),        # M cap
    (64, 4096, 32, 1), (64, 4096, 33, 0),        # R cap
    (16, 4096, 16, 1), (16, 4096, 17, 0),        # R = M, R = M + 1
    (24, 100, 24, 1), (24, 100, 25, 0),
    (8, 1200, 5, 0),                             # stays composed (tests/test_gpu_parity.py pins it)
    (16, 4096, 1, 0), (8, 512, 2, 0),            # shapes of the old families
    (64, 1024, 4, 0), (65, 1024, 4, 1), (64, 1024, 5, 1), (65, 1030, 1, 1),
    (64, 1, 7, 1), (64, 0, 7, 0), (64, 1024, 0, 0),
])
def test_gate_table(lib, M, N, R, want):
    assert lib.fz_gnmfx_supported(M, N, R, 5, 5) == want == int(Fn.gnmfx_supported(M, N, R, 5, 5))
    if want:   # only what both existing families decline
        assert not lib.fz_gnmf_supported(M, N, R, 5, 5) and not lib.fz_nmf_supported(M, N, R, 5, 5)
    assert lib.fz_gnmfx_supported(M, N, R, -1, 0) == 0
    assert lib.fz_gnmfx_supported(M, N, R, 0, 0) == want


def test_entry_points_refuse(lib):
    p8 = ctypes.c_void_p(8)   # a non-null pointer value the host code never dereferences

    def fwd(M, N, R, solver, x=p8, ws=p8, nmat=2):
        return lib.fz_gnmfx_fwd(x, p8, p8, p8, None, None, nmat, M, N, R, 5, solver, 1e-16, ws, None)

    def bwd(M, N, R, solver, gy=p8, gu=None, gv=None, gx=p8, G=5, nmat=2):
        return lib.fz_gnmfx_bwd(p8, p8, p8, gy, gu, gv, gx, nmat, M, N, R, 5, G, solver, 1e-16, p8, None)

    for M, N, R in ((8, 1200, 5), (16, 4096, 1), (8, 512, 2), (513, 512, 26), (64, 4096, 33), (16, 4096, 17)):
        assert fwd(M, N, R, 1) == -2 and b"fz_gnmfx_fwd" in lib.fz_last_error_string()
        assert bwd(M, N, R, 1) == -2 and b"fz_gnmfx_bwd" in lib.fz_last_error_string()
        assert lib.fz_gnmfx_workspace_bytes(2, M, N, R, 5, 1) == -1
    for solver in (_native.SOLVER_ID["cd"], _native.SOLVER_ID["smu"], 4, -1):
        assert fwd(64, 1024, 7, solver) == -4 and b"solver" in lib.fz_last_error_string()
        assert bwd(64, 1024, 7, solver) == -4 and b"solver" in lib.fz_last_error_string()
    assert fwd(64, 1024, 7, 1, x=None) == -4 and b"null" in lib.fz_last_error_string()
    assert fwd(64, 1024, 7, 0, ws=None) == -4
    assert bwd(64, 1024, 7, 1, gy=None) == -4 and b"null" in lib.fz_last_error_string()
    assert bwd(64, 1024, 7, 1, gx=None) == -4
    assert fwd(64, 1024, 7, 1, nmat=65536) == -1 and bwd(64, 1024, 7, 0, nmat=65536) == -1
    assert bwd(64, 1024, 7, 1, G=0) == -4 and b"no iteration" in lib.fz_last_error_string()   # the caller returns zeros
    assert fwd(64, 1024, 7, 1, nmat=0) == 0 and bwd(64, 1024, 7, 1, nmat=0) == 0              # nothing to do


@pytest.mark.parametrize("M,N,R", [(64, 1024, 7), (128, 2052, 13), (512, 512, 26), (40, 4100, 32), (65, 1030, 1)])
def test_sizes_and_counts(lib, M, N, R):
    ws = lib.fz_gnmfx_workspace_bytes
    assert ws(-1, M, N, R, 5, 0) == -1
    for backward in (0, 1):
        sizes = [ws(n, M, N, R, 5, backward) for n in (1, 2, 3, 8)]
        assert sizes[0] > 0 and sizes == sorted(sizes)
        sizes = [ws(2, M, N, R, T, backward) for T in (0, 1, 2, 5, 9)]
        assert sizes[0] > 0 and sizes == sorted(sizes)
    for T in (0, 1, 5):
        assert 0 < ws(2, M, N, R, T, 0) <= ws(2, M, N, R, T, 1)
    ln = lib.fz_gnmfx_launches
    for T in (0, 1, 3, 5):
        assert ln(M, N, R, T, T, 0) >= 1
        for G in range(0, T + 1):
            assert ln(M, N, R, T, G, 1) >= ln(M, N, R, T, G, 0) == ln(M, N, R, T, T, 0)
        assert ln(M, N, R, T, T + 3, 1) == ln(M, N, R, T, T, 1)      # Tgrad is clamped to T


WIDTHS = (32, 64, 128, 256, 512)
TABLE = {128: (4, 7, 13, 25, 26), 64: (4, 7, 13, 18, 6)}


@pytest.mark.parametrize("side", [128, 64])
def test_rank_rule_plans_onto_a_native_family(lib, side):
    """the reference's default-constructed model at side^3: every stage's (M, N, rank=None) is covered by one of the
    three native families, with the ranks of matrix_factorization.py:406-408"""
    for i, (C, want) in enumerate(zip(WIDTHS, TABLE[side])):
        N = (side >> i) ** 3
        nmf = ft.NMF((C, N), rank=None)
        assert nmf.rank == want == O.nmf_rank(C, N), (C, N, nmf.rank)
        T, G = nmf.num_iters, nmf.num_iters
        fams = [Fn.nmf_supported(C, N, nmf.rank, T, G), Fn.gnmf_supported(C, N, nmf.rank, T, G),
                Fn.gnmfx_supported(C, N, nmf.rank, T, G)]
        assert any(fams), (C, N, nmf.rank)
        if i > 0:
            assert fams == [False, False, True], (C, N, nmf.rank, fams)


def test_rank_above_the_cap_is_not_planned(lib):
    nmf = ft.NMF((512, 32 * 32), rank=None)     # 2-D 512^2 input, stage 4
    assert nmf.rank == 35
    assert not (Fn.nmf_supported(512, 1024, 35, 5, 5) or Fn.gnmf_supported(512, 1024, 35, 5, 5)
                or Fn.gnmfx_supported(512, 1024, 35, 5, 5))


@pytest.mark.parametrize("M,N,R,T,G,solver", W.PAIRS, ids=W.IDS)
def test_conditioning_guard(M, N, R, T, G, solver):
    """a condition on the inputs: the fp32 oracle within 3e-5 of the float64 oracle, y and gx"""
    assert W.GUARD == 3e-5
    W.guard(M, N, R, T, G, solver)


@pytest.mark.parametrize("solver", ["mu", "hals"])
@pytest.mark.parametrize("M,N,R", [(8, 1200, 5), (64, 1024, 7)])
def test_composed_paths_are_untouched(M, N, R, solver):
    """CPU tensors (any shape) and the composed path of a refused shape still compute the oracle's values"""
    x, u0, v0, gy = W.inputs(M, N, R)
    nmf = ft.NMF(size=(M, N), rank=R, num_iters=4, init="uniform", solver=solver)
    nmf.load_state_dict({"init.u0": u0, "init.v0": v0})
    xc = x.clone().requires_grad_(True)
    with warnings.catch_warnings():
        warnings.simplefilter("error", RuntimeWarning)
        y = nmf(xc)
    assert nmf._wide is False
    (gx,) = torch.autograd.grad(y, xc, gy)
    P.close(f"composed y {M}x{N} R{R} {solver}", y, O.nmf_forward(x, u0, v0, 4, solver))
    P.close(f"composed gx {M}x{N} R{R} {solver}", gx, O.nmf_backward(x, u0, v0, gy, 4, solver))
