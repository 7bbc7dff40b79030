"""-m gpu: the two-window rank-1 forward of the fused FactMixer core that hands the first window to the second as its
factors (csrc/nmf_cf_fwd.hip; entry points in csrc/nmf_cf.hip: fz_nmf_cf_fwd_store_factors / fz_nmf_cf_fwd_from_factors) against the two fz_nmf_cf_fwd launches it
replaces — bit for bit, the issue's contract — and once against the CPU oracle's restatement of the reference chain
SWMatricize.forward -> NMF(rank 1) -> SWMatricize.inverse_forward (factorizer.py:41-50; operations.py:417-434)."""
import pytest
import torch

import factorizer_amd as ft
from factorizer_amd import _native as N
from factorizer_amd import functional as Fn
from oracle import cpu_ref as O
import parity as P

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
B, C = 2, 16
FZ_E_ARG = -4          # include/factorizer_hip.h

SHAPES = [(8, 8, 64), (16, 8, 64), (8, 16, 128)]
# the last pair has a SHIFTED first window: the second window's lookup of the first window's patch wraps on every axis
SHIFT_PAIRS = [[None, (4, 4, 4)], [None, (4, 0, 4)], [(4, 4, 0), (0, 4, 4)]]


def _s3(s):
    return (0, 0, 0) if s is None else ((s,) * 3 if isinstance(s, int) else tuple(s))


def _input(S, signed=False):
    """ReLU'd normals (both signs for the sign-free solvers) with an all-zero patch and an all-zero channel"""
    torch.manual_seed(5)
    t = torch.randn(B, C, *S)
    if not signed:
        t = torch.relu(t)
    t[0, :8, :8, :8, :8] = 0
    t[1, 3] = 0
    return t


def _init(T):
    nmf = ft.NMF(size=(8, 512), rank=1, num_iters=T, init="uniform", solver="hals")
    return nmf.init.u0.clone(), nmf.init.v0.clone()


def _arr(s):
    return (N._i * 3)(*_s3(s))


def _plain(td, u0, v0, shifts, T, solver):
    """one fz_nmf_cf_fwd per window: window 0 stores 0 + z0, the last window adds and divides"""
    out = torch.empty_like(td)
    S = tuple(td.shape[2:])
    for w, s in enumerate(shifts):
        rc = N.lib().fz_nmf_cf_fwd(td.data_ptr(), u0.data_ptr(), v0.data_ptr(), out.data_ptr(), B, C, *S, _arr(s), int(w > 0),
                                   len(shifts) if w == len(shifts) - 1 else 1, 1, T, N.SOLVER_ID[solver], 1e-16,
                                   N.act_dtype(td), N.stream_ptr(td))
        N.check(rc, "fz_nmf_cf_fwd")
    return out


def _workspaces(S, fill=None):
    make = torch.empty if fill is None else (lambda *a, **k: torch.full(*a, fill, **k))
    vfac = make((B, C // 8, *S), device=DEV, dtype=torch.float32)
    ufac = make((B * (C // 8) * (S[0] // 8) * (S[1] // 8) * (S[2] // 8), 8), device=DEV, dtype=torch.float32)
    return vfac, ufac


def _factored(td, u0, v0, shifts, T, solver):
    S = tuple(td.shape[2:])
    out = torch.empty_like(td)
    vfac, ufac = _workspaces(S, float("nan"))      # every element the second window reads must have been written by the first
    ad, st = N.act_dtype(td), N.stream_ptr(td)
    rc = N.lib().fz_nmf_cf_fwd_store_factors(td.data_ptr(), u0.data_ptr(), v0.data_ptr(), vfac.data_ptr(), ufac.data_ptr(), B, C,
                                             *S, _arr(shifts[0]), 1, T, N.SOLVER_ID[solver], 1e-16, ad, st)
    N.check(rc, "fz_nmf_cf_fwd_store_factors")
    rc = N.lib().fz_nmf_cf_fwd_from_factors(td.data_ptr(), u0.data_ptr(), v0.data_ptr(), vfac.data_ptr(), ufac.data_ptr(),
                                            out.data_ptr(), B, C, *S, _arr(shifts[1]), _arr(shifts[0]), 2, 1, T,
                                            N.SOLVER_ID[solver], 1e-16, ad, st)
    N.check(rc, "fz_nmf_cf_fwd_from_factors")
    assert not torch.isnan(vfac).any() and not torch.isnan(ufac).any()
    return out


def _supported(S, shifts, R=1):
    flat = [v for s in shifts for v in _s3(s)]
    return bool(N.lib().fz_nmf_cf_factors_supported(C, *S, 8, 8, 8, 8, R, 5, 5, len(shifts), (N._i * len(flat))(*flat)))


@pytest.mark.parametrize("S", SHAPES)
@pytest.mark.parametrize("shifts", SHIFT_PAIRS, ids=["w1_444", "w1_404", "w0_440_w1_044"])
@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_factor_pair_equals_two_plain_launches_bitwise(S, shifts, dt):
    """every solver the issue names, T = 5 and T = 1; `cd` on inputs of both signs, so that products u·v = −0 occur and the
    `0.0f +` of the first window matters"""
    assert _supported(S, shifts)
    for solver in ("hals", "mu", "cd"):
        td = _input(S, signed=solver == "cd").to(DEV).to(dt)
        for T in (5, 1):
            u0, v0 = (x.to(DEV) for x in _init(T))
            ref = _plain(td, u0, v0, shifts, T, solver)
            got = _factored(td, u0, v0, shifts, T, solver)
            torch.cuda.synchronize()
            assert torch.isfinite(ref.float()).all(), (solver, T)
            # bit patterns, not values: torch.equal would let +0 pass for −0
            bits = torch.int32 if dt == torch.float32 else torch.int16
            assert torch.equal(got.view(bits), ref.view(bits)), (solver, T, int((got != ref).sum()))


def test_factor_pair_vs_cpu_oracle():
    S, shifts, T = (16, 8, 64), [None, (4, 4, 4)], 5
    t = _input(S)
    u0, v0 = _init(T)
    got = _factored(t.to(DEV), u0.to(DEV), v0.to(DEV), shifts, T, "hals")
    sh = [_s3(s) for s in shifts]
    x = O.swm_forward(t, head_dim=8, patch_size=8, shifts=sh)
    y = O.nmf_forward(x, u0, v0, T, "hals")
    ref = O.swm_inverse(y, C, S, head_dim=8, patch_size=8, shifts=sh)
    P.close("a from factors vs cpu oracle", got, ref)


class _Bytes:
    """functional.set_timer hook: the algorithmic bytes each timed launch declares"""

    def __init__(self):
        self.calls = []

    def launch(self, name, nbytes, fn, cols, flops):
        self.calls.append((name, nbytes))
        return fn()


def _core(td, geo, u0, v0, T=5, G=5):
    tr = td.clone().requires_grad_(True)
    a = Fn.FactCoreFn.apply(tr, u0, v0, geo, T, G, "hals", 1e-16, True)
    return tr, a


def test_factcore_takes_the_factor_path_on_a_supported_geometry():
    S, shifts = (16, 8, 64), [None, (4, 4, 4)]
    m = ft.SWMatricize((None, C, *S), head_dim=8, patch_size=8, shifts=shifts)
    assert Fn.nmf_cf_factors_supported(m.geometry, 1, 5, 5)
    u0, v0 = (x.to(DEV) for x in _init(5))
    td = _input(S).to(DEV)
    _core(td, m.geometry, u0, v0)          # warm the allocator and the library
    torch.cuda.synchronize()
    rec = _Bytes()
    Fn.set_timer(rec)
    try:
        n0 = N.launch_count()
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        with torch.no_grad():
            a = Fn.FactCoreFn.apply(td, u0, v0, m.geometry, 5, 5, "hals", 1e-16, True)
        torch.cuda.synchronize()
        peak = torch.cuda.max_memory_allocated() - base
        assert N.launch_count() == n0 + 2
    finally:
        Fn.set_timer(None)
    nb = td.numel() * 4
    # the output, the v plane (1/8) and u (1/512) — no second tensor of t's size (allocator granularity: 512 B per block)
    assert nb <= peak < nb + nb // 8 + nb // 512 + 4096, (peak, nb)
    key = "nmf_cf_fwd_16x16x8x64"
    assert rec.calls == [(key, nb + nb // 8), (key, 2 * nb + nb // 8)], rec.calls
    assert torch.equal(a, _plain(td, u0, v0, shifts, 5, "hals"))


@pytest.mark.parametrize("S,shifts,R", [((8, 8, 32), [None, (4, 4, 4)], 1), ((8, 8, 64), [None, (4, 4, 2)], 1),
                                        ((8, 8, 64), [None, 2, 4, 6], 1), ((8, 8, 64), [None, (4, 4, 4)], 2)],
                         ids=["W32", "wshift2", "four_windows", "rank2"])
def test_factcore_keeps_the_plain_path_elsewhere(S, shifts, R):
    m = ft.SWMatricize((None, C, *S), head_dim=8, patch_size=8, shifts=shifts)
    geo = m.geometry
    assert Fn.nmf_cf_supported(geo, R, 5, 5) and not Fn.nmf_cf_factors_supported(geo, R, 5, 5)
    nmf = ft.NMF(size=(8, 512), rank=R, num_iters=5, init="uniform", solver="hals")
    u0, v0 = nmf.init.u0.to(DEV), nmf.init.v0.to(DEV)
    td = _input(S).to(DEV)
    rec = _Bytes()
    Fn.set_timer(rec)
    try:
        n0 = N.launch_count()
        with torch.no_grad():
            a = Fn.FactCoreFn.apply(td, u0, v0, geo, 5, 5, "hals", 1e-16, True)
        assert N.launch_count() == n0 + geo.nshift
    finally:
        Fn.set_timer(None)
    nb = td.numel() * 4
    assert [b for _, b in rec.calls] == [2 * nb] + [3 * nb] * (geo.nshift - 1)
    # the same windows launched by hand through fz_nmf_cf_fwd
    out = torch.empty_like(td)
    for w, s in enumerate(geo.shifts3):
        N.check(N.lib().fz_nmf_cf_fwd(td.data_ptr(), u0.data_ptr(), v0.data_ptr(), out.data_ptr(), B, C, *S, (N._i * 3)(*s),
                                      int(w > 0), geo.nshift if w == geo.nshift - 1 else 1, R, 5, N.SOLVER_ID["hals"], 1e-16,
                                      N.act_dtype(td), N.stream_ptr(td)), "fz_nmf_cf_fwd")
    assert torch.equal(a, out)


def test_gradient_through_the_factor_path_equals_the_plain_path(monkeypatch):
    S, shifts = (16, 8, 64), [(4, 4, 0), (0, 4, 4)]
    m = ft.SWMatricize((None, C, *S), head_dim=8, patch_size=8, shifts=shifts)
    u0, v0 = (x.to(DEV) for x in _init(5))
    td = _input(S).to(DEV)
    torch.manual_seed(7)
    ga = torch.randn(B, C, *S, device=DEV)
    n0 = N.launch_count()
    tr, a = _core(td, m.geometry, u0, v0)
    (g,) = torch.autograd.grad(a, tr, ga)
    assert N.launch_count() > n0
    monkeypatch.setattr(Fn, "nmf_cf_factors_supported", lambda *a, **k: False)     # the dispatcher's other branch
    tr2, a2 = _core(td, m.geometry, u0, v0)
    (g2,) = torch.autograd.grad(a2, tr2, ga)
    assert torch.equal(a, a2) and torch.equal(g, g2)
    assert torch.isfinite(g).all() and g.abs().max() > 0


def test_new_entry_points_check_their_arguments():
    S = (8, 8, 64)
    td = _input(S).to(DEV)
    out = torch.empty_like(td)
    vfac, ufac = _workspaces(S)
    z, s = _arr(None), _arr((4, 4, 4))
    ad, st = N.act_dtype(td), N.stream_ptr(td)
    L = N.lib()

    def store(t=td, S=S, vf=vfac, uf=ufac, R=1):
        u0, v0 = _dev_init(R)
        return L.fz_nmf_cf_fwd_store_factors(t.data_ptr(), u0.data_ptr(), v0.data_ptr(), N.ptr(vf), N.ptr(uf), B, C, *S, z, R, 5,
                                             N.SOLVER_ID["hals"], 1e-16, ad, st)

    def rebuild(t=td, S=S, vf=vfac, uf=ufac, R=1, o=out, shift=s, prev=z):
        u0, v0 = _dev_init(R)
        return L.fz_nmf_cf_fwd_from_factors(t.data_ptr(), u0.data_ptr(), v0.data_ptr(), N.ptr(vf), N.ptr(uf), N.ptr(o), B, C, *S,
                                            shift, prev, 2, R, 5, N.SOLVER_ID["hals"], 1e-16, ad, st)

    n0 = N.launch_count()
    assert store(vf=None) == FZ_E_ARG and store(uf=None) == FZ_E_ARG
    assert rebuild(vf=None) == FZ_E_ARG and rebuild(uf=None) == FZ_E_ARG and rebuild(o=None) == FZ_E_ARG
    assert rebuild(prev=None) == FZ_E_ARG
    assert store(R=2) == N.FZ_E_UNSUPPORTED and rebuild(R=2) == N.FZ_E_UNSUPPORTED
    S32 = (8, 8, 32)
    t32 = _input(S32).to(DEV)
    assert store(t=t32, S=S32) == N.FZ_E_UNSUPPORTED and rebuild(t=t32, S=S32, o=torch.empty_like(t32)) == N.FZ_E_UNSUPPORTED
    assert rebuild(shift=_arr((4, 4, 2))) == N.FZ_E_UNSUPPORTED and rebuild(prev=_arr((0, 0, 2))) == N.FZ_E_UNSUPPORTED
    assert N.launch_count() == n0                     # nothing was launched
    assert not _supported(S, [None, (4, 4, 4)], R=2) and not _supported(S32, [None, (4, 4, 4)])
    assert not _supported(S, [None, (4, 4, 2)]) and not _supported(S, [None, 2, 4, 6]) and not _supported(S, [None])
    assert _supported(S, [None, (4, 4, 4)]) and _supported(S, [(4, 4, 0), (0, 4, -4)])
    assert store() == 0 and rebuild() == 0
    torch.cuda.synchronize()


def _dev_init(R):
    nmf = ft.NMF(size=(8, 512), rank=R, num_iters=5, init="uniform", solver="hals")
    return nmf.init.u0.to(DEV), nmf.init.v0.to(DEV)
