"""-m gpu: the two-window HALS rank-1 backward of the fused FactMixer core that hands the first window's gradient to the
second as its factors (csrc/nmf_cf_gram.hip: fz_nmf_cf_bwd_store_factors / fz_nmf_cf_bwd_from_factors) against the two
fz_nmf_cf_bwd launches it replaces — bit for bit; every shape here has far fewer than 2^15 matrices, so the plain launches
take the row-space kernel for both windows — and once against float64 autograd through the CPU oracle's restatement of
relu -> SWMatricize.forward -> NMF(rank 1, "hals") -> SWMatricize.inverse_forward (factorizer.py:41-50; operations.py:417-434)."""
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
COFAC = 88             # u_T[8], gs[8], ga1[8], S[8][8] per patch

SHAPES = [(8, 8, 64), (16, 8, 64), (8, 16, 128)]
# the last pair has a SHIFTED first window: the second window's lookup of the first window's patch wraps on every axis
SHIFT_PAIRS = [[None, (4, 4, 4)], [None, (4, 0, 4)], [(4, 4, 0), (0, 4, 4)]]
SHIFT_IDS = ["w1_444", "w1_404", "w0_440_w1_044"]


def _s3(s):
    return (0, 0, 0) if s is None else ((s,) * 3 if isinstance(s, int) else tuple(s))


def _arr(s):
    return (N._i * 3)(*_s3(s))


def _input(S):
    """ReLU'd normals with an all-zero patch and an all-zero channel, and normals for dL/da"""
    torch.manual_seed(5)
    t = torch.relu(torch.randn(B, C, *S))
    t[0, :8, :8, :8, :8] = 0
    t[1, 3] = 0
    ga = torch.randn(B, C, *S)
    return t, ga


def _init(T, R=1):
    nmf = ft.NMF(size=(8, 512), rank=R, num_iters=T, init="uniform", solver="hals")
    return nmf.init.u0.clone(), nmf.init.v0.clone()


def _plain(td, u0, v0, gad, shifts, T, G):
    """one fz_nmf_cf_bwd per window: window 0 stores, window 1 accumulates"""
    gt = torch.empty_like(td)
    S = tuple(td.shape[2:])
    for w, s in enumerate(shifts):
        rc = N.lib().fz_nmf_cf_bwd(td.data_ptr(), u0.data_ptr(), v0.data_ptr(), gad.data_ptr(), gt.data_ptr(), B, C, *S, _arr(s),
                                   int(w > 0), len(shifts), 1, 1, T, G, N.SOLVER_ID["hals"], 1e-16, N.act_dtype(td),
                                   N.stream_ptr(td))
        N.check(rc, "fz_nmf_cf_bwd")
    return gt


def _workspaces(S, fill=None):
    make = torch.empty if fill is None else (lambda *a, **k: torch.full(*a, fill, **k))
    gcfac = make((B, C // 8, *S), device=DEV, dtype=torch.float32)
    cofac = make((B * (C // 8) * (S[0] // 8) * (S[1] // 8) * (S[2] // 8), COFAC), device=DEV, dtype=torch.float32)
    return gcfac, cofac


def _factored(td, v0, gad, shifts, T, G):
    S = tuple(td.shape[2:])
    gt = torch.full_like(td, float("nan"))
    gcfac, cofac = _workspaces(S, float("nan"))    # every element the second window reads must have been written by the first
    ad, st = N.act_dtype(td), N.stream_ptr(td)
    rc = N.lib().fz_nmf_cf_bwd_store_factors(td.data_ptr(), v0.data_ptr(), gad.data_ptr(), gcfac.data_ptr(), cofac.data_ptr(),
                                             B, C, *S, _arr(shifts[0]), 2, T, G, 1e-16, ad, st)
    N.check(rc, "fz_nmf_cf_bwd_store_factors")
    assert torch.isnan(gt.float()).all()           # the first window does not touch gt
    rc = N.lib().fz_nmf_cf_bwd_from_factors(td.data_ptr(), v0.data_ptr(), gad.data_ptr(), gcfac.data_ptr(), cofac.data_ptr(),
                                            gt.data_ptr(), B, C, *S, _arr(shifts[1]), _arr(shifts[0]), 2, T, G, 1e-16, ad, st)
    N.check(rc, "fz_nmf_cf_bwd_from_factors")
    assert not torch.isnan(gcfac).any() and not torch.isnan(cofac).any()
    return gt


def _supported(S, shifts, R=1, T=5, G=5, solver="hals", gate=1):
    flat = [v for s in shifts for v in _s3(s)]
    return bool(N.lib().fz_nmf_cf_bwd_factors_supported(C, *S, 8, 8, 8, 8, R, T, G, N.SOLVER_ID[solver], gate, len(shifts),
                                                        (N._i * len(flat))(*flat)))


@pytest.mark.parametrize("S", SHAPES)
@pytest.mark.parametrize("shifts", SHIFT_PAIRS, ids=SHIFT_IDS)
@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_factor_pair_equals_two_plain_launches_bitwise(S, shifts, dt):
    assert _supported(S, shifts)
    t, ga = _input(S)
    td, gad = t.to(DEV).to(dt), ga.to(DEV).to(dt)
    for T in (5, 1):
        u0, v0 = (x.to(DEV) for x in _init(T))
        ref = _plain(td, u0, v0, gad, shifts, T, T)
        got = _factored(td, v0, gad, shifts, T, T)
        torch.cuda.synchronize()
        assert torch.isfinite(ref.float()).all() and torch.isfinite(got.float()).all(), T
        assert ref.float().abs().max() > 0
        # bit patterns, not values: torch.equal would let +0 pass for −0
        bits = torch.int32 if dt == torch.float32 else torch.int16
        assert torch.equal(got.view(bits), ref.view(bits)), (T, int((got != ref).sum()))


class _Bytes:
    """functional.set_timer hook: the algorithmic bytes each timed launch declares"""

    def __init__(self):
        self.calls = []

    def launch(self, name, nbytes, fn, cols, flops):
        self.calls.append((name, nbytes))
        return fn()


def _core_grad(td, gad, geo, u0, v0, T=5, G=5, solver="hals", gate=True):
    tr = td.clone().requires_grad_(True)
    a = Fn.FactCoreFn.apply(tr, u0, v0, geo, T, G, solver, 1e-16, gate)
    (g,) = torch.autograd.grad(a, tr, gad)
    return g


@pytest.mark.parametrize("shifts", [SHIFT_PAIRS[0], SHIFT_PAIRS[2]], ids=[SHIFT_IDS[0], SHIFT_IDS[2]])
def test_factcore_backward_vs_float64_autograd_through_the_cpu_oracle(shifts):
    """the second pair has a shifted first window: the window-0 patch lookup wraps on every axis, checked here against code
    that shares nothing with the kernels"""
    S, T = (16, 8, 64), 5
    torch.manual_seed(5)
    z = torch.randn(B, C, *S)
    z[0, :8, :8, :8, :8] = 0
    z[1, 3] = 0
    ga = torch.randn(B, C, *S)
    u0, v0 = _init(T)
    m = ft.SWMatricize((None, C, *S), head_dim=8, patch_size=8, shifts=shifts)
    assert Fn.nmf_cf_bwd_factors_supported(m.geometry, 1, T, T, "hals", True)
    g = _core_grad(torch.relu(z).to(DEV), ga.to(DEV), m.geometry, u0.to(DEV), v0.to(DEV))
    sh = [_s3(s) for s in shifts]
    zd = z.double().requires_grad_(True)
    x = O.swm_forward(torch.relu(zd), head_dim=8, patch_size=8, shifts=sh)
    y = O.nmf_forward(x, u0.double(), v0.double(), T, "hals")
    a = O.swm_inverse(y, C, S, head_dim=8, patch_size=8, shifts=sh)
    (ref,) = torch.autograd.grad(a, zd, ga.double())
    P.close("gt from factors vs float64 autograd through the cpu oracle", g, ref.float())


def test_factcore_backward_declares_the_pairs_bytes():
    S, shifts = (16, 8, 64), [None, (4, 4, 4)]
    m = ft.SWMatricize((None, C, *S), head_dim=8, patch_size=8, shifts=shifts)
    u0, v0 = (x.to(DEV) for x in _init(5))
    t, ga = _input(S)
    td, gad = t.to(DEV), ga.to(DEV)
    tr = td.clone().requires_grad_(True)
    a = Fn.FactCoreFn.apply(tr, u0, v0, m.geometry, 5, 5, "hals", 1e-16, True)
    rec = _Bytes()
    Fn.set_timer(rec)
    try:
        n0 = N.launch_count()
        (g,) = torch.autograd.grad(a, tr, gad)
        assert N.launch_count() == n0 + 2
    finally:
        Fn.set_timer(None)
    n = td.numel()
    nf = 4 * (n // 8) + 4 * COFAC * (B * (C // 8) * (n // (B * C)) // 512)
    key = "nmf_cf_bwd_16x16x8x64"
    assert rec.calls == [(key, 2 * 4 * n + nf), (key, 3 * 4 * n + nf)], rec.calls
    assert torch.equal(g, _plain(td, u0, v0, gad, shifts, 5, 5))


OUTSIDE = [((8, 8, 64), [None, (4, 4, 4)], dict(R=2)), ((8, 8, 64), [None, 2, 4, 6], {}), ((8, 8, 64), [None, (4, 4, 2)], {}),
           ((8, 8, 32), [None, (4, 4, 4)], {}), ((8, 8, 64), [None, (4, 4, 4)], dict(solver="mu")),
           ((8, 8, 64), [None, (4, 4, 4)], dict(solver="cd")), ((8, 8, 64), [None, (4, 4, 4)], dict(gate=0)),
           ((8, 8, 64), [None, (4, 4, 4)], dict(T=5, G=3))]


@pytest.mark.parametrize("S,shifts,kw", OUTSIDE, ids=["rank2", "four_windows", "wshift2", "W32", "mu", "cd", "no_gate", "G_lt_T"])
def test_predicate_is_zero_outside_the_pair(S, shifts, kw):
    assert not _supported(S, shifts, **kw)
    assert _supported((8, 8, 64), [None, (4, 4, 4)]) and _supported((8, 8, 64), [(4, 4, 0), (0, 4, -4)], T=1, G=1)


def test_factcore_keeps_the_plain_loop_outside_the_pair():
    """G < T: v_start is a per-patch vector — the launch refuses, FactCoreFn.backward runs the two plain launches"""
    S, shifts, T, G = (8, 8, 64), [None, (4, 4, 4)], 5, 3
    m = ft.SWMatricize((None, C, *S), head_dim=8, patch_size=8, shifts=shifts)
    assert Fn.nmf_cf_supported(m.geometry, 1, T, G) and not Fn.nmf_cf_bwd_factors_supported(m.geometry, 1, T, G, "hals", True)
    u0, v0 = (x.to(DEV) for x in _init(T))
    t, ga = _input(S)
    td, gad = t.to(DEV), ga.to(DEV)
    gcfac, cofac = _workspaces(S)
    n0 = N.launch_count()
    rc = N.lib().fz_nmf_cf_bwd_store_factors(td.data_ptr(), v0.data_ptr(), gad.data_ptr(), gcfac.data_ptr(), cofac.data_ptr(),
                                             B, C, *S, _arr(None), 2, T, G, 1e-16, N.act_dtype(td), N.stream_ptr(td))
    assert rc == N.FZ_E_UNSUPPORTED and N.launch_count() == n0
    rec = _Bytes()
    Fn.set_timer(rec)
    try:
        g = _core_grad(td, gad, m.geometry, u0, v0, T, G)
    finally:
        Fn.set_timer(None)
    nb = td.numel() * 4
    assert [b for k, b in rec.calls if k.startswith("nmf_cf_bwd_")] == [3 * nb, 4 * nb]
    assert torch.equal(g, _plain(td, u0, v0, gad, shifts, T, G))
    assert torch.isfinite(g).all() and g.abs().max() > 0


def test_new_entry_points_check_their_arguments():
    S = (8, 8, 64)
    t, ga = _input(S)
    td, gad = t.to(DEV), ga.to(DEV)
    gt = torch.empty_like(td)
    gcfac, cofac = _workspaces(S)
    _, v0 = (x.to(DEV) for x in _init(5))
    z, s = _arr(None), _arr((4, 4, 4))
    ad, st = N.act_dtype(td), N.stream_ptr(td)
    L = N.lib()

    def store(t=td, S=S, v=v0, g=gad, gc=gcfac, co=cofac, nshift=2, shift=z):
        return L.fz_nmf_cf_bwd_store_factors(N.ptr(t), N.ptr(v), N.ptr(g), N.ptr(gc), N.ptr(co), B, C, *S, shift, nshift, 5, 5,
                                             1e-16, ad, st)

    def rebuild(t=td, S=S, v=v0, g=gad, gc=gcfac, co=cofac, o=gt, shift=s, prev=z, nshift=2):
        return L.fz_nmf_cf_bwd_from_factors(N.ptr(t), N.ptr(v), N.ptr(g), N.ptr(gc), N.ptr(co), N.ptr(o), B, C, *S, shift, prev,
                                            nshift, 5, 5, 1e-16, ad, st)

    n0 = N.launch_count()
    for k in ("t", "v", "g", "gc", "co"):
        assert store(**{k: None}) == FZ_E_ARG and rebuild(**{k: None}) == FZ_E_ARG, k
    assert rebuild(o=None) == FZ_E_ARG and rebuild(prev=None) == FZ_E_ARG
    S32 = (8, 8, 32)
    t32 = torch.zeros(B, C, *S32, device=DEV)
    assert store(t=t32, g=t32, S=S32) == N.FZ_E_UNSUPPORTED
    assert rebuild(t=t32, g=t32, S=S32, o=torch.empty_like(t32)) == N.FZ_E_UNSUPPORTED
    assert store(shift=_arr((0, 0, 2))) == N.FZ_E_UNSUPPORTED
    assert rebuild(shift=_arr((4, 4, 2))) == N.FZ_E_UNSUPPORTED and rebuild(prev=_arr((0, 0, 2))) == N.FZ_E_UNSUPPORTED
    assert store(nshift=4) == N.FZ_E_UNSUPPORTED and rebuild(nshift=4) == N.FZ_E_UNSUPPORTED
    assert N.launch_count() == n0                     # nothing was launched
    assert store() == 0 and rebuild() == 0
    torch.cuda.synchronize()
