"""-m gpu: the one-pass backward of the full-resolution decoder node (csrc/upcat_bwd.hip, fz_upcat_bwd; dispatched by
pointwise.UpCatLinearFn.backward for 32 adapter outputs, 32 skip channels, 64 deep channels, fine W % 64 == 0, fp32 storage)
against the three launches over g it replaces (FZ_UPCAT_BWD=0) and against a float64 evaluation of
adapter(cat([skip, conv_transpose3d(deep)])).  Coarse extents are (D, H, W).

Bounds: max |Δ| <= 1e-5 · max |ref| for the two input gradients and 1e-4 for the parameter gradients between the kernel forms
(the bounds tests/test_gpu_dense.py uses between kernel forms), 1e-4 against float64; bf16 storage is not built: it must take
the three launches."""
import ctypes
import functools

import pytest
import torch
import torch.nn.functional as F

from factorizer_amd import _native as N
from factorizer_amd import functional as Fn
from factorizer_amd import pointwise as PW

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAMES = ("g_skip", "g_deep", "gw_t", "gb_t", "gw_ad", "gb_ad")
OLD = ("dgrad_wgrad_32", "tconv_k2s2_dgrad_32->64", "wgrad_tconv_k2s2_64x256")


@functools.lru_cache(maxsize=None)
def _inputs(S, B, C1=32, Cd=64, O=32, M=32):
    """seeded host inputs of one problem (shared by every test that uses the shape; never modified)"""
    gen = torch.Generator().manual_seed(1000 * B + S[0] * 101 + S[1] * 11 + S[2] + C1 + Cd)
    fine = tuple(2 * d for d in S)
    r = lambda *sh: torch.randn(*sh, generator=gen)   # noqa: E731
    return dict(skip=r(B, C1, *fine), deep=r(B, Cd, *S), w_t=r(Cd, O, 2, 2, 2) * 0.2, b_t=r(O) * 0.1, w_ad=r(M, C1 + O, 1) * 0.2,
                b_ad=r(M) * 0.1, g=r(B, M, *fine))


def _backward(inp, one_pass, has_bt=True, has_bad=True, deep_grad=True, dt=torch.float32, timer=None):
    """the six gradients of one UpCatLinearFn backward (None where a bias is absent or deep needs none)"""
    t = {k: v.to(DEV) for k, v in inp.items()}
    skip = t["skip"].to(dt).requires_grad_(True)
    deep = t["deep"].to(dt).requires_grad_(deep_grad)
    w_t, w_ad = t["w_t"].requires_grad_(True), t["w_ad"].requires_grad_(True)
    b_t = t["b_t"].requires_grad_(True) if has_bt else None
    b_ad = t["b_ad"].requires_grad_(True) if has_bad else None
    y = PW.up_cat_linear(skip, deep, w_t, b_t, w_ad, b_ad)
    want = {"g_skip": skip, "g_deep": deep if deep_grad else None, "gw_t": w_t, "gb_t": b_t, "gw_ad": w_ad, "gb_ad": b_ad}
    keys = [k for k in NAMES if want[k] is not None]
    was = PW._UPCAT_BWD
    PW._UPCAT_BWD = one_pass
    if timer is not None:
        Fn.set_timer(timer)
    try:
        gr = torch.autograd.grad(y, [want[k] for k in keys], t["g"].to(dt))
        torch.cuda.synchronize()
    finally:
        PW._UPCAT_BWD = was
        Fn.set_timer(None)
    out = dict.fromkeys(NAMES)
    out.update(zip(keys, gr))
    return out


@functools.lru_cache(maxsize=None)
def _three(S, B, has_bt=True, has_bad=True):
    return _backward(_inputs(S, B), False, has_bt, has_bad)


@functools.lru_cache(maxsize=None)
def _one(S, B, has_bt=True, has_bad=True):
    return _backward(_inputs(S, B), True, has_bt, has_bad)


@functools.lru_cache(maxsize=None)
def _fp64(S, B, has_bt=True, has_bad=True):
    inp = _inputs(S, B)
    r = {k: inp[k].double().requires_grad_(True) for k in ("skip", "deep", "w_t", "b_t", "w_ad", "b_ad")}
    up = F.conv_transpose3d(r["deep"], r["w_t"], r["b_t"] if has_bt else None, stride=2)
    y = F.conv1d(torch.cat([r["skip"], up], 1).flatten(2), r["w_ad"], r["b_ad"] if has_bad else None).reshape(inp["g"].shape)
    want = {"g_skip": r["skip"], "g_deep": r["deep"], "gw_t": r["w_t"], "gb_t": r["b_t"] if has_bt else None, "gw_ad": r["w_ad"],
            "gb_ad": r["b_ad"] if has_bad else None}
    keys = [k for k in NAMES if want[k] is not None]
    out = dict.fromkeys(NAMES)
    out.update(zip(keys, torch.autograd.grad(y, [want[k] for k in keys], inp["g"].double())))
    return out


def _check(got, ref, tol_in, tol_par, what):
    for k in NAMES:
        assert (got[k] is None) == (ref[k] is None), (k, what)
        if ref[k] is None:
            continue
        scale = ref[k].abs().max().item() + 1e-30
        err = (got[k].double().cpu() - ref[k].double().cpu()).abs().max().item()
        tol = tol_in if k in ("g_skip", "g_deep") else tol_par
        print(f"{what} {k}: max|d| / max|ref| = {err / scale:.3e} (bound {tol:.0e})")
        assert err <= tol * scale, (k, what, err / scale)


SMALL = [((1, 1, 32), 1),     # one tile in the whole launch
         ((3, 2, 64), 2),     # odd D, two segments per row
         ((2, 3, 32), 3)]     # a tile count that is a multiple of nothing
LARGE = ((16, 32, 96), 1)     # 1 536 tiles on 256 persistent workgroups, six each (uneven walks: test_uneven_tiles_per_workgroup)


@pytest.mark.parametrize("S,B", SMALL + [LARGE])
def test_one_pass_vs_three_launches(S, B):
    _check(_one(S, B), _three(S, B), 1e-5, 1e-4, "vs three launches")


def test_uneven_tiles_per_workgroup():
    """(16, 32, 96), B = 1 has 1 536 tiles = 6 x 256; (5, 11, 96), B = 1 has 165 (every workgroup one tile) and (9, 11, 96), B = 1
    has 297: 41 workgroups walk two tiles and 215 one."""
    for S, B in (((5, 11, 96), 1), ((9, 11, 96), 1)):
        _check(_one(S, B), _three(S, B), 1e-5, 1e-4, f"{S} vs three launches")


@pytest.mark.parametrize("S,B", SMALL)
def test_one_pass_vs_float64(S, B):
    _check(_one(S, B), _fp64(S, B), 1e-4, 1e-4, "vs float64")


@pytest.mark.parametrize("has_bt,has_bad", [(True, True), (True, False), (False, True), (False, False)])
def test_bias_combinations(has_bt, has_bad):
    S, B = SMALL[0]
    got = _one(S, B, has_bt, has_bad)
    _check(got, _three(S, B, has_bt, has_bad), 1e-5, 1e-4, "vs three launches")
    _check(got, _fp64(S, B, has_bt, has_bad), 1e-4, 1e-4, "vs float64")


@pytest.mark.parametrize("S,B", [SMALL[1], LARGE])
def test_replay_is_bit_identical(S, B):
    a, b = _one(S, B), _backward(_inputs(S, B), True)
    for k in NAMES:
        assert torch.equal(a[k], b[k]), k


def test_deferred_finishes_are_bit_identical():
    """with deferral armed by an owner of the parameters (as FlatAdamW.zero_grad arms it) the node's finish jobs — the two of
    fz_upcat_bwd and fz_upcat_wgrads behind them — run at the end of the backward and give the bits of the immediate form"""
    S, B = SMALL[1]
    inp = {k: v.to(DEV) for k, v in _inputs(S, B).items()}

    def run(defer):
        leaves = {k: inp[k].clone().requires_grad_(True) for k in ("skip", "deep", "w_t", "b_t", "w_ad", "b_ad")}
        params = [leaves[k] for k in ("w_t", "b_t", "w_ad", "b_ad")]
        f0, r0 = PW._Defer.flushed, PW._Defer.refused
        PW.defer_finishes(defer)
        try:
            if defer:
                PW.arm_deferred_finishes(params)
            y = PW.up_cat_linear(leaves["skip"], leaves["deep"], leaves["w_t"], leaves["b_t"], leaves["w_ad"], leaves["b_ad"])
            y.backward(inp["g"])
            torch.cuda.synchronize()
        finally:
            PW.defer_finishes(False)
        return [leaves[k].grad.clone() for k in ("skip", "deep", "w_t", "b_t", "w_ad", "b_ad")], PW._Defer.flushed - f0, PW._Defer.refused - r0

    g_def, queued, refused = run(True)
    g_imm, queued0, _ = run(False)
    assert queued == 3 and refused == 0 and queued0 == 0, (queued, refused, queued0)   # row sums of Gt, of dW_a | Σg, the contraction
    for k, u, v in zip(NAMES, g_def, g_imm):
        assert torch.equal(u, v), k
    for k, u in zip(NAMES, g_def):
        assert torch.equal(u, _one(S, B)[k].reshape(u.shape)), k


def _launches(inp, one_pass, **kw):
    t = Fn.KernelTimer()
    out = _backward(inp, one_pass, timer=t, **kw)
    return out, t.summary()


@pytest.mark.parametrize("S,C,Cd,deep_grad", [((2, 2, 16), 32, 64, True),     # fine W = 32
                                              ((1, 2, 32), 16, 32, True),     # 16 skip channels (a 16-wide level: 16 / 16 / 32)
                                              ((1, 2, 32), 32, 128, True),    # 128 deep channels
                                              ((1, 2, 32), 32, 64, False)])   # deep needs no gradient
def test_outside_the_predicate_takes_the_old_launches(S, C, Cd, deep_grad):
    inp = _inputs(S, 2, C, Cd, C, C)
    a, la = _launches(inp, True, deep_grad=deep_grad)
    b, _ = _launches(inp, False, deep_grad=deep_grad)
    assert not any(n.startswith("upcat_bwd") for n in la), sorted(la)
    assert f"wgrad_tconv_k2s2_{Cd}x{8 * C}" in la and (f"tconv_k2s2_dgrad_{C}->{Cd}" in la) == deep_grad, sorted(la)
    assert ("dgrad_wgrad_32" in la) == (C == 32), sorted(la)
    for k in NAMES:
        assert (a[k] is None and b[k] is None) or torch.equal(a[k], b[k]), k


def test_bf16_storage_takes_the_old_launches():
    """bf16 storage is not instantiated: the predicate answers 0 and the node keeps its three launches (2e-2 of float64)"""
    S, B = (4, 8, 32), 2
    assert N.lib().fz_upcat_bwd_supported(32, 64, *S, N.STORE_F32) == 1 and N.lib().fz_upcat_bwd_supported(32, 64, *S, N.STORE_BF16) == 0
    a, la = _launches(_inputs(S, B), True, dt=torch.bfloat16)
    assert not any(n.startswith("upcat_bwd") for n in la) and all(n in la for n in OLD), sorted(la)
    ref = _fp64(S, B)
    _check(a, ref, 2e-2, 2e-2, "bf16 vs float64")


def test_declared_bytes_and_launch_names():
    S, B = SMALL[1]
    inp = _inputs(S, B)
    _, la = _launches(inp, True)
    new = [n for n in la if n.startswith("upcat_bwd")]
    assert new == ["upcat_bwd_64->32"] and la[new[0]]["calls"] == 1, sorted(la)
    assert not any(n in la for n in OLD), sorted(la)
    U = 4 * inp["g"].numel()
    assert la[new[0]]["bytes"] == 3.5 * U and la[new[0]]["cols"] == B * 8 * S[0] * S[1] * S[2]
    assert la[new[0]]["flops"] == 12288 * B * 8 * S[0] * S[1] * S[2]
    _, lb = _launches(inp, False)
    assert all(n in lb for n in OLD) and not any(n.startswith("upcat_bwd") for n in lb), sorted(lb)


def test_predicate_and_argument_checks():
    lib = N.lib()
    ok = lambda *a: lib.fz_upcat_bwd_supported(*a, N.STORE_F32)   # noqa: E731
    assert ok(32, 64, 1, 1, 32) == 1 and ok(32, 64, 64, 64, 64) == 1
    assert ok(32, 64, 2, 2, 16) == 0 and ok(32, 64, 2, 2, 48) == 0 and ok(16, 64, 1, 1, 32) == 0 and ok(32, 128, 1, 1, 32) == 0
    assert ok(64, 128, 32, 32, 32) == 0                                # the stage-1 level keeps its launches
    assert lib.fz_upcat_bwd_workspace_bytes(1, 1, 1, 32) == (64 * 32 * 8 + 4 * 1120) * 4
    assert lib.fz_upcat_bwd_workspace_bytes(2, 64, 64, 64) == 256 * (64 * 32 * 8 + 4 * 1120) * 4
    n0 = N.launch_count()
    p = ctypes.c_void_p(256)   # (a non-null, aligned pointer value the host code never dereferences)
    call = lambda ws, B, W: lib.fz_upcat_bwd(p, p, p, p, 64, p, p, p, ws, p, 64, p, p, B, 32, 64, 2, 2, W, N.STORE_F32, None)   # noqa: E731
    assert call(None, 1, 32) == -4          # FZ_E_ARG: null workspace
    assert call(p, 1, 16) == -2             # FZ_E_UNSUPPORTED: fine W = 32
    assert call(p, 1, 48) == -2             # ... fine W = 96
    assert call(p, 0, 32) == -1             # FZ_E_SHAPE: empty batch
    assert lib.fz_upcat_bwd(p, p, p, p, 64, p, p, p, p, p, 64, p, p, 1, 32, 64, 2, 2, 32, N.STORE_BF16, None) == -2
    assert N.launch_count() == n0
