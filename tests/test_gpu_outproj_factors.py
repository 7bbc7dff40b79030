"""-m gpu: the out-projection of the C = 32 block on the core's rank-1 factors (csrc/outproj_fac.h; the factor forms of
gemm_chain_kernel, csrc/mlp_chain32.hip, and gemm_dw_kernel, csrc/gemm_dw.hip; fz_nmf_cf_factors_to_tensor, csrc/nmf_cf_fwd.hip).
The contract is bits: the core's output a rebuilt from the factors of both windows is the a that the launch pair
fz_nmf_cf_fwd_store_factors + fz_nmf_cf_fwd_from_factors stores, so everything behind it is torch.equal to the stored-tensor path.
Grids: one 64-voxel run per W row, and two runs per row with the shifted windows wrapping across the W boundary; shifts: a plain
and a shifted window, and the shifted-first-window pair of tests/test_gpu_cf_factors.py; T = 5 and 1; t >= 0 with all-zero patches."""
import pytest
import torch
from torch import nn

import factorizer_amd as ft
from factorizer_amd import _native as N
from factorizer_amd import functional as Fn
from factorizer_amd import pointwise as PW
from oracle import cpu_ref as O
import parity as P

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
C, HD = 32, 64

GRIDS = [(1, (8, 8, 64)), (2, (16, 8, 128))]
SHIFT_PAIRS = [[None, (4, 4, 4)], [(4, 4, 0), (0, 4, 4)]]
CASES = [pytest.param(B, S, sh, id=f"{B}x{'x'.join(map(str, S))}-{i}") for B, S in GRIDS for i, sh in zip(("w1_444", "w0_440_w1_044"), SHIFT_PAIRS)]


def _bits(t):
    return t.contiguous().view(torch.int32)


def _same(a, b):
    """bit patterns, not values: torch.equal would let +0 pass for -0"""
    return a.shape == b.shape and torch.equal(_bits(a), _bits(b))


def _input(B, S):
    """ReLU'd normals with all-zero patches (of the plain and of the shifted windows' tiling) and an all-zero channel"""
    torch.manual_seed(5)
    t = torch.relu(torch.randn(B, C, *S))
    t[0, :8, :8, :8, :8] = 0
    t[-1, 8:16, :, :, 20:36] = 0
    t[-1, 19] = 0
    return t.to(DEV)


def _geo(S, shifts):
    return ft.SWMatricize((None, C, *S), head_dim=8, patch_size=8, shifts=shifts).geometry


def _init(T):
    nmf = ft.NMF(size=(8, 512), rank=1, num_iters=T, init="uniform", solver="hals")
    return nmf.init.u0.to(DEV), nmf.init.v0.to(DEV)


_CORE = {}


def _core(B, S, shifts, T):
    """(geometry, the factors of both windows, a as the core's launch pair stores it) — computed once, shared, left unchanged"""
    k = (B, S, str(shifts), T)
    if k not in _CORE:
        geo, t = _geo(S, shifts), _input(B, S)
        u0, v0 = _init(T)
        assert Fn.nmf_cf_factors_supported(geo, 1, T, T)
        with torch.no_grad():
            a = Fn.FactCoreFn.apply(t, u0, v0, geo, T, T, "hals", 1e-16, True)
        fac = Fn.core_factors(t, u0, v0, geo, T, "hals", 1e-16)
        torch.cuda.synchronize()
        assert torch.isfinite(a).all() and a.abs().max() > 0
        _CORE[k] = (geo, fac, a)
    return _CORE[k]


def _weights():
    g = torch.Generator().manual_seed(11)
    r = lambda *s, k=1.0: (torch.randn(*s, generator=g) * k).to(DEV)   # noqa: E731
    return dict(wout=r(C, C, k=0.2), bout=r(C, k=0.1), ln_w=1 + r(C, k=0.1), ln_b=r(C, k=0.1), w1=r(HD, C, k=0.2), b1=r(HD, k=0.1),
                w2=r(C, HD, k=0.2), b2=r(C, k=0.1), hw=r(3, C, k=0.2), hb=r(3, k=0.1))


@pytest.mark.parametrize("B,S,shifts", CASES)
@pytest.mark.parametrize("T", [5, 1])
def test_factors_to_tensor_is_the_stored_output_bitwise(B, S, shifts, T):
    geo, fac, a = _core(B, S, shifts, T)
    got = Fn.factors_to_tensor(fac, geo, a)
    torch.cuda.synchronize()
    assert _same(got, a), int((_bits(got) != _bits(a)).sum())


@pytest.mark.parametrize("B,S,shifts", CASES)
@pytest.mark.parametrize("T", [5, 1])
def test_chain_on_factors_equals_chain_on_the_tensor_bitwise(B, S, shifts, T):
    geo, fac, a = _core(B, S, shifts, T)
    w = _weights()
    torch.manual_seed(3)
    x = torch.randn(B, C, *S, device=DEV)
    args = (w["wout"], w["bout"], x, w["ln_w"], w["ln_b"], 1e-5, w["w1"], w["b1"], w["w2"], w["b2"])
    for head in (None, (w["hw"], w["hb"])):
        ref = PW._outproj_mlp_fwd_chain(a, *args, head=head)
        got = PW._outproj_mlp_fwd_chain(None, *args, head=head, fac=(fac, geo))
        torch.cuda.synchronize()
        assert len(got) == len(ref) == (4 if head is None else 5)
        for name, g, r in zip(("x1", "x2", "z1", "stats", "logits"), got, ref):
            assert torch.isfinite(r).all()
            assert _same(g, r), (name, int((_bits(g) != _bits(r)).sum()))


@pytest.mark.parametrize("B,S,shifts", CASES)
@pytest.mark.parametrize("T", [5, 1])
def test_gemm_dw_on_factors_equals_gemm_dw_on_the_tensor_bitwise(B, S, shifts, T):
    geo, fac, a = _core(B, S, shifts, T)
    w = _weights()
    torch.manual_seed(4)
    g = torch.randn(B, C, *S, device=DEV)
    yr, gwr, gbr, _, _ = PW._gemm_dw(g, w["wout"], a, want_bias=True)
    yg, gwg, gbg, _, _ = PW._gemm_dw(g, w["wout"], None, want_bias=True, fac=(fac, geo))
    torch.cuda.synchronize()
    for name, got, ref in (("y", yg, yr), ("gw", gwg, gwr), ("gb", gbg, gbr)):
        assert torch.isfinite(ref).all() and ref.abs().max() > 0
        assert _same(got, ref), (name, int((_bits(got) != _bits(ref)).sum()))


# ---------------------------------------------------------------- the block ------------------------------------------------
class _Launches:
    """functional.set_timer hook: (timer key, algorithmic bytes) of every timed launch"""

    def __init__(self):
        self.calls = []

    def launch(self, name, nbytes, fn, cols, flops):
        self.calls.append((name, nbytes))
        return fn()


def _block(Cb, S, shifts, T=5, rank=1, mlp_ratio=2, dropout=0.0):
    torch.manual_seed(0)
    blk = ft.FactorizerBlock(channels=Cb, spatial_size=S, norm=ft.LayerNorm, reshape=(ft.SWMatricize, dict(head_dim=8, patch_size=8, shifts=shifts)),
                             act=nn.ReLU, factorize=ft.NMF, init="uniform", mlp_ratio=mlp_ratio, dropout=dropout, rank=rank, num_iters=T,
                             solver="hals")
    with torch.no_grad():      # biases and LayerNorm affines away from their initial 0 / 1
        for p in blk.parameters():
            if p.dim() == 1:
                p.add_(0.1 * torch.randn_like(p))
    return blk


def _run(blk, x, gy, dtype=torch.float32):
    """one forward + backward: (outputs and gradients, the launches)"""
    rec = _Launches()
    blk.zero_grad(set_to_none=True)
    xd = x.to(dtype).requires_grad_(True)
    torch.manual_seed(9)       # (the dropout seed draw of a training-mode block)
    Fn.set_timer(rec)
    try:
        y = blk(xd)
        y.backward(gy.to(dtype))
    finally:
        Fn.set_timer(None)
    torch.cuda.synchronize()
    out = {"y": y.detach(), "gx": xd.grad.detach(), **{k: p.grad.detach().clone() for k, p in blk.named_parameters()}}
    return out, rec.calls


@pytest.mark.parametrize("B,S,shifts", CASES)
@pytest.mark.parametrize("T", [5, 1])
def test_block_switch_on_equals_switch_off_bitwise(B, S, shifts, T, monkeypatch):
    blk = _block(C, S, shifts, T=T).to(DEV)
    torch.manual_seed(1)
    x, gy = torch.rand(B, C, *S, device=DEV), torch.randn(B, C, *S, device=DEV)
    on, calls_on = _run(blk, x, gy)
    again, calls_again = _run(blk, x, gy)
    monkeypatch.setattr(Fn, "_OUTPROJ_FACTORS", False)
    off, calls_off = _run(blk, x, gy)
    nb = x.numel() * 4
    V = x.numel() // C
    sp = "x".join(str(v) for v in (C, *S))
    # the factor path ran: both core windows are store-factors launches, both consumers declare the v fields in place of a
    core_on = [b for k, b in calls_on if k == f"nmf_cf_fwd_{sp}"]
    core_off = [b for k, b in calls_off if k == f"nmf_cf_fwd_{sp}"]
    assert core_on[:2] == [nb + nb // 8] * 2 and core_off[:2] == [nb + nb // 8, 2 * nb + nb // 8]
    by = lambda calls, key: [b for k, b in calls if k == key][0]      # noqa: E731
    assert by(calls_off, "outproj_mlp_chain_fwd_32") - by(calls_on, "outproj_mlp_chain_fwd_32") == nb - nb // 4
    assert by(calls_off, "dgrad_wgrad_32") - by(calls_on, "dgrad_wgrad_32") == nb - nb // 4
    assert [k for k, _ in calls_on] == [k for k, _ in calls_off]      # the same launches under the same timer keys
    assert V % 64 == 0
    assert set(on) == set(off) and len(on) > 10
    for k in on:
        assert torch.isfinite(off[k]).all()
        assert _same(on[k], off[k]), (k, int((_bits(on[k]) != _bits(off[k])).sum()))
        assert _same(on[k], again[k]), ("replay", k)                   # two runs replay bit for bit
    assert calls_on == calls_again


def test_block_on_factors_vs_float64():
    """the factor path against the CPU oracle's restatement of the reference block in float64, at the suite's 1e-4"""
    B, S, shifts = 1, (8, 8, 64), [None, (4, 4, 4)]
    blk = _block(C, S, shifts)
    sd = {k: v.clone().double() for k, v in blk.state_dict().items()}
    torch.manual_seed(2)
    x, gy = torch.rand(B, C, *S), torch.rand(B, C, *S)
    xo = x.double().requires_grad_(True)
    yo = O.factorizer_block(xo, sd, "", dict(reshape=dict(head_dim=8, patch_size=8, shifts=shifts), num_iters=5, solver="hals"))
    (gxo,) = torch.autograd.grad(yo, xo, gy.double())
    assert yo.dtype == torch.float64
    blk = blk.to(DEV)
    got, calls = _run(blk, x.to(DEV), gy.to(DEV))
    nb = x.numel() * 4
    assert [b for k, b in calls if k.startswith("nmf_cf_fwd_")][:2] == [nb + nb // 8] * 2      # the factor path
    P.close("block on factors: y vs float64", got["y"], yo)
    P.close("block on factors: gx vs float64", got["gx"], gxo)


EXCLUDED = {
    # what the issue leaves to today's launches: stage 1 (C = 64), bf16 storage, rank 2, four windows, hidden 128, live dropout,
    # a W that the core's factor windows do not take, a W-axis shift of 2
    "C64": dict(Cb=64, S=(8, 8, 64), shifts=[None, (4, 4, 4)]),
    "bf16": dict(Cb=32, S=(8, 8, 64), shifts=[None, (4, 4, 4)], dtype=torch.bfloat16),
    "rank2": dict(Cb=32, S=(8, 8, 64), shifts=[None, (4, 4, 4)], rank=2),
    "four_windows": dict(Cb=32, S=(8, 8, 64), shifts=[None, 2, 4, 6]),
    "hidden128": dict(Cb=32, S=(8, 8, 64), shifts=[None, (4, 4, 4)], mlp_ratio=4),
    "dropout": dict(Cb=32, S=(8, 8, 64), shifts=[None, (4, 4, 4)], dropout=0.1),
    "W32": dict(Cb=32, S=(8, 8, 32), shifts=[None, (4, 4, 4)]),
    "wshift2": dict(Cb=32, S=(8, 8, 64), shifts=[None, (4, 4, 2)]),
}


@pytest.mark.parametrize("name", sorted(EXCLUDED))
def test_excluded_configurations_run_todays_launches(name, monkeypatch):
    kw = dict(EXCLUDED[name])
    dtype = kw.pop("dtype", torch.float32)
    blk = _block(**kw).to(DEV)
    blk.train(kw.get("dropout", 0.0) > 0)
    torch.manual_seed(1)
    x = torch.rand(1, kw["Cb"], *kw["S"], device=DEV)
    gy = torch.randn_like(x)
    on, calls_on = _run(blk, x, gy, dtype)
    monkeypatch.setattr(Fn, "_OUTPROJ_FACTORS", False)
    off, calls_off = _run(blk, x, gy, dtype)
    assert calls_on == calls_off and len(calls_on) > 4, (calls_on, calls_off)
    assert not any(k == "nmf_cf_factors_to_tensor" for k, _ in calls_on)
    for k in on:
        assert torch.equal(on[k], off[k]), k


def test_unsupported_descriptors_are_refused_on_the_device():
    """with real device buffers behind every pointer: a refused descriptor launches nothing and leaves its outputs alone"""
    B, S, shifts = 1, (8, 8, 64), [None, (4, 4, 4)]
    geo, fac, a = _core(B, S, shifts, 5)
    w = _weights()
    x = torch.randn(B, C, *S, device=DEV)
    g = torch.randn(B, C, *S, device=DEV)
    n0 = N.launch_count()
    with pytest.raises(N.NativeError, match="fz_mlp_chain_fac"):        # a tensor AND factors
        PW._outproj_mlp_fwd_chain(a, w["wout"], w["bout"], x, w["ln_w"], w["ln_b"], 1e-5, w["w1"], w["b1"], w["w2"], w["b2"], fac=(fac, geo))
    with pytest.raises(N.NativeError, match="fz_gemm_dw_fac"):        # the LayerNorm form of fz_gemm_dw
        st = torch.zeros(B, 2, x.numel() // C, device=DEV)
        PW._gemm_dw(g, w["wout"], None, ln=(w["ln_w"], w["ln_b"]), stats=st, fac=(fac, geo))
    with pytest.raises(N.NativeError, match="fz_mlp_chain_fac"):        # fp32-MFMA products
        with N.use_products(N.PRODUCTS_FP32_MFMA):
            PW._outproj_mlp_fwd_chain(None, w["wout"], w["bout"], x, w["ln_w"], w["ln_b"], 1e-5, w["w1"], w["b1"], w["w2"], w["b2"], fac=(fac, geo))
    bad = _geo((8, 16, 64), shifts)                        # factors of another volume: D H W != V
    with pytest.raises(N.NativeError, match="D H W == V"):
        PW._gemm_dw(g, w["wout"], None, want_bias=True, fac=(fac, bad))
    with pytest.raises(N.NativeError, match="fp32 storage"):
        Fn.factors_to_tensor(fac, geo, a.to(torch.bfloat16))
    torch.cuda.synchronize()
    assert N.launch_count() == n0
