"""-m gpu: the Deconver family on bf16 activation storage (csrc/deconv_kernels.h with AT = bf16; include/factorizer_hip.h
fz_gcorr_act / fz_gcorr_wgrad_act / fz_gcorr_mu_bwd): activations and their gradients are STORED as bf16, the filters, the
filter gradients, the lag correlations and every accumulator are fp32.

Conventions of tests/test_gpu_bf16.py: the reference is ATen / float64 on the CPU — never the project's own composed path —
evaluated on the SAME bf16-rounded inputs; bounds are n · u · max|ref| with u = 2^-8 and n the number of stored tensors between
the inputs and the result, counted in each test.  Where several stores are chained (the layer), the reference is the
restatement tests/deconv_bf16_ref.py with the same storage roundings inserted, and its distance to plain fp32 is recorded."""
import warnings

import pytest
import torch
from torch import nn

import deconv_bf16_ref as R
import factorizer_amd as ft
import parity as P
from factorizer_amd import _native, composed
from factorizer_amd import functional as Fn

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BF = torch.bfloat16
U = R.U


def close(what, got, ref, n_stores):
    """max|got − ref| ≤ n_stores · u · max|ref|"""
    assert got.dtype in (BF, torch.float32)
    return P.close(what, got.float(), ref, rel=n_stores * U, floor=1e-6,
                   why=f"bf16 storage: {n_stores} stored tensor(s) x u = 2^-8 between input and this result")


# ------------------------------------------------------------------ 1. the operators ------------------------------------
OPS = [
    ((3, 3, 3), 4, 1, 1, (5, 6, 7), False),      # odd W: rows off 4-byte alignment, every extent below the tile
    ((3, 3, 3), 2, 3, 4, (4, 4, 66), True),      # a ragged second W tile, per-sample filters
    ((5, 5, 5), 1, 2, 16, (5, 6, 20), False),
    ((7, 7), 8, 1, 1, (9, 70), False),           # 2-D depthwise k = 7: the FIVES form
    ((5, 3, 3), 1, 8, 8, (6, 6, 8), False),      # run-time-extent kernels: anisotropic
    ((3, 3, 3), 2, 4, 20, (4, 6, 36), False),    # ... and more than 16 output channels per group
]


@pytest.mark.parametrize("ks,G,Ci,Co,S,batched", OPS)
def test_grouped_correlation_on_bf16_storage(ks, G, Ci, Co, S, batched):
    """forward, input gradient and fused update at 1 u (one store each: the output), the fp32 filter gradient of operands that
    are exact in bf16 against float64 at the fp32 bound; 4 launches as on fp32; repeated filter gradient bit-identical."""
    torch.manual_seed(sum(ks) * 11 + Co)
    B = 2
    x = R.rb(torch.rand(B, G * Ci, *S))
    w = torch.rand(B if batched else 1, G, Co, Ci, *ks) / (Ci * float(torch.tensor(ks).prod())) ** 0.5
    xc, wc = x.clone().requires_grad_(True), w.clone().requires_grad_(True)
    yc = R.corr(xc, wc)
    gy = R.rb(torch.rand_like(yc))
    (gxc,) = torch.autograd.grad(yc, xc, gy)
    x64, w64 = x.double(), w.double().requires_grad_(True)
    (gw64,) = torch.autograd.grad(R.corr(x64, w64), w64, gy.double())
    xd, wd = x.to(DEV, BF).requires_grad_(True), w.to(DEV).requires_grad_(True)
    assert Fn.gcorr_supported(xd, wd)
    n0 = _native.launch_count()
    yd = Fn.gcorr(xd, wd, 0.0)
    gxd, gwd = torch.autograd.grad(yd, [xd, wd], gy.to(DEV, BF))
    assert _native.launch_count() - n0 == 4          # forward, input gradient, filter gradient (sweep + finish)
    assert yd.dtype == BF and gxd.dtype == BF and gwd.dtype == torch.float32
    close("y", yd, yc, 1)
    close("gx", gxd, gxc, 1)
    P.close("gw (fp32 sums of products of bf16-exact operands)", gwd, gw64.float())
    gwd2 = torch.autograd.grad(Fn.gcorr(xd, wd, 0.0), wd, gy.to(DEV, BF))[0]
    assert torch.equal(gwd, gwd2)
    a, b = R.rb(torch.rand_like(yc)), R.rb(torch.rand_like(yc))
    fused = Fn.gcorr_mu_update(a.to(DEV, BF), b.to(DEV, BF), xd.detach(), wd.detach(), 1e-3)
    assert fused.dtype == BF
    close("fused a*b/(corr+eps): computed in fp32, rounded once", fused, a * b / (yc.detach() + 1e-3), 1)


def test_lag_correlation_on_bf16_storage():
    """Fn.lag_corr on bf16 operands: fp32 result against float64 at the fp32 bound, both gradients (bf16) at 1 u"""
    torch.manual_seed(5)
    B, G, K, C, S, ks = 2, 2, 3, 4, (5, 6, 70), (3, 3, 3)
    s, x = R.rb(torch.rand(B, G * K, *S)), R.rb(torch.rand(B, G * C, *S))
    sc, xc = s.double().requires_grad_(True), x.double().requires_grad_(True)
    Lc = R.lag_corr(sc, xc, G, ks)
    gL = torch.rand(Lc.shape)
    gsc, gxc = torch.autograd.grad(Lc, [sc, xc], gL.double())
    sd, xd = s.to(DEV, BF).requires_grad_(True), x.to(DEV, BF).requires_grad_(True)
    assert Fn.lag_corr_supported(sd, xd, G, ks)
    Ld = Fn.lag_corr(sd, xd, G, ks)
    gsd, gxd = torch.autograd.grad(Ld, [sd, xd], gL.to(DEV))
    assert Ld.dtype == torch.float32 and gsd.dtype == BF and gxd.dtype == BF
    P.close("L", Ld, Lc.float())
    close("gs", gsd, gsc.float(), 1)
    close("gx", gxd, gxc.float(), 1)


# ------------------------------------------------------------------ 2. the update node ----------------------------------
MU = [(2, 4, 1, 1, (3, 3, 3), (5, 6, 7)), (2, 2, 2, 3, (7, 7), (9, 70))]      # B, G, K, C, kernel, S


def _mu_case(B, G, K, C, ks, S, seed):
    """s, num (B, G·K, *S), r (B, G·C, *S) from U(0.5, 1.5); wT (1, G, K, C, *k) positive with unit sum per output channel:
    den = corr(r, wT) + eps stays inside [0.5 · (interior fraction), 1.5] and every partial derivative is O(1)"""
    torch.manual_seed(seed)
    s, num = torch.rand(B, G * K, *S) + 0.5, torch.rand(B, G * K, *S) + 0.5
    r = torch.rand(B, G * C, *S) + 0.5
    wT = torch.rand(1, G, K, C, *ks) + 0.1
    wT = wT / wT.sum(dim=tuple(range(3, wT.ndim)), keepdim=True)
    g = torch.rand(B, G * K, *S) - 0.5
    return s, num, r, wT, g


def _mu_ref64(s, num, r, wT, g, eps, need_num=True):
    t = [v.double().requires_grad_(True) for v in (s, num, r, wT)]
    y = R.mu_update(*t, eps)
    wrt = [t[0], t[2], t[3]] + ([t[1]] if need_num else [])
    return y, torch.autograd.grad(y, wrt, g.double())


@pytest.mark.parametrize("B,G,K,C,ks,S", MU)
@pytest.mark.parametrize("need_num", [True, False])
def test_mu_update_node_fp32_against_float64(B, G, K, C, ks, S, need_num):
    """GCorrMuFn on fp32: forward, ds, dnum, dr, dwT against float64 autograd of s * num / (corr(r, wT) + eps) at the fp32
    bound; with `need_num` false the dnum pointer of the backward launch is null."""
    eps = 1e-16
    s, num, r, wT, g = _mu_case(B, G, K, C, ks, S, 21)
    y64, g64 = _mu_ref64(s, num, r, wT, g, eps, need_num)
    sd, rd, wd = (v.to(DEV).requires_grad_(True) for v in (s, r, wT))
    nd_ = num.to(DEV).requires_grad_(need_num)
    n0 = _native.launch_count()
    yd = Fn.gcorr_mu_update_graded(sd, nd_, rd, wd, eps)
    assert _native.launch_count() - n0 == 1
    got = torch.autograd.grad(yd, [sd, rd, wd] + ([nd_] if need_num else []), g.to(DEV))
    assert _native.launch_count() - n0 == 5          # update; its backward; dr; dwT (sweep + finish)
    P.close("s'", yd, y64.float())
    for k, a, b in zip(("ds", "dr", "dwT", "dnum"), got, g64):
        P.close(k, a, b.float())


@pytest.mark.parametrize("B,G,K,C,ks,S", MU)
def test_mu_update_node_on_bf16_storage(B, G, K, C, ks, S):
    """the same draws rounded to bf16: forward, ds, dnum one store each; dr two (dden, then the correlation's output); dwT is
    fp32 but reads the stored dden: one."""
    eps = 1e-16
    s, num, r, wT, g = _mu_case(B, G, K, C, ks, S, 22)
    s, num, r, g = (R.rb(v) for v in (s, num, r, g))
    y64, (ds, dr, dw, dnum) = _mu_ref64(s, num, r, wT, g, eps)
    sd, nd_, rd = (v.to(DEV, BF).requires_grad_(True) for v in (s, num, r))
    wd = wT.to(DEV).requires_grad_(True)
    yd = Fn.gcorr_mu_update_graded(sd, nd_, rd, wd, eps)
    gs, gn, gr, gw = torch.autograd.grad(yd, [sd, nd_, rd, wd], g.to(DEV, BF))
    assert yd.dtype == BF and gs.dtype == BF and gn.dtype == BF and gr.dtype == BF and gw.dtype == torch.float32
    close("s'", yd, y64.float(), 1)
    close("ds", gs, ds.float(), 1)
    close("dnum", gn, dnum.float(), 1)
    close("dr", gr, dr.float(), 2)
    close("dwT", gw, dw.float(), 1)


# ------------------------------------------------------------------ 3. the layer ----------------------------------------
LAYERS = {
    "recipe_dw_k3": dict(channels=8, groups=-1, ratio=1, kernel_size=(3, 3, 3), num_iters=1),
    "g2_r2_grad1": dict(channels=8, groups=2, ratio=2, kernel_size=(3, 3, 3), num_iters=2, num_grad_iters=1),
}


def _layer(cfg):
    torch.manual_seed(0)
    m = ft.Deconv(**cfg)
    with torch.no_grad():
        m.init.linear.linear.bias.add_(0.5)      # most sources start positive
    return m


def _layer_ref(m, x, store):
    lin = m.init.linear.linear
    return R.deconv_forward(x, lin.weight, lin.bias, m.init.h0, m.groups, m.kernel_size, m.num_iters, m.num_grad_iters,
                            m.eps, m.update_filter, store)


@pytest.mark.parametrize("tag", sorted(LAYERS))
def test_deconv_layer_on_bf16_input(tag):
    """ft.Deconv on a bf16 device input, no framework fallback (a RuntimeWarning is an error), against the restatement with
    the storage roundings.  Stored between x and the sources: s0, num, and r, s' per iteration: n_fwd = 2 + 2 · num_iters.
    Gradients: autograd through the restatement (rounding as a straight-through op); the device additionally stores, with all
    iterations carrying gradient, ds, dnum, dden, dr, the source gradient of H, the accumulated source gradient, the two input
    gradients (linear, Hᵀ) and their sum — 9 for dx, 3 (dnum, dden, dr) for dh0, 5 (ds, dden, dr, gs, their sum) for the
    linear weight; when the sources enter the last iteration detached only dnum and the input gradient of Hᵀ remain for dx."""
    m = _layer(LAYERS[tag])
    torch.manual_seed(4)
    x = R.rb(torch.rand(2, 8, 6, 6, 10))
    xr = x.clone().requires_grad_(True)
    yr = _layer_ref(m, xr, R.store_bf16)
    with torch.no_grad():
        plain = _layer_ref(m, x, R.store_none)
    gy = R.rb(torch.rand_like(yr))
    params = [m.init.h0, m.init.linear.linear.weight]
    ref = torch.autograd.grad(yr, [xr] + params, gy, allow_unused=True)
    md = _layer(LAYERS[tag]).to(DEV)
    pd = [md.init.h0, md.init.linear.linear.weight]
    xd = x.to(DEV, BF).requires_grad_(True)
    composed._warned.clear()
    n0 = _native.launch_count()
    with warnings.catch_warnings():
        warnings.simplefilter("error", RuntimeWarning)
        yd = md(xd)
        got = torch.autograd.grad(yd, [xd] + pd, gy.to(DEV, BF), allow_unused=True)
    assert _native.launch_count() > n0 and yd.dtype == BF
    n_fwd = 2 + 2 * m.num_iters
    P.note(f"deconv layer {tag}: restatement with bf16 stores against plain fp32",
           rel_err=((yr.detach() - plain).abs().max() / plain.abs().max()).item(), n_fwd=n_fwd)
    assert float(yr.detach().max()) > 0
    close("sources", yd, yr.detach(), n_fwd)
    full = m.num_grad_iters == m.num_iters
    for k, a, b, n_bwd in zip(("dx", "dh0", "dlinear.weight"), got, ref, (9 if full else 2, 3, 5)):
        if b is None:
            assert a is None and not full
            continue
        assert a.dtype == (BF if k == "dx" else torch.float32)
        close(k, a, b, n_fwd + n_bwd)


def test_deconv_filter_update_is_native_on_bf16():
    """update_filter=True on a bf16 input: lag correlations and the grouped correlations with per-sample filters run native
    (no warning), the result is the restatement's (filters and ratio fp32 throughout)."""
    cfg = dict(channels=8, groups=2, ratio=1, kernel_size=(3, 3, 3), num_iters=2, update_filter=True)
    m = _layer(cfg)
    torch.manual_seed(6)
    x = R.rb(torch.rand(2, 8, 6, 6, 10))
    with torch.no_grad():
        yr = _layer_ref(m, x, R.store_bf16)
    assert float(yr.max()) > 0
    md = _layer(cfg).to(DEV)
    composed._warned.clear()
    n0 = _native.launch_count()
    with warnings.catch_warnings(), torch.no_grad():
        warnings.simplefilter("error", RuntimeWarning)
        yd = md(x.to(DEV, BF))
    # per iteration: Hᵀx, H s, the fused update, 2 lag correlations (sweep + finish each) and the H s they read: 8; + the linear
    assert _native.launch_count() - n0 >= 2 * 8 + 1
    assert yd.dtype == BF
    # stored: s0; num, r, s' of each iteration (the filters move, so num is formed twice): 7.  The first filter update reads one
    # more stored tensor, H s; its relative error (<= u) passes into h, and h enters the next update three times (Hᵀx once,
    # HᵀH s twice): 3 more.
    close("sources after two source + filter updates", yd, yr, 7 + 3)


# ------------------------------------------------------------------ 4. the network --------------------------------------
def _net(nd, **kw):
    torch.manual_seed(0)
    return ft.Deconver(in_channels=2, out_channels=3, spatial_dims=nd, encoder_width=(8, 16), encoder_depth=(1, 1),
                       strides=(1, 2), decoder_depth=(1,), act=nn.ReLU, groups=-1, ratio=1, kernel_size=(3,) * nd, num_iters=2,
                       mlp_ratio=2, dropout=0.0, **kw).to(DEV)


def test_deconver_under_bf16_autocast():
    """ft.Deconver (3-D, widths (8, 16), one down-sampling, 16^3) under torch.autocast("cuda", bfloat16): forward and backward
    without a RuntimeWarning, native launches, bf16 finite output, fp32 finite parameter gradients, bit-identical when repeated.
    The distance to the fp32 run is recorded, not asserted: no bound for a whole network can be derived."""
    model = _net(3)
    torch.manual_seed(8)
    x = torch.rand(1, 2, 16, 16, 16, device=DEV)
    gy = torch.rand(1, 3, 16, 16, 16, device=DEV)

    def run():
        composed._warned.clear()
        with warnings.catch_warnings(), torch.autocast("cuda", dtype=BF):
            warnings.simplefilter("error", RuntimeWarning)
            y = model(x)
            grads = torch.autograd.grad(y, list(model.parameters()), gy.to(y.dtype), allow_unused=True)
        return y, grads

    n0 = _native.launch_count()
    y1, g1 = run()
    assert _native.launch_count() > n0
    y2, g2 = run()
    assert y1.dtype == BF and torch.isfinite(y1.float()).all()
    assert torch.equal(y1, y2)
    for (k, _), a, b in zip(model.named_parameters(), g1, g2):
        assert a is not None or "deconv" not in k, k
        if a is None:
            continue
        assert a.dtype == torch.float32 and torch.isfinite(a).all(), k
        assert torch.equal(a, b), k
    with torch.no_grad():
        y32 = model(x)
    P.note("deconver 3-D under bf16 autocast against its fp32 run",
           rel_l2=((y1.float() - y32).norm() / y32.norm()).item())
    # the same forward on a bf16 input without autocast
    composed._warned.clear()
    with warnings.catch_warnings(), torch.no_grad():
        warnings.simplefilter("error", RuntimeWarning)
        y3 = model(x.to(BF))
    assert y3.dtype == BF and torch.isfinite(y3.float()).all()


def test_deconver_2d_with_framework_instance_norm_under_bf16_autocast():
    """norm=nn.InstanceNorm2d: the framework norm, whatever type it hands back, must not break the mixer"""
    model = _net(2, norm=nn.InstanceNorm2d)
    torch.manual_seed(9)
    x = torch.rand(2, 2, 16, 24, device=DEV)
    n0 = _native.launch_count()
    with torch.autocast("cuda", dtype=BF):
        y = model(x)
        grads = torch.autograd.grad(y.float().sum(), list(model.parameters()), allow_unused=True)
    assert _native.launch_count() > n0
    assert torch.isfinite(y.float()).all()
    assert all(g is None or (g.dtype == torch.float32 and torch.isfinite(g).all()) for g in grads)
