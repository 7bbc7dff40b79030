"""-m gpu: the convolutions of a 2-D U-shape (convs.Conv2d / convs.ConvTranspose2d) on the 2-D tap geometries of the GEMM family
(FZ_LOAD_S2D_2D, FZ_LOAD_K3_2D, FZ_EPI_D2S_2D in fz_gemm; FZ_QL_S2D_2D, FZ_QL_K3_2D in fz_wgrad): forward, input, weight and
bias gradients against float64 CPU autograd, in both product modes and with bf16 storage, natively (no RuntimeWarning) and
deterministically; whole 2-D Factorizer / Deconver models against the reference goldens (g10 / g9)."""
import ctypes
import warnings

import pytest
import torch
import torch.nn.functional as F

import factorizer_amd as ft
import parity as P
from factorizer_amd import _native as N
from factorizer_amd import composed, convs
from factorizer_amd import functional as Fn
from factorizer_amd import pointwise as PW

from test_deconver_cpu import MODELS
from test_modules_cpu import lower_d_model

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAMES = {"k3": ("conv2d_k3", "wgrad_conv2d_k3"), "k2s2": ("conv2d_k2s2", "wgrad_conv2d_k2s2"),
         "t2": ("tconv2d_k2s2", "wgrad_tconv2d_k2s2"), "k1": ("act_linear_res",)}


def _layer(kind, cin, cout, bias=True):
    if kind == "t2":
        return convs.ConvTranspose2d(cin, cout, kernel_size=2, stride=2, bias=bias)
    k, s, p = {"k3": (3, 1, 1), "k2s2": (2, 2, 0), "k1": (1, 1, 0)}[kind]
    return convs.Conv2d(cin, cout, kernel_size=k, stride=s, padding=p, bias=bias)


def _ref64(m, x, gy):
    """float64 CPU autograd of the framework convolution"""
    x64 = x.detach().double().cpu().requires_grad_(True)
    w64 = m.weight.detach().double().cpu().requires_grad_(True)
    b64 = None if m.bias is None else m.bias.detach().double().cpu().requires_grad_(True)
    if isinstance(m, torch.nn.ConvTranspose2d):
        y = F.conv_transpose2d(x64, w64, b64, stride=2)
    else:
        y = F.conv2d(x64, w64, b64, stride=m.stride, padding=m.padding)
    ins = [x64, w64] + ([b64] if b64 is not None else [])
    return [y] + list(torch.autograd.grad(y, ins, gy.double().cpu()))


def _run(m, x, gy):
    xd = x.to(DEV).requires_grad_(True)
    y = m(xd)
    grads = torch.autograd.grad(y, [xd] + list(m.parameters()), gy.to(DEV).to(y.dtype))
    return [y] + list(grads)


def _case(kind, cin, cout, B, hw, products, seed=0):
    torch.manual_seed(seed)
    m = _layer(kind, cin, cout, bias=(kind != "k3" or cout != 32))
    H, W = hw
    x = torch.randn(B, cin, H, W)
    oh, ow = {"k2s2": (H // 2, W // 2), "t2": (2 * H, 2 * W)}.get(kind, (H, W))
    gy = torch.randn(B, cout, oh, ow)
    ref = _ref64(m, x, gy)
    m = m.to(DEV)
    timer = Fn.KernelTimer()
    Fn.set_timer(timer)
    composed._warned.clear()
    n0 = N.launch_count()
    try:
        with warnings.catch_warnings(), N.use_products(products):
            warnings.simplefilter("error", RuntimeWarning)
            got = _run(m, x, gy)
    finally:
        Fn.set_timer(None)
    ran = timer.summary()
    assert N.launch_count() > n0
    for name in NAMES[kind]:
        assert any(k.startswith(name + "_") for k in ran), (name, sorted(ran))
    for what, a, r in zip(["y", "dx", "dW", "db"], got, ref):
        P.close(f"{kind} {cin}->{cout} {what}", a, r)
    return m, x, gy, ref


CASES = ([("k3", ci, co, B, hw) for ci in (3, 4, 32) for co in (16, 32) for B, hw in ((1, (16, 16)), (2, (8, 12)))]
         + [("k2s2", c, 2 * c if c < 256 else c, B, hw) for c in (32, 64, 256) for B, hw in ((1, (16, 16)), (2, (8, 24)))]
         + [("t2", c, c // 2, B, hw) for c in (32, 64, 256) for B, hw in ((1, (8, 8)), (2, (4, 12)))]
         + [("k1", 32, o, B, hw) for o in (1, 3) for B, hw in ((1, (16, 16)), (2, (8, 12)))])
PRODUCTS = {"split_bf16": N.PRODUCTS_SPLIT_BF16, "fp32_mfma": N.PRODUCTS_FP32_MFMA}


@pytest.mark.parametrize("products", sorted(PRODUCTS))
@pytest.mark.parametrize("kind,cin,cout,B,hw", CASES)
def test_layer_parity_against_float64(kind, cin, cout, B, hw, products):
    _case(kind, cin, cout, B, hw, PRODUCTS[products])


@pytest.mark.parametrize("products", sorted(PRODUCTS))
@pytest.mark.parametrize("kind,cin,cout", [("k3", 3, 32), ("k2s2", 32, 64)])
def test_fives_sized_layers(kind, cin, cout, products):
    """the FIVES model's stem (3 -> 32) and first down-sampling (32 -> 64) at 512^2, B = 1"""
    _case(kind, cin, cout, 1, (512, 512), PRODUCTS[products])


@pytest.mark.parametrize("kind,cin,cout,hw", [("k3", 3, 32, (16, 16)), ("k3", 32, 16, (8, 12)), ("k2s2", 32, 64, (16, 16)),
                                              ("t2", 64, 32, (8, 8)), ("k1", 32, 3, (16, 16))])
def test_bf16_activation_storage(kind, cin, cout, hw):
    torch.manual_seed(4)
    m = _layer(kind, cin, cout)
    x = torch.randn(2, cin, *hw).bfloat16().float()
    oh, ow = {"k2s2": (hw[0] // 2, hw[1] // 2), "t2": (2 * hw[0], 2 * hw[1])}.get(kind, hw)
    gy = torch.randn(2, cout, oh, ow).bfloat16().float()
    ref = _ref64(m, x, gy)
    m = m.to(DEV)
    composed._warned.clear()
    with warnings.catch_warnings():
        warnings.simplefilter("error", RuntimeWarning)
        xd = x.to(DEV).bfloat16().requires_grad_(True)
        y = m(xd)
        assert y.dtype == torch.bfloat16
        got = [y] + list(torch.autograd.grad(y, [xd] + list(m.parameters()), gy.to(DEV).bfloat16()))
    why = "bf16 activation storage: outputs / input gradients are rounded to 8 significand bits once, the weight gradients take bf16 MFMA products"
    for what, a, r in zip(["y", "dx", "dW", "db"], got, ref):
        P.close(f"bf16 {kind} {what}", a, r, rel=3 * 2.0 ** -8, why=why)


@pytest.mark.parametrize("kind,cin,cout,hw", [("k3", 3, 16, (16, 16)), ("k2s2", 32, 64, (16, 16)), ("t2", 64, 32, (8, 8))])
def test_backward_is_deterministic(kind, cin, cout, hw):
    torch.manual_seed(5)
    m = _layer(kind, cin, cout).to(DEV)
    x = torch.randn(2, cin, *hw, device=DEV).requires_grad_(True)
    y = m(x)
    gy = torch.randn_like(y)
    g1 = torch.autograd.grad(y, [x] + list(m.parameters()), gy, retain_graph=True)
    g2 = torch.autograd.grad(y, [x] + list(m.parameters()), gy)
    for a, b in zip(g1, g2):
        assert torch.equal(a, b)


def test_skip_fork_adds_the_skip_gradient_in_the_epilogue():
    torch.manual_seed(6)
    m = _layer("k2s2", 32, 64)
    x = torch.randn(2, 32, 16, 16)
    gs, gy = torch.randn(2, 32, 16, 16), torch.randn(2, 64, 8, 8)
    ref = _ref64(m, x, gy)
    m = m.to(DEV)
    xd = x.to(DEV).requires_grad_(True)
    skip, y = m.forward_fork(xd)
    assert type(y.grad_fn).__name__.startswith("SkipConvK2S2Fn")
    (gx,) = torch.autograd.grad([skip, y], [xd], [gs.to(DEV), gy.to(DEV)])
    P.close("fork dx", gx, ref[1] + gs.double())
    P.close("fork y", y, ref[0])


def test_out_of_gate_shape_warns_once_and_matches_torch():
    torch.manual_seed(7)
    m = _layer("k3", 4, 8).to(DEV)
    x = torch.randn(1, 4, 10, 10, device=DEV)                       # W % 4 != 0
    composed._warned.clear()
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        y1 = m(x)
        y2 = m(x)
    hits = [r for r in rec if issubclass(r.category, RuntimeWarning) and "Conv2d" in str(r.message)]
    assert len(hits) == 1, [str(r.message) for r in rec]
    assert torch.equal(y1, F.conv2d(x, m.weight, m.bias, padding=1)) and torch.equal(y1, y2)


def _deconver2d():
    return ft.Deconver(in_channels=4, out_channels=3, **MODELS["model2d"])


def test_whole_models_run_every_ushape_conv_natively(golden):
    checks = []
    g9 = golden("g9_deconver")
    d = _deconver2d().eval()
    d.load_state_dict(g9.case("model2d:sd"))
    checks.append(("deconver", d, g9["model2d:x"], g9["model2d:gy"], g9["model2d:y"],
                   {k: g9[f"model2d:grad:{k}"] for k, _ in d.named_parameters() if f"model2d:grad:{k}" in g9.z}, g9["model2d:gx"]))
    g10 = golden("g10_lower_d").case("model2d")
    f = lower_d_model().eval()
    f.load_state_dict({k[3:]: v for k, v in g10.items() if k.startswith("sd:")})
    checks.append(("factorizer", f, g10["x"], g10["gy"], g10["y"],
                   {k: g10["grad:" + k] for k, _ in f.named_parameters()}, g10["gx"]))
    for tag, model, x, gy, y_ref, g_ref, gx_ref in checks:
        model = model.to(DEV)
        timer = Fn.KernelTimer()
        Fn.set_timer(timer)
        composed._warned.clear()
        try:
            with warnings.catch_warnings():
                warnings.simplefilter("error", RuntimeWarning)
                xd = x.to(DEV).requires_grad_(True)
                y = model(xd)
                names = [k for k, _ in model.named_parameters()]
                grads = torch.autograd.grad(y, [xd] + list(model.parameters()), gy.to(DEV), allow_unused=True)
        finally:
            Fn.set_timer(None)
        ran = timer.summary()
        for name in ("conv2d_k3_", "conv2d_k2s2_", "tconv2d_k2s2_", "conv2d_k2s2_dgrad_", "tconv2d_k2s2_dgrad_",
                     "wgrad_conv2d_k3_", "wgrad_conv2d_k2s2_", "wgrad_tconv2d_k2s2_"):
            assert any(k.startswith(name) for k in ran), (tag, name, sorted(ran))
        P.close(f"{tag} y", y, y_ref)
        P.close(f"{tag} gx", grads[0], gx_ref)
        for k, gr in zip(names, grads[1:]):
            if k in g_ref:
                P.close(f"{tag} grad:{k}", gr, g_ref[k])


def test_deferred_finishes_are_bit_identical():
    from factorizer_amd.training import FlatAdamW
    torch.manual_seed(8)
    model = _deconver2d().to(DEV)
    x = torch.randn(2, 4, 16, 16, device=DEV)
    gy = torch.randn(2, 3, 16, 16, device=DEV)
    opt = FlatAdamW(model, lr=1e-3, deferred_finishes=True)

    def grads():
        opt.zero_grad()
        model(x).backward(gy)
        torch.cuda.synchronize()
        return [None if p.grad is None else p.grad.detach().clone() for p in model.parameters()]   # (some are unused)
    try:
        f0 = PW._Defer.flushed
        g_def = grads()
        assert PW._Defer.flushed > f0
        PW.defer_finishes(False)
        g_imm = grads()
    finally:
        PW.defer_finishes(False)
    assert sum(a is not None for a in g_def) >= 10
    for a, b in zip(g_def, g_imm):
        assert (a is None and b is None) or torch.equal(a, b)


def test_training_step_bf16_autocast_is_finite_and_deterministic():
    from factorizer_amd.training import FlatAdamW
    out = []
    for _ in range(2):
        torch.manual_seed(9)
        model = _deconver2d().to(DEV)
        opt = FlatAdamW(model, lr=1e-3)
        x = torch.randn(2, 4, 32, 32, device=DEV)
        t = (torch.rand(2, 3, 32, 32, device=DEV) > 0.5).float()
        composed._warned.clear()
        with warnings.catch_warnings(record=True) as rec:
            warnings.simplefilter("always")
            opt.zero_grad()
            with torch.autocast("cuda", dtype=torch.bfloat16):
                loss = ft.dice_ce_loss(model(x), t)
            loss.backward()
            opt.step()
        torch.cuda.synchronize()
        assert not [r for r in rec if "Conv" in str(r.message)], [str(r.message) for r in rec]   # the convolutions stay native
        assert torch.isfinite(loss).item()
        out.append([loss.detach().float().cpu()] + [p.detach().cpu().clone() for p in model.parameters()])
    for a, b in zip(*out):
        assert torch.isfinite(a).all() and torch.equal(a, b)


# ---- the C ABI, called directly ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["s2d", "k3", "d2s"])
def test_fz_gemm_and_fz_wgrad_through_ctypes(form):
    torch.manual_seed(10)
    lib = N.lib()
    B, C, O, H, W = 2, 8, 16, 8, 12
    Ho, Wo = H // 2, W // 2
    st = N.stream_ptr(torch.empty(1, device=DEV))
    d = N.GemmDesc()
    d.nsrc, d.act_dtype, d.products = 1, N.STORE_F32, N.PRODUCTS_FP32_MFMA
    if form == "s2d":
        x, w = torch.randn(B, C, H, W, device=DEV), torch.randn(O, C, 2, 2, device=DEV)
        y, ref = torch.empty(B, O, Ho, Wo, device=DEV), F.conv2d(x.double(), w.double(), stride=2)
        d.loader, d.Cin, d.K, d.M, d.Vin, d.Ncol = PW.LOAD_S2D_2D, C, 4 * C, O, H * W, Ho * Wo
        d.Di, d.Hi, d.Wi, d.Ho, d.Wo, d.ldw = 1, H, W, Ho, Wo, 4 * C
    elif form == "k3":
        x, w = torch.randn(B, C, H, W, device=DEV), torch.randn(O, C, 3, 3, device=DEV)
        y, ref = torch.empty(B, O, H, W, device=DEV), F.conv2d(x.double(), w.double(), padding=1)
        d.loader, d.Cin, d.K, d.M, d.Vin, d.Ncol = PW.LOAD_K3_2D, C, 9 * C, O, H * W, H * W
        d.Di, d.Hi, d.Wi, d.ldw = 1, H, W, 9 * C
    else:
        x, w = torch.randn(B, C, Ho, Wo, device=DEV), torch.randn(C, O, 2, 2, device=DEV)
        y, ref = torch.empty(B, O, H, W, device=DEV), F.conv_transpose2d(x.double(), w.double(), stride=2)
        d.epilogue, d.Cin, d.K, d.M, d.Vin, d.Ncol = PW.EPI_D2S_2D, C, C, 4 * O, Ho * Wo, Ho * Wo
        d.Ho, d.Wo, d.w_t, d.ldw = Ho, Wo, 1, 4 * O
    d.x[0], d.w, d.y, d.B = x.data_ptr(), w.data_ptr(), y.data_ptr(), B
    n0 = N.launch_count()
    assert lib.fz_gemm(ctypes.byref(d), st) == 0, lib.fz_last_error_string()
    torch.cuda.synchronize()
    assert N.launch_count() > n0
    P.close(f"fz_gemm {form}", y, ref)
    if form == "d2s":
        return
    # weight gradient through fz_wgrad with the matching Q loader
    gy = torch.randn_like(y)
    gw = torch.empty_like(w)
    q = N.WgradDesc()
    q.p, q.q[0], q.gw, q.M, q.Cin, q.nsrc, q.B = gy.data_ptr(), x.data_ptr(), gw.data_ptr(), O, C, 1, B
    q.act_dtype, q.products, q.Vq, q.H, q.W, q.D = N.STORE_F32, N.PRODUCTS_FP32_MFMA, H * W, H, W, 1
    if form == "s2d":
        q.loader, q.K, q.N, q.Ho, q.Wo = PW.QL_S2D_2D, 4 * C, Ho * Wo, Ho, Wo
        ref_w = torch.nn.grad.conv2d_weight(x.double(), w.shape, gy.double(), stride=2)
    else:
        q.loader, q.K, q.N = PW.QL_K3_2D, 9 * C, H * W
        ref_w = torch.nn.grad.conv2d_weight(x.double(), w.shape, gy.double(), padding=1)
    ws = torch.empty(max(lib.fz_wgrad_workspace_bytes(ctypes.byref(q)) // 4, 1), device=DEV)
    assert lib.fz_wgrad(ctypes.byref(q), ctypes.c_void_p(ws.data_ptr()), st) == 0, lib.fz_last_error_string()
    torch.cuda.synchronize()
    P.close(f"fz_wgrad {form}", gw, ref_w)
    # malformed: wrong K / odd Wo are refused
    q.K += 2
    assert lib.fz_wgrad(ctypes.byref(q), ctypes.c_void_p(ws.data_ptr()), st) == -1
    d.K += 2
    assert lib.fz_gemm(ctypes.byref(d), st) == -1
