"""No GPU: the convolutions of a 2-D U-shape are the native containers convs.Conv2d / convs.ConvTranspose2d (still nn.Conv2d /
nn.ConvTranspose2d, so seeded initialisation and state_dict keys stay the reference's), their CPU forward is the framework's,
the tap orders and weight packing the host hands to fz_gemm / fz_wgrad reproduce F.conv2d in float64, and the C ABI refuses
malformed 2-D descriptors before anything touches a device."""
import ctypes

import pytest
import torch
import torch.nn.functional as F
from torch import nn

import factorizer_amd as ft
from factorizer_amd import _native, convs
from factorizer_amd import pointwise as PW

from test_deconver_cpu import MODELS
from test_modules_cpu import lower_d_model


def _fives_like():
    torch.manual_seed(0)
    return ft.Deconver(in_channels=4, out_channels=3, **MODELS["model2d"]).eval()


def _ushape_convs(model):
    out = {"stem": model.stem, "head": model.head}
    for i, blk in enumerate(model.encoder.blocks):
        if not isinstance(blk.downsample, nn.Identity):
            out[f"down{i}"] = blk.downsample
    for i, blk in enumerate(model.decoder.blocks):
        out[f"up{i}"] = blk.upsample
    return out


@pytest.mark.parametrize("which", ["factorizer", "deconver"])
def test_2d_ushape_builds_the_native_containers(which):
    model = lower_d_model() if which == "factorizer" else _fives_like()
    layers = _ushape_convs(model)
    assert sum(k.startswith("down") for k in layers) >= 1 and sum(k.startswith("up") for k in layers) >= 1
    for name, m in layers.items():
        if name.startswith("up"):
            assert type(m) is convs.ConvTranspose2d and isinstance(m, nn.ConvTranspose2d), (name, type(m))
        else:
            assert type(m) is convs.Conv2d and isinstance(m, nn.Conv2d), (name, type(m))
    assert tuple(model.stem.kernel_size) == (3, 3) and tuple(model.stem.padding) == (1, 1) and model.stem.bias is None
    assert tuple(model.head.kernel_size) == (1, 1)


def test_seeded_state_dicts_equal_the_goldens(golden):
    g9 = golden("g9_deconver").case("model2d:sd")
    sd = _fives_like().state_dict()
    assert list(sd) == list(g9)
    for k, v in sd.items():
        assert torch.equal(v, g9[k]), k
    g10 = {k[3:]: v for k, v in golden("g10_lower_d").case("model2d").items() if k.startswith("sd:")}
    torch.manual_seed(0)
    sd = lower_d_model().state_dict()
    assert sorted(sd) == sorted(g10)
    for k, v in sd.items():
        assert torch.equal(v, g10[k]), k


@pytest.mark.parametrize("kind,cin,cout,hw", [("k3", 3, 16, (8, 12)), ("k3", 4, 8, (16, 16)), ("k2s2", 8, 16, (8, 12)),
                                              ("k1", 8, 3, (6, 10)), ("t2", 16, 8, (4, 6))])
def test_cpu_forward_is_the_framework_conv(kind, cin, cout, hw):
    torch.manual_seed(1)
    if kind == "t2":
        m = convs.ConvTranspose2d(cin, cout, kernel_size=2, stride=2)
    else:
        k, s, p = {"k3": (3, 1, 1), "k2s2": (2, 2, 0), "k1": (1, 1, 0)}[kind]
        m = convs.Conv2d(cin, cout, kernel_size=k, stride=s, padding=p)
    x = torch.randn(2, cin, *hw)
    y = m(x)
    ref = (F.conv_transpose2d(x, m.weight, m.bias, stride=2) if kind == "t2"
           else F.conv2d(x, m.weight, m.bias, stride=m.stride, padding=m.padding))
    assert torch.equal(y, ref)
    if kind == "k2s2":
        skip, y2 = m.forward_fork(x.requires_grad_(True))
        assert skip is x and torch.equal(y2, ref)


# ---- host emulation of the kernels' operand orders ------------------------------------------------------------------
def _s2d(x):
    """In[(c, th, tw)][coarse n] = x[b, c, 2h+th, 2w+tw]  (FZ_LOAD_S2D_2D / FZ_QL_S2D_2D): (B, 4C, Ho*Wo)"""
    return F.unfold(x, kernel_size=2, stride=2)


def _d2s(rows, O, Ho, Wo):
    """rows m = (o, th, tw) -> y[b, o, 2h+th, 2w+tw]  (FZ_EPI_D2S_2D)"""
    B = rows.shape[0]
    return rows.reshape(B, O, 2, 2, Ho, Wo).permute(0, 1, 4, 2, 5, 3).reshape(B, O, 2 * Ho, 2 * Wo)


def _k3(x):
    """In[(c, kh, kw)][n] = x[b, c, h+kh-1, w+kw-1], zero padded  (FZ_LOAD_K3_2D / FZ_QL_K3_2D): (B, 9C, H*W)"""
    B, C, H, W = x.shape
    xp = F.pad(x, (1, 1, 1, 1))
    taps = [xp[:, :, kh:kh + H, kw:kw + W] for kh in range(3) for kw in range(3)]
    return torch.stack(taps, 2).reshape(B, 9 * C, H * W)


def test_tap_orders_and_weight_packing_match_conv2d_in_float64():
    torch.manual_seed(2)
    B, C, O, H, W = 2, 6, 5, 8, 12
    Ho, Wo = H // 2, W // 2
    x = torch.randn(B, C, H, W, dtype=torch.float64)
    k3_rows = _k3(x)
    assert torch.equal(k3_rows, F.unfold(x, 3, padding=1))      # the same (c, kh, kw) order as the framework's im2col
    # Conv2d k3p1: A = w.view(O, 9C) (row-major (c, kh, kw)), Out = A · In
    w3 = torch.randn(O, C, 3, 3, dtype=torch.float64)
    y = (w3.reshape(O, 9 * C) @ k3_rows).reshape(B, O, H, W)
    torch.testing.assert_close(y, F.conv2d(x, w3, padding=1), rtol=1e-12, atol=1e-12)
    # its input gradient: the same loader on gy with the flipped, channel-transposed filters (ConvK3Fn.backward)
    gy = torch.randn(B, O, H, W, dtype=torch.float64)
    wt = torch.flip(w3, dims=(2, 3)).transpose(0, 1).reshape(C, 9 * O)
    gx = (wt @ _k3(gy)).reshape(B, C, H, W)
    torch.testing.assert_close(gx, torch.nn.grad.conv2d_input(x.shape, w3, gy, padding=1), rtol=1e-12, atol=1e-12)
    # weight gradient: GW[o][(c,kh,kw)] = Σ P[o][n] Q[(c,kh,kw)][n]
    gw = torch.einsum("bon,bkn->ok", gy.reshape(B, O, -1), k3_rows).reshape(O, C, 3, 3)
    torch.testing.assert_close(gw, torch.nn.grad.conv2d_weight(x, w3.shape, gy, padding=1), rtol=1e-12, atol=1e-12)

    # Conv2d k2s2: K = 4C in (c, th, tw) order = w.view(O, 4C)
    w2 = torch.randn(O, C, 2, 2, dtype=torch.float64)
    q = _s2d(x)
    y = (w2.reshape(O, 4 * C) @ q).reshape(B, O, Ho, Wo)
    torch.testing.assert_close(y, F.conv2d(x, w2, stride=2), rtol=1e-12, atol=1e-12)
    # input gradient: rows (c, th, tw) from w used transposed (A[m][k] = w[k*4C + m]), then depth-to-space
    gy = torch.randn(B, O, Ho, Wo, dtype=torch.float64)
    gx = _d2s(w2.reshape(O, 4 * C).t() @ gy.reshape(B, O, -1), C, Ho, Wo)
    torch.testing.assert_close(gx, torch.nn.grad.conv2d_input(x.shape, w2, gy, stride=2), rtol=1e-12, atol=1e-12)
    gw = torch.einsum("bon,bkn->ok", gy.reshape(B, O, -1), q).reshape(O, C, 2, 2)
    torch.testing.assert_close(gw, torch.nn.grad.conv2d_weight(x, w2.shape, gy, stride=2), rtol=1e-12, atol=1e-12)

    # ConvTranspose2d k2s2: rows m = (o, th, tw), M = 4O, A[m][k] = w[k*4O + m] (w: (C, O, 2, 2)), bias per o = m // 4
    xc = torch.randn(B, C, Ho, Wo, dtype=torch.float64)
    wtc = torch.randn(C, O, 2, 2, dtype=torch.float64)
    bias = torch.randn(O, dtype=torch.float64)
    rows = wtc.reshape(C, 4 * O).t() @ xc.reshape(B, C, -1) + bias.repeat_interleave(4)[:, None]
    y = _d2s(rows, O, Ho, Wo)
    torch.testing.assert_close(y, F.conv_transpose2d(xc, wtc, bias, stride=2), rtol=1e-12, atol=1e-12)
    # its input gradient is the S2D loader on gy with w as [C][4O]; its weight gradient GW[c][(o,th,tw)] = Σ X[c][n] S2D(gy)
    gyf = torch.randn(B, O, H, W, dtype=torch.float64)
    xr = xc.detach().requires_grad_(True)
    wr = wtc.detach().requires_grad_(True)
    gxr, gwr = torch.autograd.grad(F.conv_transpose2d(xr, wr, stride=2), [xr, wr], gyf)
    torch.testing.assert_close((wtc.reshape(C, 4 * O) @ _s2d(gyf)).reshape(B, C, Ho, Wo), gxr, rtol=1e-12, atol=1e-12)
    gw = torch.einsum("bcn,bkn->ck", xc.reshape(B, C, -1), _s2d(gyf)).reshape(C, O, 2, 2)
    torch.testing.assert_close(gw, gwr, rtol=1e-12, atol=1e-12)


# ---- C ABI: the new ids are validated on the host ---------------------------------------------------------------------
def _gemm_desc(**kw):
    d = _native.GemmDesc()
    d.x[0] = d.w = d.y = 256            # never dereferenced: every case below is refused by the host checks
    d.nsrc, d.act_dtype, d.B = 1, _native.STORE_F32, 1
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def _wgrad_desc(**kw):
    d = _native.WgradDesc()
    d.p = d.q[0] = d.gw = 256
    d.nsrc, d.B = 1, 1
    for k, v in kw.items():
        setattr(d, k, v)
    return d


S2D = dict(loader=PW.LOAD_S2D_2D, Cin=8, K=32, M=16, Hi=8, Wi=8, Ho=4, Wo=4, Ncol=16, Vin=64)
K3 = dict(loader=PW.LOAD_K3_2D, Cin=8, K=72, M=16, Hi=8, Wi=8, Ncol=64, Vin=64)
D2S = dict(epilogue=PW.EPI_D2S_2D, Cin=8, K=8, M=16, Ho=4, Wo=4, Ncol=16, Vin=16)
BAD_GEMM = [
    ("s2d wrong K", dict(S2D, K=64), -1), ("s2d odd Wo", dict(S2D, Wi=6, Wo=3, Ncol=12, Vin=48), -1),
    ("s2d grid", dict(S2D, Hi=10), -1), ("s2d with d2s epilogue", dict(S2D, epilogue=PW.EPI_D2S_2D), -4),
    ("s2d with LayerNorm", dict(S2D, ln=1), -4), ("s2d two sources", dict(S2D, nsrc=2), -4),
    ("k3 wrong K", dict(K3, K=27 * 8), -1), ("k3 odd Cin", dict(K3, Cin=7, K=63), -1), ("k3 W % 4", dict(K3, Wi=6, Ncol=48, Vin=48), -1),
    ("k3 with 3-D d2s", dict(K3, epilogue=1), -4), ("d2s rows", dict(D2S, M=18), -1), ("d2s columns", dict(D2S, Ncol=20, Vin=20), -1),
    ("d2s with s2d loader", dict(D2S, loader=PW.LOAD_S2D), -4), ("d2s with activation", dict(D2S, eact=1), -4),
    ("bad loader", dict(S2D, loader=5), -4), ("bad epilogue", dict(D2S, epilogue=4), -4),
]


@pytest.mark.parametrize("what,kw,rc", BAD_GEMM, ids=[c[0] for c in BAD_GEMM])
def test_fz_gemm_refuses_malformed_2d_descriptors(what, kw, rc):
    lib = _native.lib()
    assert lib.fz_gemm(ctypes.byref(_gemm_desc(**kw)), None) == rc, lib.fz_last_error_string()


BAD_WGRAD = [
    ("s2d wrong K", dict(loader=PW.QL_S2D_2D, Cin=8, K=64, M=16, H=8, W=8, Ho=4, Wo=4, N=16, Vq=64), -1),
    ("s2d odd Wo", dict(loader=PW.QL_S2D_2D, Cin=8, K=32, M=16, H=8, W=6, Ho=4, Wo=3, N=12, Vq=48), -1),
    ("k3 wrong K", dict(loader=PW.QL_K3_2D, Cin=8, K=27 * 8, M=16, H=8, W=8, N=64, Vq=64), -1),
    ("k3 columns", dict(loader=PW.QL_K3_2D, Cin=8, K=72, M=16, H=8, W=8, N=32, Vq=64), -1),
    ("k3 two sources", dict(loader=PW.QL_K3_2D, Cin=8, K=72, M=16, H=8, W=8, N=64, Vq=64, nsrc=2), -4),
    ("bad loader", dict(loader=5, Cin=8, K=8, M=16, N=64, Vq=64), -4),
]


@pytest.mark.parametrize("what,kw,rc", BAD_WGRAD, ids=[c[0] for c in BAD_WGRAD])
def test_fz_wgrad_refuses_malformed_2d_descriptors(what, kw, rc):
    lib = _native.lib()
    assert lib.fz_wgrad(ctypes.byref(_wgrad_desc(**kw)), ctypes.c_void_p(256), None) == rc, lib.fz_last_error_string()


def test_header_names_the_2d_ids():
    import os
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "factorizer_hip.h")).read()
    for name, v in (("FZ_LOAD_S2D_2D", PW.LOAD_S2D_2D), ("FZ_LOAD_K3_2D", PW.LOAD_K3_2D), ("FZ_EPI_D2S_2D", PW.EPI_D2S_2D),
                    ("FZ_QL_S2D_2D", PW.QL_S2D_2D), ("FZ_QL_K3_2D", PW.QL_K3_2D)):
        assert f"#define {name} {v} " in hdr, name
