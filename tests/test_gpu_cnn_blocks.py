"""-m gpu: the CNN blocks (factorizer_amd/cnn.py) and the default ft.UNet on the device.  A block's output and gradients equal,
bit for bit, the composition of the public pieces (the block's own convolution modules, ft.group_norm(act=...)) called one
after the other; every launch is native (no composed.warn_once fires); output and every gradient agree with the same module in
float64 on the CPU run under the activation gates the device had (cnn_cases.record_gates / replay_gates); under bf16 autocast a
block stays native.  Shapes: blocks at (16 -> 32, 8x8x8), the fixture's UNets at 16^3 / 32^2, B = 2."""
import copy
import warnings

import pytest
import torch
from torch import nn

import cnn_cases as CC
import factorizer_amd as ft
import parity as P
from factorizer_amd import _native, composed

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def gn(norm, x, act=None, slope=0.01):
    return ft.group_norm(x, norm.num_groups, norm.weight, norm.bias, norm.eps, act, slope)


def compose_double(m, x):
    for blk in (m.block1, m.block2):
        x = gn(blk[2], blk[0](x), "leaky_relu", blk[3].negative_slope)
    return x


def compose_basic(m, x):
    sc = m.shortcut(x)
    out = gn(m.norm1, m.conv1(x), "leaky_relu", m.act.negative_slope)
    return torch.nn.functional.leaky_relu(gn(m.norm2, m.conv2(out)) + sc, m.act.negative_slope)


def compose_preact(m, x):
    out = gn(m.norm1, x, "leaky_relu", m.act.negative_slope)
    sc = m.shortcut(out)
    out = gn(m.norm2, m.conv1(out), "leaky_relu", m.act.negative_slope)
    return m.conv2(out) + sc


def compose_sep(m, x):
    return m.pwconv2(m.dwconv(torch.nn.functional.gelu(m.pwconv1(x))))


COMPOSE = {"double": compose_double, "basic": compose_basic, "preact": compose_preact, "sep": compose_sep}


def _grads(fn, m, x, gy):
    composed._warned.clear()
    n0 = _native.launch_count()
    with warnings.catch_warnings():
        warnings.simplefilter("error", RuntimeWarning)                # a composed device branch would warn
        xr = x.clone().requires_grad_(True)
        y = fn(xr)
        grads = torch.autograd.grad(y, [xr] + list(m.parameters()), gy)
    return y, grads, _native.launch_count() - n0


@pytest.mark.parametrize("name", list(COMPOSE))
def test_block_equals_the_composition_of_the_public_pieces(name):
    m, x, gy = CC.gpu_case(name)
    m, x, gy = m.to(DEV), x.to(DEV), gy.to(DEV)
    y, grads, n = _grads(m, m, x, gy)
    y2, grads2, n2 = _grads(lambda t: COMPOSE[name](m, t), m, x, gy)
    assert n == n2 > 0                                                # the same native launches, norm + activation fused
    assert torch.equal(y, y2)
    for (k, _), a, b in zip([("x", None)] + list(m.named_parameters()), grads, grads2):
        assert torch.equal(a, b), k


@pytest.mark.parametrize("name", CC.GPU_CASES)
def test_against_float64_under_the_device_gates(name):
    """Output and every gradient against the same module in float64 on the CPU.  A LeakyReLU's derivative jumps at zero, and a
    pre-activation within rounding of zero can fall on either side in two correct evaluations; so the float64 module runs with
    the gates the DEVICE had ([y > 0] of each activation's output), the value staying float64's own.  Where a device gate differs
    from float64's sign the element must be a tie — |z64| within P.close's bound of that tensor (asserted) — and ties are
    counted: at most 8 per activation, 32 per case.  Bound: P.close's default, plus the fp32 CPU module's own distance to
    float64 under the same gates."""
    m, x, gy = CC.gpu_case(name)
    md = copy.deepcopy(m).to(DEV)
    gates = []
    with CC.record_gates(gates):
        y, grads, n = _grads(md, md, x.to(DEV), gy.to(DEV))
    assert n > 0 and len(gates) == {"double": 2, "basic": 2, "preact": 2, "sep": 0, "unet3d": 10, "unet2d": 10}[name]
    y64, g64, ties, extra = CC.gated_float64(m, x, gy, gates)
    P.note(f"{name}: gate ties per activation", ties=ties)
    CC.check_ties(ties)
    P.close(f"{name} y (float64, device gates)", y.detach(), y64, extra=extra[0])
    for k, a, b, e in zip(["x"] + [k for k, _ in m.named_parameters()], grads, g64, extra[1:]):
        P.close(f"{name} d{k} (float64, device gates)", a, b, extra=e)


@pytest.mark.parametrize("name", list(CC.UNETS))
def test_default_unet_trains_a_step_natively(name):
    nd, shape = CC.UNETS[name]
    m, x, gy = CC.gpu_case(name)
    m, x, gy = m.to(DEV), x.to(DEV), gy.to(DEV)
    norms = [mod for mod in m.modules() if type(mod) is ft.GroupNorm]
    assert len(norms) == 10
    y, grads, n = _grads(m, m, x, gy)
    y2, grads2, _ = _grads(m, m, x, gy)
    assert n > 0 and torch.equal(y, y2) and all(torch.equal(a, b) for a, b in zip(grads, grads2))
    assert all(torch.isfinite(t).all() for t in (y, *grads))
    # the same model on the framework's norm and activation: fewer native launches by exactly the norm's
    plain = CC.make_unet(name, norm=(nn.GroupNorm, (8,))).to(DEV)
    plain.load_state_dict(m.state_dict())
    y0, grads0, n_plain = _grads(plain, plain, x, gy)
    L = _native.lib()
    expect = 0
    for mod in norms:
        cg = mod.num_channels // 8
        V = x[0, 0].numel() // {16: 1, 32: 2 ** nd, 64: 4 ** nd}[mod.num_channels]
        expect += L.fz_gnorm_launches(cg, V, 0, 0) + L.fz_gnorm_launches(cg, V, 1, 1)
    assert n - n_plain == expect
    P.note(f"{name}: native norm against the framework norm, same weights",
           rel_l2=((y - y0).norm() / y0.norm()).item())


BF16_WHY = ("bf16 storage: the block stores four activation tensors (conv, norm + activation, conv, norm + activation), each rounded "
            "once to bf16, half a unit in the last place = 2^-9 of the element; the layers between them have gain about one "
            "(unit-variance x-hat, gamma = 1, He-scaled convolutions), so the roundings add to at most 4 x 2^-9 = 2^-7 of the "
            "largest element — the project's bf16 unit u of tests/gnorm_cases.py, in parity.close's max-norm form")


def test_a_block_under_bf16_autocast_stays_native():
    """DoubleConv under torch.autocast(bf16) on a bf16 input: no composed branch, bf16 activations, fp32 parameter gradients; output
    and every gradient against the float64 module on the rounded inputs under the device's gates, at the bf16 bound.  The tie
    tolerance is that bound too (a stored pre-activation is only that accurate), and ties are recorded, not capped: about one
    element in a hundred of a unit-variance tensor lies within 2^-7 max|z| of zero."""
    m, x, gy = CC.gpu_case("double")
    x, gy = x.bfloat16(), gy.bfloat16()
    md = copy.deepcopy(m).to(DEV)
    gates = []
    with CC.record_gates(gates), torch.autocast("cuda", dtype=torch.bfloat16):
        y, grads, n = _grads(md, md, x.to(DEV), gy.to(DEV))
    assert n > 0 and y.dtype == grads[0].dtype == torch.bfloat16 and all(p.dtype == torch.float32 for p in grads[1:])
    y64, g64, ties, _ = CC.gated_float64(m, x, gy, gates, tie_bound=lambda z: CC.close_bound(z, rel=2.0 ** -7))
    P.note("double bf16: gate ties per activation (not capped)", ties=ties)
    P.close("double bf16 y (float64 on the rounded input, device gates)", y.detach(), y64, rel=2.0 ** -7, why=BF16_WHY)
    for k, a, b in zip(["x"] + [k for k, _ in m.named_parameters()], grads, g64):
        P.close(f"double bf16 d{k} (float64 on the rounded input, device gates)", a, b, rel=2.0 ** -7, why=BF16_WHY)
