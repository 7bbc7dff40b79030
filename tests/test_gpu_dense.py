"""-m gpu: the fp32-MFMA GEMM family (csrc/gemm.hip, gemm_p32.hip, gemm_stream.hip, mlp_chain32.hip, mlp_chain64.hip, mlp_chain_wg.hip,
gemm_dw.hip, wgrad.hip, ln.hip) behind the layer
Functions of factorizer_amd/pointwise.py, against ATen on CPU (the arithmetic the reference
runs: nn.Conv1d / nn.LayerNorm / nn.Conv3d / nn.ConvTranspose3d) and the reference goldens."""
import pytest
import torch
import torch.nn.functional as F
from torch import nn

import factorizer_amd as ft
from factorizer_amd import _native
from factorizer_amd import pointwise as PW
import parity as P

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TOL = dict(rtol=2e-4, atol=2e-4)


def _cmp(a, b, what, rtol=1e-4, why=None):
    """max|a − b| ≤ rtol · max|b| (+1e-6): the north-star bound, achieved error recorded (tests/parity.py)."""
    P.close(what, a, b, rel=rtol, why=why)


def _run_both(fn_dev, fn_cpu, tensors, gy_shape_like=None):
    """tensors: list of CPU leaf tensors (None allowed).  Returns nothing; asserts parity."""
    cpu = [None if t is None else t.clone().requires_grad_(True) for t in tensors]
    dev = [None if t is None else t.clone().to(DEV).requires_grad_(True) for t in tensors]
    n0 = _native.launch_count()
    yd = fn_dev(*dev)
    yc = fn_cpu(*cpu)
    _cmp(yd, yc, "forward")
    torch.manual_seed(99)
    gy = torch.randn_like(yc)
    gd = torch.autograd.grad(yd, [t for t in dev if t is not None], gy.to(DEV))
    gc = torch.autograd.grad(yc, [t for t in cpu if t is not None], gy)
    torch.cuda.synchronize()
    assert _native.launch_count() > n0
    for i, (a, b) in enumerate(zip(gd, gc)):
        _cmp(a, b, f"grad[{i}]")


def _lin_cpu(x, w, b=None):
    return F.conv1d(x.flatten(2), w, b).reshape(x.shape[0], w.shape[0], *x.shape[2:])


SHAPES = [
    (2, 32, 32, (8, 8, 8)),
    (1, 16, 24, (4, 4, 4)),     # rows not a multiple of 32, tiny V (tile tail)
    (2, 64, 32, (6, 4, 4)),     # V = 96: partial wave tiles
    (1, 32, 64, (8, 8, 16)),    # two row blocks (MB = 2)
    (1, 32, 3, (8, 8, 8)),      # head
    (1, 128, 128, (4, 4, 8)),   # several row blocks, K > one LDS chunk? (64 a-steps = K 128)
    (1, 512, 256, (4, 4, 4)),   # K-chunked weights
]


@pytest.mark.parametrize("B,Cin,Cout,S", SHAPES)
@pytest.mark.parametrize("bias", [True, False])
def test_linear(B, Cin, Cout, S, bias):
    torch.manual_seed(0)
    x = torch.randn(B, Cin, *S)
    w = torch.randn(Cout, Cin, 1) / Cin ** 0.5
    b = torch.randn(Cout) if bias else None
    _run_both(lambda x, w, b=None: PW.linear_cf(x, w, b), _lin_cpu, [x, w, b])


@pytest.mark.parametrize("B,Cin,Cout,S", SHAPES[:5])
@pytest.mark.parametrize("act", ["relu", "none"])
def test_ln_linear(B, Cin, Cout, S, act):
    torch.manual_seed(1)
    x = torch.randn(B, Cin, *S) * 2 + 0.5
    g, bt = torch.rand(Cin) + 0.5, torch.randn(Cin) * 0.3
    w = torch.randn(Cout, Cin, 1) / Cin ** 0.5
    b = torch.randn(Cout)

    def cpu(x, g, bt, w, b):
        y = _lin_cpu(F.layer_norm(x.movedim(1, -1), (Cin,), g, bt, 1e-5).movedim(-1, 1), w, b)
        return torch.relu(y) if act == "relu" else y

    _run_both(lambda x, g, bt, w, b: PW.ln_linear(x, g, bt, 1e-5, w, b, act), cpu, [x, g, bt, w, b])


def test_ln_linear_large_mean():
    """single-pass variance must stay accurate when |mean| >> std"""
    torch.manual_seed(2)
    x = torch.randn(1, 32, 8, 8, 8) * 0.5 + 30.0
    g, bt = torch.rand(32) + 0.5, torch.randn(32)
    w = torch.randn(32, 32, 1) / 32 ** 0.5
    y = PW.ln_linear(x.to(DEV), g.to(DEV), bt.to(DEV), 1e-5, w.to(DEV), None, "none")
    yc = _lin_cpu(F.layer_norm(x.movedim(1, -1), (32,), g, bt, 1e-5).movedim(-1, 1), w)
    _cmp(y, yc, "ln large mean")


@pytest.mark.parametrize("kind", ["ln", "ln_relu", "plain", "plain_nobias", "head3"])
@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16])
def test_stage0_persistent_32_to_32(kind, dt):
    """gemm_p32_kernel (persistent waves, >= 4096 wave tiles): 32 -> 32 at 81 x 81 x 80 voxels — 4100.6 tiles of 128 columns,
    so the last tile is partial — against float64 on the host; forward values and the LayerNorm statistics it leaves for
    the backward (through the input gradient)."""
    torch.manual_seed(11)
    S = (81, 81, 80)
    x = (torch.randn(1, 32, *S) * 2 + 0.5)
    g, bt = torch.rand(32) + 0.5, torch.randn(32) * 0.3
    M = 3 if kind == "head3" else 32   # (M < 32: the 32 -> 3 head; rows beyond M are neither computed into nor stored)
    w = torch.randn(M, 32, 1) / 32 ** 0.5
    b = None if kind == "plain_nobias" else torch.randn(M)
    xd = x.to(DEV, dt).requires_grad_(True)
    n0 = _native.launch_count()
    if kind.startswith("ln"):
        y = PW.ln_linear(xd, g.to(DEV), bt.to(DEV), 1e-5, w.to(DEV), b.to(DEV), "relu" if kind == "ln_relu" else "none")
    else:
        y = PW.linear_cf(xd, w.to(DEV), None if b is None else b.to(DEV))
    assert _native.launch_count() > n0
    x64 = xd.detach().double().cpu().requires_grad_(True)
    if kind.startswith("ln"):
        z = F.layer_norm(x64.movedim(1, -1), (32,), g.double(), bt.double(), 1e-5).movedim(-1, 1)
    else:
        z = x64
    y64 = _lin_cpu(z, w.double(), None if b is None else b.double())
    if kind == "ln_relu":
        y64 = torch.relu(y64)
    tol = 1e-4 if dt == torch.float32 else 8e-3
    why = None if dt == torch.float32 else "bf16 storage: the output (and the gradient) is rounded to 8 bits of mantissa"
    _cmp(y.float().cpu(), y64.float(), f"p32 {kind} forward", rtol=tol, why=why)
    torch.manual_seed(12)
    gy = torch.randn(y64.shape, dtype=torch.float64)
    (gx,) = torch.autograd.grad(y, xd, gy.to(DEV, dt))
    (gx64,) = torch.autograd.grad(y64, x64, gy.to(dt).double())
    _cmp(gx.float().cpu(), gx64.float(), f"p32 {kind} input gradient", rtol=tol * 2,
         why=why or "input gradient of LayerNorm + Linear: two chained fp32 kernels against float64")


@pytest.mark.parametrize("B,Cin,Cout,S", SHAPES[:4])
@pytest.mark.parametrize("act", ["gelu", "none"])
@pytest.mark.parametrize("res", [True, False])
def test_act_linear_res(B, Cin, Cout, S, act, res):
    torch.manual_seed(3)
    z = torch.randn(B, Cin, *S)
    w = torch.randn(Cout, Cin, 1) / Cin ** 0.5
    b = torch.randn(Cout)
    r = torch.randn(B, Cout, *S) if res else None

    def cpu(z, w, b, r=None):
        y = _lin_cpu(F.gelu(z) if act == "gelu" else z, w, b)
        return y if r is None else y + r

    _run_both(lambda z, w, b, r=None: PW.act_linear_res(z, w, b, r, act), cpu, [z, w, b, r])


def test_cat_linear():
    torch.manual_seed(4)
    x1, x2 = torch.randn(2, 32, 8, 8, 8), torch.randn(2, 32, 8, 8, 8)
    w = torch.randn(32, 64, 1) / 8
    _run_both(lambda a, b, w: PW.cat_linear(a, b, w), lambda a, b, w: _lin_cpu(torch.cat([a, b], 1), w), [x1, x2, w])
    x1, x2 = torch.randn(1, 16, 4, 4, 4), torch.randn(1, 8, 4, 4, 4)
    w = torch.randn(8, 24, 1) / 5
    _run_both(lambda a, b, w: PW.cat_linear(a, b, w), lambda a, b, w: _lin_cpu(torch.cat([a, b], 1), w), [x1, x2, w])


@pytest.mark.parametrize("C,S", [(32, (8, 8, 8)), (16, (4, 4, 4)), (512, (4, 4, 4)), (6, (2, 2, 4)), (64, (8, 8, 6)),
                                 (128, (4, 8, 8)), (256, (4, 4, 4))])
def test_layernorm(C, S):
    torch.manual_seed(5)
    x = torch.randn(2, C, *S) * 3 + 1
    g, bt = torch.rand(C) + 0.5, torch.randn(C)
    _run_both(lambda x, g, bt: PW.layernorm_cf(x, g, bt, 1e-5),
              lambda x, g, bt: F.layer_norm(x.movedim(1, -1), (C,), g, bt, 1e-5).movedim(-1, 1), [x, g, bt])


@pytest.mark.parametrize("Cin,Cout,S", [(32, 64, (8, 8, 8)), (8, 16, (8, 8, 8)), (64, 128, (4, 4, 8)),
                                        (256, 512, (4, 4, 4)), (16, 16, (4, 6, 4))])
def test_conv_k2s2(Cin, Cout, S):
    torch.manual_seed(6)
    m = nn.Conv3d(Cin, Cout, kernel_size=2, stride=2)
    d = ft.Conv3d(Cin, Cout, kernel_size=2, stride=2)
    d.load_state_dict(m.state_dict())
    d = d.to(DEV)
    x = torch.randn(2, Cin, *S)
    _run_both(lambda x, w, b: F.conv3d(x, w, b, stride=2) if not x.is_cuda else PW.ConvK2S2Fn.apply(x, w, b),
              lambda x, w, b: F.conv3d(x, w, b, stride=2), [x, m.weight.detach(), m.bias.detach()])
    _cmp(d(x.to(DEV)), m(x), "module")


@pytest.mark.parametrize("Cin,Cout,S", [(32, 64, (8, 8, 8)), (8, 16, (4, 4, 12)), (64, 128, (4, 4, 8))])
def test_skip_plus_conv_k2s2_one_node(Cin, Cout, S):
    """An encoder output that feeds both the skip connection and the down-convolution
    (unet.py:95-99): the fused node (Conv3d.forward_fork) adds the two gradients inside the
    input-gradient kernel; same values as autograd's separate accumulation on CPU."""
    torch.manual_seed(3)
    conv = ft.Conv3d(Cin, Cout, kernel_size=2, stride=2)
    x = torch.randn(2, Cin, *S)
    gs, gd = torch.randn(2, Cin, *S), torch.randn(2, Cout, *(d // 2 for d in S))
    xc = x.clone().requires_grad_(True)
    (xc * gs).sum().add((conv(xc) * gd).sum()).backward()
    ref_w, ref_b = conv.weight.grad.clone(), conv.bias.grad.clone()
    conv.zero_grad()
    conv = conv.to(DEV)
    xd = x.to(DEV).requires_grad_(True)
    h = xd * 1.0     # a non-leaf, as in the encoder
    n0 = _native.launch_count()
    skip, y = conv.forward_fork(h)
    assert skip.data_ptr() == h.data_ptr()
    ((skip * gs.to(DEV)).sum() + (y * gd.to(DEV)).sum()).backward()
    assert _native.launch_count() > n0
    _cmp(xd.grad, xc.grad, "gx")
    _cmp(conv.weight.grad, ref_w, "gw")
    _cmp(conv.bias.grad, ref_b, "gb")
    # only the skip branch reaches the loss: the node passes its gradient through
    xd2 = x.to(DEV).requires_grad_(True)
    skip, y = conv.forward_fork(xd2 * 1.0)
    (skip * gs.to(DEV)).sum().backward()
    _cmp(xd2.grad, gs, "gx skip only")


@pytest.mark.parametrize("Cin,Cout,S", [(64, 32, (4, 4, 4)), (16, 8, (4, 4, 4)), (512, 256, (2, 2, 4)),
                                        (32, 16, (2, 4, 2))])
def test_tconv_k2s2(Cin, Cout, S):
    torch.manual_seed(7)
    m = nn.ConvTranspose3d(Cin, Cout, kernel_size=2, stride=2)
    x = torch.randn(2, Cin, *S)
    _run_both(lambda x, w, b: PW.TConvK2S2Fn.apply(x, w, b),
              lambda x, w, b: F.conv_transpose3d(x, w, b, stride=2), [x, m.weight.detach(), m.bias.detach()])


@pytest.mark.parametrize("Cin,Cout,S", [(4, 32, (8, 8, 8)), (4, 8, (4, 6, 8)), (2, 16, (16, 4, 4))])
def test_conv_k3_stem(Cin, Cout, S):
    torch.manual_seed(8)
    w = torch.randn(Cout, Cin, 3, 3, 3) / 5
    x = torch.randn(2, Cin, *S)
    _run_both(lambda x, w: PW.ConvK3Fn.apply(x, w, None), lambda x, w: F.conv3d(x, w, None, padding=1), [x, w])


@pytest.mark.parametrize("name", ["conv_k2s2", "tconv_k2s2", "conv_k3", "conv_k1", "linear", "linear_nobias",
                                  "layernorm", "mlp"])
def test_reference_layer_goldens(golden, name):
    """tests/golden/g7_layers.npz: outputs of the reference's own layers."""
    g = golden("g7_layers").case(name)
    sd = {k[3:]: v for k, v in g.items() if k.startswith("sd:")}
    mods = {
        "conv_k2s2": lambda: ft.Conv3d(8, 16, kernel_size=2, stride=2),
        "tconv_k2s2": lambda: ft.ConvTranspose3d(16, 8, kernel_size=2, stride=2),
        "conv_k3": lambda: ft.Conv3d(4, 8, kernel_size=3, padding=1, bias=False),
        "conv_k1": lambda: ft.Conv3d(8, 3, kernel_size=1),
        "linear": lambda: ft.Linear(16, 24),
        "linear_nobias": lambda: ft.Linear(16, 16, bias=False),
        "layernorm": lambda: ft.LayerNorm(16),
        "mlp": lambda: ft.MLP(16, ratio=2),
    }
    m = mods[name]()
    m.load_state_dict(sd)
    m = m.to(DEV)
    x = g["x"].to(DEV).requires_grad_(True)
    n0 = _native.launch_count()
    y = m(x)
    names = [k for k, _ in m.named_parameters()]
    grads = torch.autograd.grad(y, [x] + list(m.parameters()), g["gy"].to(DEV))
    torch.cuda.synchronize()
    assert _native.launch_count() > n0
    _cmp(y, g["y"], "y")
    _cmp(grads[0], g["gx"], "gx")
    for k, gr in zip(names, grads[1:]):
        _cmp(gr, g["grad:" + k], k)


@pytest.mark.parametrize("Cin,Cout,S", [(4, 32, (8, 8, 32)), (4, 32, (4, 6, 64)), (2, 48, (8, 4, 32)), (4, 8, (3, 5, 32))])
def test_conv_k3_stem_direct_wgrad(Cin, Cout, S):
    """W % 32 == 0: the LDS-halo weight-gradient kernel of csrc/conv3.hip."""
    torch.manual_seed(18)
    w = torch.randn(Cout, Cin, 3, 3, 3) / 5
    b = torch.randn(Cout)
    x = torch.randn(2, Cin, *S)
    _run_both(lambda x, w, b: PW.ConvK3Fn.apply(x, w, b), lambda x, w, b: F.conv3d(x, w, b, padding=1), [x, w, b])


def test_dice_bce_loss_fused():
    """csrc/loss.hip against the composed ATen form (and the oracle's restatement)."""
    from oracle import cpu_ref as O
    torch.manual_seed(21)
    z = torch.randn(2, 3, 8, 8, 16) * 3
    t = (torch.rand(2, 3, 8, 8, 16) > 0.5).float()
    zc = z.clone().requires_grad_(True)
    lc = O.dice_bce_loss(zc, t)
    (gc,) = torch.autograd.grad(lc * 1.7, zc)
    zd = z.to(DEV).requires_grad_(True)
    n0 = _native.launch_count()
    ld = ft.dice_bce_loss(zd, t.to(DEV))
    (gd,) = torch.autograd.grad(ld * 1.7, zd)
    assert _native.launch_count() > n0
    assert abs(ld.item() - lc.item()) <= 1e-5 * abs(lc.item()) + 1e-6
    _cmp(gd, gc, "dloss/dlogits", rtol=1e-4)


@pytest.mark.parametrize("C", [2, 3, 4, 8])
def test_dice_ce_loss_fused(C):
    """The recipe's DiceCELoss(sigmoid, squared_pred) for a multi-channel head (softmax cross entropy with
    float multi-label targets, MONAI >= 1.3) — csrc/loss.hip dice_ce_* against the oracle's restatement."""
    from oracle import cpu_ref as O
    torch.manual_seed(22)
    z = torch.randn(2, C, 8, 8, 16) * 3
    t = (torch.rand(2, C, 8, 8, 16) > 0.5).float()
    zc = z.clone().requires_grad_(True)
    lc = O.dice_ce_loss(zc, t)
    (gc,) = torch.autograd.grad(lc * 1.7, zc)
    zd = z.to(DEV).requires_grad_(True)
    n0 = _native.launch_count()
    ld = ft.dice_ce_loss(zd, t.to(DEV))
    (gd,) = torch.autograd.grad(ld * 1.7, zd)
    assert _native.launch_count() > n0
    assert abs(ld.item() - lc.item()) <= 1e-5 * abs(lc.item()) + 1e-6
    _cmp(gd, gc, "dloss/dlogits", rtol=1e-4)
    assert abs(ft.DiceCELoss(sigmoid=True, squared_pred=True)(zd, t.to(DEV)).item() - ld.item()) == 0.0


@pytest.mark.parametrize("products", [_native.PRODUCTS_DEFAULT, _native.PRODUCTS_SPLIT_BF16, _native.PRODUCTS_FP32_MFMA],
                         ids=["default", "split_bf16", "fp32_mfma"])
@pytest.mark.parametrize("bf", [False, True])
@pytest.mark.parametrize("C,Hd", [(32, 64), (32, 128), (64, 128)])
@pytest.mark.parametrize("B,S", [(2, (8, 8, 8)), (1, (6, 4, 5)), (2, (16, 16, 12))])
def test_mlp_chain_kernel(B, S, C, Hd, bf, products):
    """fz_mlp_chain modes 0 and 1 (csrc/mlp_chain.hip: the dispatch; mlp_chain32.hip gemm_chain_kernel, mlp_chain64.hip
    gemm_chain64_kernel) against the layer-by-layer CPU composition x + fc2(gelu(fc1(LN(x)))) (factorizer.py:76,
    mlp.py:54-60, norm.py:29-34): forward, the saved pre-activation / statistics, and the backward chain (gz1, gx1, dγ, dβ).
    V = 120 and 3072 cover partial column tiles; V = 120 at C = 64 is one tile, an odd count: the 256-thread fp32-MFMA form
    whatever the products.  Every form the dispatch can pick: fp32 and bf16 storage, each on the library's default products,
    on split-bf16 and on fp32-MFMA products.  bf16 storage: inputs rounded first, the backward's reference reads the STORED
    pre-activation, and each tensor written in bf16 is allowed its one stored rounding."""
    torch.manual_seed(3)
    # C = 32: hidden 64 = mlp_ratio 2 (README), 128 = mlp_ratio 4 (BraTS bundle, train.yaml:62); C = 64, hidden 128 =
    # stage 1 of the README model (gemm_chain64_kernel: the hidden tensor in two passes of 64 rows)
    rnd = (lambda t: t.bfloat16().float()) if bf else (lambda t: t)
    x = rnd(torch.randn(B, C, *S) * 2 + 0.5)
    ln_w, ln_b = torch.rand(C) + 0.5, torch.randn(C) * 0.1
    w1, b1 = torch.randn(Hd, C) * 0.2, torch.randn(Hd) * 0.1
    w2, b2 = torch.randn(C, Hd) * 0.2, torch.randn(C) * 0.1
    g2 = rnd(torch.randn(B, C, *S))
    dt = torch.bfloat16 if bf else torch.float32
    d = lambda t: t.to(DEV).contiguous()  # noqa: E731
    xd, g2d = d(x).to(dt), d(g2).to(dt)
    stored = dict(rtol=2.0 ** -8, why="bf16 storage: one rounding of the stored tensor") if bf else {}
    n0 = _native.launch_count()
    with _native.use_products(products):
        x2, z1, st = PW._mlp_fwd_chain(xd, d(ln_w), d(ln_b), 1e-5, d(w1), d(b1), d(w2), d(b2))
        gz1, gx1, gg, gb = PW._mlp_bwd_chain(g2d, z1, d(w1), d(w2), xd, st, d(ln_w))
    assert _native.launch_count() > n0
    assert x2.dtype == dt and z1.dtype == dt and gz1.dtype == dt and gx1.dtype == dt
    # CPU composition with autograd
    xc = x.clone().requires_grad_(True)
    lw, lb = ln_w.clone().requires_grad_(True), ln_b.clone().requires_grad_(True)
    xn = F.layer_norm(xc.movedim(1, -1), (C,), lw, lb, 1e-5).movedim(-1, 1)
    z1c = _lin_cpu(xn, w1.unsqueeze(-1), b1)
    _cmp(z1.float(), z1c, "z1", **stored)
    _cmp(x2.float(), xc + _lin_cpu(F.gelu(z1c), w2.unsqueeze(-1), b2), "x2", **stored)
    _cmp(st[:, 0], x.mean(1).reshape(B, -1), "mean")
    if bf:
        # the backward reads the STORED pre-activation (bf16): give the CPU graph exactly those values (a bf16 tie
        # broken the other way is 2^-8 of one addend)
        z1c = z1c + (z1.float().cpu().reshape(z1c.shape) - z1c.detach())
    z1c.retain_grad()
    yc = xc + _lin_cpu(F.gelu(z1c), w2.unsqueeze(-1), b2)
    yc.backward(g2)
    for n, a, r in (("gz1", gz1, z1c.grad), ("gx1", gx1, xc.grad)):
        _cmp(a.float(), r, n, **(dict(rtol=4e-3, why=f"bf16 activation storage: {n} is rounded once on store (2^-9 relative)") if bf else {}))
    _cmp(gg, lw.grad, "dgamma")
    _cmp(gb, lb.grad, "dbeta")


@pytest.mark.parametrize("bf", [False, True])
@pytest.mark.parametrize("C,Hd", [(32, 64), (64, 128)])
@pytest.mark.parametrize("B,S", [(2, (8, 8, 8)), (1, (6, 4, 5)), (1, (8, 8, 6)), (2, (16, 16, 12)), (3, (32, 32, 40))])
def test_outproj_and_mlp_chain_in_one_launch(B, S, bf, C, Hd):
    """Steps 3 + 4 of FactorizerBlock.forward — x1 = x + out_proj(a) (factorizer.py:53,75) and x2 = x1 + mlp(LN(x1))
    (factorizer.py:76; mlp.py:54-63; norm.py:29-34) — as ONE launch (fz_mlp_chain with pre_in: the out-projection on the
    accumulators in front of the chained GEMMs, x1 written once and never read back) against the float64 composition on
    the CPU and against the two-launch form it replaces.  V = 120 covers a ragged tile; (3, 32·32·40) is 480 tiles, below the
    cap of 512 resident workgroups (240 pairs, below 256, at C = 64): one tile per workgroup (the tile walk:
    tests/test_gpu_mlp_chain.py).  bf16 storage: everything downstream of x1 must see the STORED (rounded) x1, as the
    two-launch form does.
    [r5] also at C = 64, hidden 128 (stage 1 of the README model: the 512-thread chain around three pre-split weight images),
    which takes an even number of 256-voxel tiles per sample — V = 384: a ragged second tile; V = 120 is refused."""
    torch.manual_seed(17)
    if C == 64 and ((S[0] * S[1] * S[2] + 255) // 256) % 2:
        assert not PW._outproj_mlp_ok(C, Hd, S[0] * S[1] * S[2])
        return
    rnd = (lambda t: t.bfloat16().float()) if bf else (lambda t: t)
    a = rnd(torch.relu(torch.randn(B, C, *S)) * 1.5)
    x = rnd(torch.randn(B, C, *S) * 2 + 0.5)
    wo, bo = torch.randn(C, C) * 0.2, torch.randn(C) * 0.1
    ln_w, ln_b = torch.rand(C) + 0.5, torch.randn(C) * 0.1
    w1, b1 = torch.randn(Hd, C) * 0.2, torch.randn(Hd) * 0.1
    w2, b2 = torch.randn(C, Hd) * 0.2, torch.randn(C) * 0.1
    dt = torch.bfloat16 if bf else torch.float32
    d = lambda t: t.to(DEV).contiguous()  # noqa: E731
    ad, xd = d(a).to(dt), d(x).to(dt)
    V = a[0, 0].numel()
    assert PW._outproj_mlp_ok(C, Hd, V)
    n0 = _native.launch_count()
    x1, x2, z1, st = PW._outproj_mlp_fwd_chain(ad, d(wo), d(bo), xd, d(ln_w), d(ln_b), 1e-5, d(w1), d(b1), d(w2), d(b2))
    assert _native.launch_count() - n0 == 1
    # float64 composition (bf16: with the storage rounding of x1, the one tensor between the two steps that reaches HBM)
    D = torch.float64
    x1c = x.to(D) + _lin_cpu(a.to(D), wo.to(D).unsqueeze(-1), bo.to(D))
    if bf:
        x1c = x1c.float().bfloat16().to(D)
    xn = F.layer_norm(x1c.movedim(1, -1), (C,), ln_w.to(D), ln_b.to(D), 1e-5).movedim(-1, 1)
    z1c = _lin_cpu(xn, w1.to(D).unsqueeze(-1), b1.to(D))
    x2c = x1c + _lin_cpu(F.gelu(z1c), w2.to(D).unsqueeze(-1), b2.to(D))
    _cmp(x1.float(), x1c.float(), "x1", **(dict(rtol=2.0 ** -8, why="bf16 storage: one rounding of the stored tensor") if bf else {}))
    if not bf:
        _cmp(z1, z1c.float(), "z1")
        _cmp(x2, x2c.float(), "x2")
        _cmp(st[:, 0], x1c.mean(1).reshape(B, -1).float(), "mean")
        _cmp(st[:, 1], (1.0 / torch.sqrt(x1c.var(1, unbiased=False) + 1e-5)).reshape(B, -1).float(), "rstd")
    # the two launches it replaces, same inputs
    x1b = torch.empty_like(ad)
    PW._gemm([ad], d(wo), x1b, B=B, Cin=C, Vin=V, M=C, K=C, Ncol=V, bias=d(bo), res=xd, name="act_linear_res")
    x2b, z1b, stb = PW._mlp_fwd_chain(x1b, d(ln_w), d(ln_b), 1e-5, d(w1), d(b1), d(w2), d(b2))
    if bf:
        # one unit in the last place of bf16 where the two product paths round a tie differently; everything else identical
        assert (x1.float() - x1b.float()).abs().max().item() <= 2.0 ** -7 * x1b.float().abs().max().item()
        same = x1 == x1b
        assert same.float().mean().item() > 0.995
        _cmp(x2.float(), x2b.float(), "x2 one launch vs two (bf16)", rtol=4 * 2.0 ** -8,
             why="bf16 storage: a handful of x1 elements rounded the other way by the two product paths, then one more stored rounding")
    else:
        _cmp(x1, x1b, "x1 one launch vs two", rtol=1e-5)
        _cmp(z1, z1b, "z1 one launch vs two", rtol=1e-5)
        _cmp(x2, x2b, "x2 one launch vs two", rtol=1e-5)
        _cmp(st, stb, "stats one launch vs two", rtol=1e-5)
    # replay: bit-identical
    x1r, x2r, z1r, str_ = PW._outproj_mlp_fwd_chain(ad, d(wo), d(bo), xd, d(ln_w), d(ln_b), 1e-5, d(w1), d(b1), d(w2), d(b2))
    assert torch.equal(x1, x1r) and torch.equal(x2, x2r) and torch.equal(z1, z1r) and torch.equal(st, str_)


@pytest.mark.parametrize("Hd", [64, 128])
@pytest.mark.parametrize("bf", [False, True])
@pytest.mark.parametrize("B,S", [(2, (8, 8, 8)), (1, (6, 4, 5)), (2, (16, 16, 12)), (3, (32, 32, 40))])
def test_mlp_chain_backward_with_weight_gradients(B, S, bf, Hd):
    """fz_mlp_chain mode 2 (gemm_chain_bwd_wg_kernel): the input-gradient chain AND dW1, db1, dW2, db2 of the MLP from
    one pass over (g2, z1, x1) — transposed MFMA operands through wave-private LDS, sums carried across the tiles of
    the persistent workgroups, rows added in order.  Against CPU autograd of x + fc2(gelu(fc1(LN(x)))); V = 120
    covers a ragged tile; (3, 32·32·40) is 480 tiles, one per workgroup (sums carried over several tiles, and the float64
    reference of the sums: tests/test_gpu_mlp_chain.py).  Run twice: bit-identical."""
    torch.manual_seed(11)
    C = 32    # Hd = 128 (mlp_ratio 4, BraTS bundle): one launch per 64-row half of the hidden tensor
    rnd = (lambda t: t.bfloat16().float()) if bf else (lambda t: t)
    x = rnd(torch.randn(B, C, *S) * 2 + 0.5)
    ln_w, ln_b = torch.rand(C) + 0.5, torch.randn(C) * 0.1
    w1, b1 = torch.randn(Hd, C) * 0.2, torch.randn(Hd) * 0.1
    w2, b2 = torch.randn(C, Hd) * 0.2, torch.randn(C) * 0.1
    g2 = rnd(torch.randn(B, C, *S))
    dt = torch.bfloat16 if bf else torch.float32
    d = lambda t: t.to(DEV).contiguous()  # noqa: E731
    xd, g2d = d(x).to(dt), d(g2).to(dt)
    x2, z1, st = PW._mlp_fwd_chain(xd, d(ln_w), d(ln_b), 1e-5, d(w1), d(b1), d(w2), d(b2))
    xc = x.clone().requires_grad_(True)
    prm = [t.clone().requires_grad_(True) for t in (ln_w, ln_b, w1, b1, w2, b2)]
    xn = F.layer_norm(xc.movedim(1, -1), (C,), prm[0], prm[1], 1e-5).movedim(-1, 1)
    z1c = _lin_cpu(xn, prm[2].unsqueeze(-1), prm[3])
    if bf:
        # the backward reads the STORED pre-activation (bf16): give the CPU graph exactly those values (a bf16 tie
        # broken the other way is 2^-8 of one addend, far above the bound on the voxel sums)
        z1c = z1c + (z1.float().cpu().reshape(z1c.shape) - z1c.detach())
    yc = xc + _lin_cpu(F.gelu(z1c), prm[4].unsqueeze(-1), prm[5])
    gxc, ggc, gbc, gw1c, gb1c, gw2c, gb2c = torch.autograd.grad(yc, [xc] + prm, g2)
    assert PW._mlp_wgrad_fused_ok(C, Hd, x[0, 0].numel())
    n0 = _native.launch_count()
    out = PW._mlp_bwd_chain_wgrad(g2d, z1, d(w1), d(w2), xd, st, d(ln_w), d(ln_b))
    assert _native.launch_count() - n0 >= 2
    out2 = PW._mlp_bwd_chain_wgrad(g2d, z1, d(w1), d(w2), xd, st, d(ln_w), d(ln_b))
    for a, b in zip(out, out2):
        assert torch.equal(a, b)
    names = ("gx1", "dgamma", "dbeta", "gw1", "gb1", "gw2", "gb2")
    refs = (gxc, ggc, gbc, gw1c, gb1c, gw2c, gb2c)
    why = "bf16 activation storage: gx1 is rounded once on store (2^-9 relative)" if bf else None
    for n, a, r in zip(names, out, refs):
        _cmp(a.float(), r, n, rtol=(4e-3 if n == "gx1" else 1e-4) if bf else 1e-4, why=why if (bf and n == "gx1") else None)


@pytest.mark.parametrize("bf", [False, True])
@pytest.mark.parametrize("ln", [False, True])
@pytest.mark.parametrize("B,S", [(2, (8, 8, 8)), (1, (6, 4, 5)), (3, (32, 32, 40))])
def test_gemm_dw_kernel(B, S, ln, bf):
    """fz_gemm_dw (gemm_dw_kernel): input gradient and weight (+ bias) gradient of a 32 -> 32 layer from one pass —
    out_proj form (y = Wᵀg, gw = Σ g ⊗ a, gb = Σ g) and in_proj form (LayerNorm backward on the accumulators + added
    gradient, gw against the LayerNorm OUTPUT γ x̂ + β, dγ / dβ).  Against CPU autograd; ragged tile (V = 120);
    at most 480 tiles, one per persistent workgroup (several: tests/test_gpu_mlp_chain.py); bit-identical when repeated."""
    torch.manual_seed(17 + B)
    C = 32
    rnd = (lambda t: t.bfloat16().float()) if bf else (lambda t: t)
    x = rnd(torch.randn(B, C, *S) * 1.5 + 0.3)
    g = rnd(torch.randn(B, C, *S))
    gadd = rnd(torch.randn(B, C, *S))
    w = torch.randn(C, C) * 0.2
    ln_w, ln_b = torch.rand(C) + 0.5, torch.randn(C) * 0.1
    xc, wc = x.clone().requires_grad_(True), w.clone().requires_grad_(True)
    lw, lb = ln_w.clone().requires_grad_(True), ln_b.clone().requires_grad_(True)
    if ln:
        inp = F.layer_norm(xc.movedim(1, -1), (C,), lw, lb, 1e-5).movedim(-1, 1)
        yc = _lin_cpu(inp, wc.unsqueeze(-1), None)
        gxc, gwc, ggc, gbc = torch.autograd.grad(yc, [xc, wc, lw, lb], g)
        gxc = gxc + gadd
    else:
        bc = torch.zeros(C, requires_grad=True)
        yc = _lin_cpu(xc, wc.unsqueeze(-1), bc)
        gxc, gwc, gbias_c = torch.autograd.grad(yc, [xc, wc, bc], g)
    dt = torch.bfloat16 if bf else torch.float32
    d = lambda t: t.to(DEV).contiguous()  # noqa: E731
    xd, gd, gaddd = d(x).to(dt), d(g).to(dt), d(gadd).to(dt)
    V = x[0, 0].numel()
    assert PW._dw_fused_ok(C, V)
    n0 = _native.launch_count()
    if ln:
        mean = xd.float().mean(1, keepdim=True)
        rstd = (xd.float().var(1, unbiased=False, keepdim=True) + 1e-5).rsqrt()
        st = torch.cat([mean, rstd], 1).reshape(B, 2, V).contiguous()
        run = lambda: PW._gemm_dw(gd, d(w), xd, ln=(d(ln_w), d(ln_b)), stats=st, gadd=gaddd)  # noqa: E731
    else:
        run = lambda: PW._gemm_dw(gd, d(w), xd, want_bias=True)  # noqa: E731
    y, gw, gb, gg, gbt = run()
    assert _native.launch_count() - n0 >= 2
    y2, gw2, gb2, gg2, gbt2 = run()
    assert torch.equal(y, y2) and torch.equal(gw, gw2)
    why = "bf16 activation storage: y is rounded once on store (2^-9 relative)" if bf else None
    _cmp(y.float(), gxc, "y", rtol=4e-3 if bf else 1e-4, why=why)
    _cmp(gw, gwc, "gw")
    if ln:
        _cmp(gg, ggc, "dgamma")
        _cmp(gbt, gbc, "dbeta")
    else:
        _cmp(gb, gbias_c, "gb")
        assert torch.equal(gb, gb2)


@pytest.mark.parametrize("C,Mz", [(32, 32), (32, 64), (64, 64)])
@pytest.mark.parametrize("B,S", [(2, (8, 8, 8)), (1, (6, 4, 5)), (2, (16, 32, 40))])
def test_dgrad_lnbwd_kernel(B, S, C, Mz):
    """fz_gemm with the LayerNorm-backward epilogue: gx = LNbwd(Wᵀ gz; x, stats, γ) + gadd, dγ, dβ — the resident kernel
    (LayerNorm width 32) and the SINGLE form of gemm_chain64_kernel (width 64, 64-channel gradient) — against CPU
    autograd of Linear∘LayerNorm."""
    torch.manual_seed(23 + C + Mz)
    x = torch.randn(B, C, *S) * 1.5 + 0.3
    gz, gadd = torch.randn(B, Mz, *S), torch.randn(B, C, *S)
    w = torch.randn(Mz, C) * 0.2
    ln_w, ln_b = torch.rand(C) + 0.5, torch.randn(C) * 0.1
    xc = x.clone().requires_grad_(True)
    lw, lb = ln_w.clone().requires_grad_(True), ln_b.clone().requires_grad_(True)
    yc = _lin_cpu(F.layer_norm(xc.movedim(1, -1), (C,), lw, lb, 1e-5).movedim(-1, 1), w.unsqueeze(-1), None)
    gxc, ggc, gbc = torch.autograd.grad(yc, [xc, lw, lb], gz)
    d = lambda t: t.to(DEV).contiguous()  # noqa: E731
    xd = d(x)
    V = x[0, 0].numel()
    st = torch.cat([xd.mean(1, keepdim=True), (xd.var(1, unbiased=False, keepdim=True) + 1e-5).rsqrt()], 1).reshape(B, 2, V).contiguous()
    n0 = _native.launch_count()
    gx, gg, gb = PW._dgrad_lnbwd(d(gz), d(w), xd, st, d(ln_w), d(gadd))
    assert _native.launch_count() > n0
    _cmp(gx, gxc + gadd, "gx")
    _cmp(gg, ggc, "dgamma")
    _cmp(gb, gbc, "dbeta")


def test_flat_adamw_kernel_matches_torch():
    """fz_adamw_step (csrc/optim.hip) against torch.optim.AdamW on the CPU: 5 steps over a 1 000 003-element
    buffer (odd length: vector body + scalar tail), lr 1e-4 / wd 1e-5 of train.yaml:72-76."""
    torch.manual_seed(0)
    n = 1_000_003
    p0 = torch.randn(n)
    ref = torch.nn.Parameter(p0.clone())
    dev = torch.nn.Parameter(p0.clone().to(DEV))
    o_ref = torch.optim.AdamW([ref], lr=1e-4, weight_decay=1e-5)
    o_dev = ft.FlatAdamW([dev], lr=1e-4, weight_decay=1e-5)
    n0 = _native.launch_count()
    for _ in range(5):
        g = torch.randn(n)
        ref.grad = g.clone()
        dev.grad = g.to(DEV)
        o_ref.step()
        o_dev.step()
    assert _native.launch_count() >= n0 + 5
    assert torch.allclose(dev.detach().cpu(), ref.detach(), rtol=1e-6, atol=1e-7)


def test_flat_adamw_skipped_parameter_subranges_are_aligned():
    """A parameter whose .grad is None splits the update into sub-range launches of the float4 kernel (torch skips such a
    parameter entirely: no decay, no moment update).  Odd-sized parameters (3, 5, 7 elements) in front make every later
    PACKED offset misaligned; the flat layout pads each parameter to a 16-byte boundary, so every sub-range is aligned and
    the result equals torch.optim.AdamW's on every parameter, 4 steps with the middle parameter unused in steps 1 and 2
    (both gradient orders: own layout and FlatGradSync's reversed views)."""
    from factorizer_amd.parallel import FlatGradSync
    for use_sync in (False, True):
        torch.manual_seed(3)
        shapes = [(3,), (5, 7), (1031,), (7,), (64, 33), (2,)]
        init = [torch.randn(*s) for s in shapes]
        ref = [torch.nn.Parameter(t.clone()) for t in init]
        mod = torch.nn.ParameterList([torch.nn.Parameter(t.clone().to(DEV)) for t in init])
        dev = list(mod)
        o_ref = torch.optim.AdamW(ref, lr=1e-3, weight_decay=1e-2)
        if use_sync:
            sync = FlatGradSync(mod, num_buckets=2, overlap=False)
            o_dev = ft.FlatAdamW(mod, lr=1e-3, weight_decay=1e-2, flat_grad=sync.flat, grad_views=sync.views)
        else:
            o_dev = ft.FlatAdamW(mod, lr=1e-3, weight_decay=1e-2)
        assert all(o % 4 == 0 for o in o_dev.offsets.values()) and o_dev.flat_param.data_ptr() % 16 == 0
        for step in range(4):
            for i, (r, d) in enumerate(zip(ref, dev)):
                if i == 2 and step in (1, 2):
                    r.grad, d.grad = None, None
                    continue
                g = torch.randn(*shapes[i])
                r.grad, d.grad = g.clone(), g.to(DEV)
            o_ref.step()
            o_dev.step()
        for i, (r, d) in enumerate(zip(ref, dev)):
            assert torch.allclose(d.detach().cpu(), r.detach(), rtol=1e-6, atol=1e-7), (use_sync, i)


@pytest.mark.parametrize("C,Hd,S,dt", [(64, 128, (8, 8, 16), torch.float32), (128, 256, (4, 8, 8), torch.float32),
                                       (64, 128, (8, 8, 16), torch.bfloat16), (48, 96, (4, 4, 8), torch.float32)])
def test_grouped_weight_gradients_equal_single_launches(C, Hd, S, dt):
    """fz_wgrad_group (csrc/wgrad.hip wgrad_fast_group_kernel): the four weight-gradient problems of a FactorizerBlock at
    C >= 64 — fc2 (GELU on the input side), fc1 behind LayerNorm (statistics + affine fold), out_proj, in_proj behind
    LayerNorm — in ONE partial-sum grid give bit for bit the gradients of the four single launches; a group that cannot
    use the 64 x 64 register-operand kernel (C = 48) runs the single launches in order."""
    torch.manual_seed(11)
    B, V = 2, S[0] * S[1] * S[2]
    r = lambda *s: torch.randn(*s, device=DEV).to(dt)  # noqa: E731
    g2, z1, gz1, x1, gx1, a, gt, x = r(B, C, *S), r(B, Hd, *S), r(B, Hd, *S), r(B, C, *S), r(B, C, *S), r(B, C, *S), r(B, C, *S), r(B, C, *S)
    st = torch.stack([torch.randn(B, V, device=DEV) * 0.1, torch.rand(B, V, device=DEV) + 0.5], 1).contiguous()
    lnw, lnb = torch.rand(C, device=DEV) + 0.5, torch.randn(C, device=DEV) * 0.1

    def problems(out):
        return [(g2, [z1], out["w2"], dict(B=B, M=C, Cin=Hd, K=Hd, Vq=V, Ncols=V, gbias=out["b2"], qact=PW.ACT["gelu"])),
                (gz1, [x1], out["w1"], dict(B=B, M=Hd, Cin=C, K=C, Vq=V, Ncols=V, gbias=out["b1"], stats=st, ln=(lnw, lnb))),
                (gx1, [a], out["wo"], dict(B=B, M=C, Cin=C, K=C, Vq=V, Ncols=V, gbias=out["bo"])),
                (gt, [x], out["wi"], dict(B=B, M=C, Cin=C, K=C, Vq=V, Ncols=V, stats=st, ln=(lnw, lnb)))]

    def outs():
        e = lambda *s: torch.full(s, float("nan"), device=DEV)  # noqa: E731
        return {"w2": e(C, Hd), "b2": e(C), "w1": e(Hd, C), "b1": e(Hd), "wo": e(C, C), "bo": e(C), "wi": e(C, C)}
    single, grouped = outs(), outs()
    for p, qs, gw, kw in problems(single):
        PW._wgrad(p, qs, gw, **kw)
    n0 = _native.launch_count()
    PW._wgrad_group(problems(grouped), "wgrad_block_test")
    assert _native.launch_count() > n0
    for k in single:
        assert torch.isfinite(grouped[k]).all(), k
        assert torch.equal(single[k], grouped[k]), k
    ref = torch.einsum("bmv,bkv->mk", g2.double().flatten(2), F.gelu(z1.float()).double().flatten(2))
    assert ((grouped["w2"].double() - ref).abs().max() / ref.abs().max()).item() < (1e-4 if dt == torch.float32 else 2e-2)


@pytest.mark.parametrize("C,Cd,S,bias_ad,dt", [(32, 64, (8, 8, 8), False, torch.float32), (64, 128, (4, 4, 8), True, torch.float32),
                                                (32, 64, (4, 8, 32), False, torch.float32), (32, 64, (2, 4, 64), True, torch.float32),
                                                (32, 64, (4, 8, 32), False, torch.bfloat16),
                                                (32, 64, (8, 8, 8), False, torch.bfloat16), (16, 32, (4, 4, 4), False, torch.float32)])
def test_up_cat_linear_node_vs_separate_nodes_and_fp64(C, Cd, S, bias_ad, dt):
    """pointwise.UpCatLinearFn — ConvTranspose3d(k2, s2) + virtual concat + adapter Linear as one autograd node whose
    backward works from the composed weights (unet.py:125-128, factorizer.py:116) — against (a) the two separate nodes it
    replaces (same forward kernels: identical output; gradients to rounding) and (b) a float64 evaluation of
    adapter(cat([skip, conv_transpose3d(deep)])) with autograd."""
    torch.manual_seed(4)
    B = 2
    fine = tuple(2 * d for d in S)
    skip = torch.randn(B, C, *fine)
    deep = torch.randn(B, Cd, *S)
    w_t = torch.randn(Cd, C, 2, 2, 2) * 0.2
    b_t = torch.randn(C) * 0.1
    w_ad = torch.randn(C, 2 * C, 1) * 0.2
    b_ad = torch.randn(C) * 0.1 if bias_ad else None
    g = torch.randn(B, C, *fine)
    # float64 reference
    r = [t.double().requires_grad_(True) for t in (skip, deep, w_t, b_t, w_ad)]
    rb = b_ad.double().requires_grad_(True) if bias_ad else None
    up = F.conv_transpose3d(r[1], r[2], r[3], stride=2)
    yr = F.conv1d(torch.cat([r[0], up], 1).flatten(2), r[4], rb).reshape(B, C, *fine)
    gr = torch.autograd.grad(yr, r + ([rb] if bias_ad else []), g.double())

    def dev_inputs():
        t = [v.to(DEV) for v in (skip, deep, w_t, b_t, w_ad)]
        t[0], t[1] = t[0].to(dt), t[1].to(dt)
        t = [v.requires_grad_(True) for v in t]
        bd = b_ad.to(DEV).requires_grad_(True) if bias_ad else None
        return t, bd
    (a, bd) = dev_inputs()
    n0 = _native.launch_count()
    y1 = PW.up_cat_linear(a[0], a[1], a[2], a[3], a[4], bd)
    assert _native.launch_count() > n0
    g1 = torch.autograd.grad(y1, a + ([bd] if bias_ad else []), g.to(DEV).to(dt))
    (c, bc) = dev_inputs()
    y2 = PW.CatLinearFn.apply(c[0], PW.TConvK2S2Fn.apply(c[1], c[2], c[3]), c[4], bc)
    g2 = torch.autograd.grad(y2, c + ([bc] if bias_ad else []), g.to(DEV).to(dt))
    tol = 1e-4 if dt == torch.float32 else 2e-2
    # (C = 32, 64 deep channels, rows of >= 64 fine voxels: one fused forward pass on composed weights, csrc/upcat.hip;
    # other shapes: the two forward launches of the separate nodes — identical output)
    assert (y1.double() - y2.double()).abs().max().item() <= (1e-5 if dt == torch.float32 else 2e-2) * yr.abs().max().item()
    assert (y1.double().cpu() - yr).abs().max().item() <= tol * yr.abs().max().item()
    names = ["skip", "deep", "w_t", "b_t", "w_ad"] + (["b_ad"] if bias_ad else [])
    for n, u, v, ref in zip(names, g1, g2, gr):
        scale = ref.abs().max().item() + 1e-30
        assert (u.double().cpu() - ref).abs().max().item() <= tol * scale, (n, "vs fp64")
        assert (u.double() - v.double()).abs().max().item() <= tol * scale, (n, "vs separate nodes")
    if dt == torch.float32:
        P.close(f"up_cat_linear {Cd}->{C} y", y1, yr.float())


@pytest.mark.parametrize("M", [1, 2, 3, 4])
@pytest.mark.parametrize("B,S,dt", [(2, (8, 8, 8), torch.float32), (1, (16, 16, 12), torch.float32), (3, (32, 32, 40), torch.float32),
                                   (2, (16, 16, 16), torch.bfloat16)])
def test_head_backward_one_pass_fp64(M, B, S, dt):
    """fz_head_bwd (csrc/headbwd.hip): backward of the network's head Linear(32 -> out_channels <= 4) (unet.py:253 through
    linear.py:53-58) — input, weight and bias gradient from one pass over (gy, x) — against a float64 evaluation."""
    torch.manual_seed(9)
    x = torch.randn(B, 32, *S)
    w = torch.randn(M, 32, 1) * 0.3
    b = torch.randn(M) * 0.1
    g = torch.randn(B, M, *S)
    xr, wr, br = (t.double().requires_grad_(True) for t in (x, w, b))
    yr = F.conv1d(xr.flatten(2), wr, br).reshape(B, M, *S)
    gr = torch.autograd.grad(yr, [xr, wr, br], g.double())
    xd = x.to(DEV).to(dt).requires_grad_(True)
    wd, bd = w.to(DEV).requires_grad_(True), b.to(DEV).requires_grad_(True)
    n0 = _native.launch_count()
    y = PW.linear_cf(xd, wd, bd)
    gd = torch.autograd.grad(y, [xd, wd, bd], g.to(DEV).to(dt))
    assert _native.launch_count() > n0
    tol = 1e-4 if dt == torch.float32 else 2e-2
    for n, u, r in zip(("gx", "gw", "gb"), gd, gr):
        assert (u.double().cpu() - r).abs().max().item() <= tol * (r.abs().max().item() + 1e-30), n


@pytest.mark.parametrize("M,B,S,dt,bias", [(3, 2, (32, 32, 32), torch.float32, True), (1, 1, (8, 12, 20), torch.float32, False),
                                          (4, 3, (8, 8, 8), torch.float32, True), (2, 2, (16, 16, 16), torch.bfloat16, True)])
def test_head_forward_valu_kernel_fp64(M, B, S, dt, bias):
    """fz_head_fwd (csrc/headbwd.hip): y = W x + b of the network's head Linear(32 -> out_channels <= 4) (unet.py:253) as 32·M
    FMAs per voxel, through the module path (fz_gemm dispatches to it) and through the entry point itself, against float64;
    a ragged quad count per workgroup (8·12·20 voxels), replay."""
    torch.manual_seed(10)
    x = torch.randn(B, 32, *S)
    w = torch.randn(M, 32, 1) * 0.3
    b = torch.randn(M) * 0.1 if bias else None
    yr = F.conv1d(x.double().flatten(2), w.double(), None if b is None else b.double()).reshape(B, M, *S)
    xd = x.to(DEV).to(dt)
    wd = w.to(DEV)
    bd = None if b is None else b.to(DEV)
    n0 = _native.launch_count()
    y = PW.linear_cf(xd, wd, bd)
    assert _native.launch_count() > n0
    y2 = torch.empty_like(y)
    V = S[0] * S[1] * S[2]
    _native.check(_native.lib().fz_head_fwd(xd.data_ptr(), wd.data_ptr(), 0 if bd is None else bd.data_ptr(), y2.data_ptr(), B, M, 32, V,
                                            _native.act_dtype(xd), _native.stream_ptr(xd)), "fz_head_fwd")
    assert torch.equal(y, y2)                      # the module path IS this kernel
    xq = xd.double().cpu()                         # (bf16: the stored input is the reference's input)
    yq = F.conv1d(xq.flatten(2), w.double(), None if b is None else b.double()).reshape(B, M, *S)
    tol = 1e-5 if dt == torch.float32 else 1e-2
    assert (y.double().cpu() - yq).abs().max().item() <= tol * yq.abs().max().item()
    assert (yq - yr).abs().max().item() <= (1e-12 if dt == torch.float32 else 5e-2) * yr.abs().max().item() + 1e-12
    assert _native.lib().fz_head_fwd(xd.data_ptr(), wd.data_ptr(), 0, y2.data_ptr(), B, 5, 32, V, _native.act_dtype(xd), _native.stream_ptr(xd)) != 0


def test_weight_gradients_land_in_the_flat_buffer():
    """With a FlatAdamW / FlatGradSync attached, every weight-gradient launch writes into its parameter's slice of the flat
    gradient buffer (factorizer_amd/gradbuf.py): after backward p.grad of every matrix / convolution weight IS that slice (no
    packing copy), the values equal the unattached run's bit for bit, a second backward without zero_grad accumulates
    (torch semantics), and the optimizer step equals the one taken from separately allocated gradients."""
    from factorizer_amd import gradbuf
    from factorizer_amd.parallel import FlatGradSync
    kw = dict(in_channels=4, out_channels=3, spatial_size=(32, 32, 32), encoder_depth=(1, 1, 1), encoder_width=(32, 64, 128),
              strides=(1, 2, 2), decoder_depth=(1, 1), norm=ft.LayerNorm, reshape=(ft.SWMatricize, {"head_dim": 8, "patch_size": 8}),
              act=torch.nn.ReLU, factorize=ft.NMF, rank=1, num_iters=5, init="uniform", solver="hals", mlp_ratio=2, dropout=0.0)
    torch.manual_seed(0)
    ref = ft.Factorizer(**kw).to(DEV)
    x = torch.rand(2, 4, 32, 32, 32, device=DEV)
    t = (torch.rand(2, 3, 32, 32, 32, device=DEV) > 0.5).float()
    ft.dice_ce_loss(ref(x), t).backward()
    g_ref = {n: p.grad.clone() for n, p in ref.named_parameters()}
    for with_sync in (False, True):
        torch.manual_seed(0)
        model = ft.Factorizer(**kw).to(DEV)
        if with_sync:
            sync = FlatGradSync(model, overlap=False)
            assert len(sync.buckets) >= 4
            opt = ft.FlatAdamW(model, lr=1e-3, flat_grad=sync.flat, grad_views=sync.views)
        else:
            opt = ft.FlatAdamW(model, lr=1e-3)
        opt.zero_grad()
        ft.dice_ce_loss(model(x), t).backward()
        in_place = 0
        for n, p in model.named_parameters():
            assert torch.equal(p.grad, g_ref[n]), n
            if p.grad.data_ptr() == opt.grad_views[p].data_ptr():
                in_place += p.numel()
            else:
                # (biases, LayerNorm parameters and the position embeddings — a batch sum formed by the framework — are packed)
                assert p.ndim == 1 or n.endswith("pos_embed.pos"), f"{n}: a weight gradient was produced outside the flat buffer"
        weights = sum(p.numel() for n, p in model.named_parameters() if p.ndim > 1 and not n.endswith("pos_embed.pos"))
        assert in_place >= weights > 0.5 * sum(p.numel() for p in model.parameters()), (in_place, weights)
        ft.dice_ce_loss(model(x), t).backward()          # no zero_grad: accumulate
        for n, p in model.named_parameters():
            assert torch.allclose(p.grad, 2 * g_ref[n], rtol=1e-6, atol=1e-9), n
            assert p.ndim == 1 or n.endswith("pos_embed.pos") or p.grad.data_ptr() == opt.grad_views[p].data_ptr(), n
        opt.zero_grad()
        ft.dice_ce_loss(model(x), t).backward()
        opt.step()
        o_ref = torch.optim.AdamW(ref.parameters(), lr=1e-3)
        o_ref.step()
        for (n, p), (_, q) in zip(model.named_parameters(), ref.named_parameters()):
            assert torch.allclose(p, q, rtol=1e-6, atol=1e-7), n
        torch.manual_seed(0)                             # a fresh reference for the second variant
        ref = ft.Factorizer(**kw).to(DEV)
        ft.dice_ce_loss(ref(x), t).backward()
        gradbuf.unregister(opt.flat_grad)


@pytest.mark.parametrize("M,K,S", [(64, 64, (16, 16, 16)), (128, 64, (8, 8, 16)), (64, 128, (8, 16, 16)), (32, 64, (16, 16, 16)),
                                   (3, 32, (8, 8, 12))])
def test_wgrad_split_bf16_mode(M, K, S):
    """The weight-gradient kernels (register-operand and generic) form each fp32 product from a three-level bf16 split of both
    operands: six exact bf16 products on the bf16 matrix pipe, fp32 accumulation (the default; csrc/wgrad.hip BF = 6).
    Against float64 its error must be at the level of the fp32-MFMA kernels' own (products = FZ_PRODUCTS_FP32_MFMA): both <= 2e-6 of
    the largest entry, the split form within 1.5x of the fp32 form (different summation order: + one rounding)."""
    torch.manual_seed(5)
    V = S[0] * S[1] * S[2]
    p = torch.randn(2, M, V, device=DEV)
    q = torch.randn(2, K, V, device=DEV)
    ref = torch.einsum("bmv,bkv->mk", p.double(), q.double())
    errs = {}
    assert _native.lib().fz_gemm_bx_enable(-1) == 1                      # the process default stays untouched ...
    for mode, prod in ((0, _native.PRODUCTS_FP32_MFMA), (1, _native.PRODUCTS_SPLIT_BF16)):
        with _native.use_products(prod):                                  # ... the descriptor's own field selects the pipe
            gw = torch.empty(M, K, device=DEV)
            gb = torch.empty(M, device=DEV)
            PW._wgrad(p, [q], gw, B=2, M=M, Cin=K, K=K, Vq=V, Ncols=V, gbias=gb)
        errs[mode] = ((gw.double() - ref).abs().max() / ref.abs().max()).item()
        assert torch.allclose(gb.double(), p.double().sum((0, 2)), rtol=1e-4, atol=1e-3)
    assert _native.lib().fz_gemm_bx_enable(-1) == 1
    P.note(f"wgrad {M}x{K}", err_f32_mfma=errs[0], err_split_bf16=errs[1])
    assert errs[0] <= 2e-6 and errs[1] <= max(1.5 * errs[0], 3e-7), errs


# ---- no silent composed-ATen path on device ------------------------------------------
def _fallback_cases():
    g = lambda *s: torch.randn(*s, device=DEV)  # noqa: E731
    odd, v3 = g(1, 5, 4, 4, 4), g(1, 8, 3, 3, 3)          # odd C_in; V = 27 (not a multiple of 4)
    return {
        "linear odd C_in": lambda: PW.linear_cf(odd, g(4, 5, 1), g(4)),
        "linear V%4": lambda: PW.linear_cf(v3, g(4, 8, 1), None),
        "linear fp16": lambda: PW.linear_cf(g(1, 8, 4, 4, 4).half(), g(4, 8, 1).half(), None),
        "layernorm V%4": lambda: PW.layernorm_cf(v3, g(8), g(8), 1e-5),
        "mlp odd": lambda: PW.mlp_cf(odd, g(6, 5, 1), g(6), g(5, 6, 1), g(5)),
        "ln_linear odd": lambda: PW.ln_linear(odd, g(5), g(5), 1e-5, g(4, 5, 1), None, "relu"),
        "act_linear_res odd": lambda: PW.act_linear_res(odd, g(5, 5, 1), g(5), odd, "gelu"),
        "cat_linear odd": lambda: PW.cat_linear(odd, odd, g(4, 10, 1), None),
        "stem input gradient": _stem_gx,
        "dice_ce fp64": lambda: ft.dice_ce_loss(g(1, 3, 4, 4, 4).double(), g(1, 3, 4, 4, 4).double()),
    }


def _stem_gx():
    x = torch.randn(1, 4, 4, 4, 8, device=DEV, requires_grad=True)
    w = torch.randn(7, 4, 3, 3, 3, device=DEV)            # odd C_out: outside the tap loader of the adjoint GEMM
    (gx,) = torch.autograd.grad(PW.ConvK3Fn.apply(x, w, None).sum(), x)
    return gx


@pytest.mark.parametrize("name", sorted(["linear odd C_in", "linear V%4", "linear fp16", "layernorm V%4", "mlp odd",
                                         "ln_linear odd", "act_linear_res odd", "cat_linear odd",
                                         "stem input gradient", "dice_ce fp64"]))
def test_every_composed_device_branch_warns(name):
    from factorizer_amd import composed
    composed._warned.clear()
    with pytest.warns(RuntimeWarning, match="composed framework ops|outside the native kernel set"):
        out = _fallback_cases()[name]()
    assert torch.isfinite(out.float()).all()


@pytest.mark.parametrize("B,C,O,S", [(2, 4, 32, (8, 8, 16)), (1, 2, 8, (4, 6, 8)), (1, 4, 6, (5, 3, 12))])
def test_stem_input_gradient_native(B, C, O, S):
    """Conv3d(k3, p1) input gradient = the k3 correlation of gy with the channel-transposed, flipped filters through the
    tap loader of the GEMM family (no framework op, no warning)."""
    import warnings
    torch.manual_seed(O)
    x, w = torch.randn(B, C, *S), torch.randn(O, C, 3, 3, 3) / (27 * C) ** 0.5
    xc = x.clone().requires_grad_(True)
    yc = F.conv3d(xc, w, None, padding=1)
    gy = torch.randn_like(yc)
    (gxc,) = torch.autograd.grad(yc, xc, gy)
    xd = x.to(DEV).requires_grad_(True)
    with warnings.catch_warnings():
        warnings.simplefilter("error", RuntimeWarning)
        yd = PW.ConvK3Fn.apply(xd, w.to(DEV), None)
        (gxd,) = torch.autograd.grad(yd, xd, gy.to(DEV))
    _cmp(yd, yc, "y")
    _cmp(gxd, gxc, "gx")


def test_odd_channel_stem_runs_native():
    """in_channels 1 / 3 (ISLES / BraTS variants of the stem, factorizer.py:145-149): the native stem kernels on a
    zero-padded channel, no warning; values and gradients against ATen."""
    import warnings
    for cin in (1, 3):
        torch.manual_seed(cin)
        conv = ft.Conv3d(cin, 8, 3, padding=1, bias=False)
        x = torch.randn(2, cin, 8, 8, 8)
        ref = F.conv3d(x, conv.weight, None, padding=1)
        gy = torch.randn_like(ref)
        (gw_ref,) = torch.autograd.grad(ref, conv.weight, gy)
        convd = ft.Conv3d(cin, 8, 3, padding=1, bias=False).to(DEV)
        convd.load_state_dict(conv.state_dict())
        n0 = _native.launch_count()
        with warnings.catch_warnings():
            warnings.simplefilter("error", RuntimeWarning)
            y = convd(x.to(DEV))
            (gw,) = torch.autograd.grad(y, convd.weight, gy.to(DEV))
        assert _native.launch_count() > n0
        _cmp(y, ref, f"stem C_in={cin} forward")
        _cmp(gw, gw_ref, f"stem C_in={cin} weight gradient")


def test_no_composed_branch_on_baseline_configs():
    """BASELINE configs[1..4] shapes (reduced extents where only the extent differs) raise no fallback warning:
    RuntimeWarning is an error inside this test."""
    import warnings

    from factorizer_amd import composed
    composed._warned.clear()
    kw = dict(norm=ft.LayerNorm, act=nn.ReLU, factorize=ft.NMF, init="uniform", solver="hals", dropout=0.0)
    with warnings.catch_warnings():
        warnings.simplefilter("error", RuntimeWarning)
        # cfg 2: FactorizerBlock C=32, d=8, p=8, HALS R1 T5 (B = 1 and 2)
        blk = ft.FactorizerBlock(channels=32, spatial_size=(32, 32, 32), reshape=(ft.SWMatricize, {"head_dim": 8, "patch_size": 8}),
                                 rank=1, num_iters=5, mlp_ratio=2, **kw).to(DEV)
        for B in (1, 2):
            x = torch.rand(B, 32, 32, 32, 32, device=DEV, requires_grad=True)
            blk(x).sum().backward()
        # cfg 3 / 4: README model, training step with the recipe's loss and the flat optimizer
        model = ft.Factorizer(in_channels=4, out_channels=3, spatial_size=(128, 128, 128),
                              reshape=(ft.SWMatricize, {"head_dim": 8, "patch_size": 8}), rank=1, num_iters=5,
                              mlp_ratio=2, **{**kw, "dropout": 0.1}).to(DEV)
        opt = ft.FlatAdamW(model, lr=1e-4, weight_decay=1e-5)
        x = torch.rand(1, 4, 128, 128, 128, device=DEV)
        t = (torch.rand(1, 3, 128, 128, 128, device=DEV) > 0.5).float()
        with torch.no_grad():
            model.eval()(x)
        ft.dice_ce_loss(model.train()(x), t).backward()
        opt.step()
        del model, opt
        # cfg 5: anisotropic patch (5,6,5), R = 2, T = 10 (fp32 here; the bf16 leg has its own test)
        blk5 = ft.FactorizerBlock(channels=32, spatial_size=(20, 24, 20), reshape=(ft.SWMatricize, {"head_dim": 8, "patch_size": (5, 6, 5)}),
                                  rank=2, num_iters=10, mlp_ratio=2, **kw).to(DEV)
        x = torch.rand(2, 32, 20, 24, 20, device=DEV, requires_grad=True)
        blk5(x).sum().backward()
    torch.cuda.synchronize()


@pytest.mark.parametrize("bf", [False, True])
@pytest.mark.parametrize("producer", ["stem", "upcat"])
def test_block_prologue_inside_the_producing_launch(producer, bf):
    """t = relu(in_proj(LayerNorm1(x))) (factorizer.py:38,44,75; norm.py:29-34) formed by the launch that PRODUCES x — the stem
    convolution (factorizer.py:145-149; fz_conv3_fwd2) or a decoder level's transposed convolution + concat + adapter
    (unet.py:125-127; fz_upcat2) — against the separate launch it replaces: x bit-identical (the producer's arithmetic is
    unchanged), t and the LayerNorm statistics to 1e-5 (another product path for the 32 -> 32 layer) and against float64."""
    torch.manual_seed(23)
    dt = torch.bfloat16 if bf else torch.float32
    d = lambda t: t.to(DEV).contiguous()  # noqa: E731
    ln_w, ln_b, w_in = torch.rand(32) + 0.5, torch.randn(32) * 0.1, torch.randn(32, 32, 1) * 0.2
    pro = (d(ln_w), d(ln_b), 1e-5, d(w_in))
    if producer == "stem":
        x0 = torch.randn(2, 4, 8, 12, 64)
        w, b = torch.randn(32, 4, 3, 3, 3) * 0.1, None
        x0d = d(x0).to(dt)
        assert PW.conv3_prologue_ok(x0d, d(w))
        n0 = _native.launch_count()
        y, t, st = PW.ConvK3Fn.apply(x0d, d(w), b, pro)
        assert _native.launch_count() - n0 == 1
        y_ref = PW.ConvK3Fn.apply(x0d, d(w), b, None)
    else:
        skip, deep = torch.randn(2, 32, 4, 8, 64), torch.randn(2, 64, 2, 4, 32)
        w_t, b_t = torch.randn(64, 32, 2, 2, 2) * 0.1, torch.randn(32) * 0.1
        w_ad, b_ad = torch.randn(32, 64, 1) * 0.1, torch.randn(32) * 0.1
        sd, dd = d(skip).to(dt), d(deep).to(dt)
        assert PW.upcat_prologue_ok(sd, dd, d(w_t), d(w_ad))
        y, t, st = PW.up_cat_linear(sd, dd, d(w_t), d(b_t), d(w_ad), d(b_ad), pro)
        y_ref = PW.up_cat_linear(sd, dd, d(w_t), d(b_t), d(w_ad), d(b_ad), None)
    assert torch.equal(y, y_ref)
    # the launch it replaces, on the stored x
    t_ref = PW.ln_linear(y_ref, d(ln_w), d(ln_b), 1e-5, d(w_in), None, "relu")
    # float64 on the stored x
    xs = y_ref.float().cpu().double()
    xn = F.layer_norm(xs.movedim(1, -1), (32,), ln_w.double(), ln_b.double(), 1e-5).movedim(-1, 1)
    t64 = torch.relu(_lin_cpu(xn, w_in.double()))
    B = xs.shape[0]
    if bf:
        _cmp(t.float(), t64.float(), "t (bf16 storage)", rtol=2.0 ** -8, why="bf16 storage: one rounding of the stored tensor")
        assert (t.float() - t_ref.float()).abs().max().item() <= 2.0 ** -7 * t_ref.float().abs().max().item()
    else:
        _cmp(t, t64.float(), "t vs float64")
        _cmp(t, t_ref, "t one launch vs two", rtol=1e-5)
    _cmp(st[:, 0], xs.mean(1).reshape(B, -1).float(), "mean")
    _cmp(st[:, 1], (1.0 / torch.sqrt(xs.var(1, unbiased=False) + 1e-5)).reshape(B, -1).float(), "rstd")
