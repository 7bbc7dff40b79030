"""-m gpu: split-N NMF for ranks up to 32 and matrices up to 512 rows (csrc/nmf_global_rank.hip) — the matrices of the
reference's default-constructed model (Matricize(num_heads=1, grid_size=1), rank=None): forward and backward against the
float64 oracle on the planted family of tests/wide_rank_cases.py, launch counts, decompose, bitwise replay and batch
independence, zero rows and columns, a block, and the default model itself."""
import copy
import warnings

import pytest
import torch

import factorizer_amd as ft
import parity as P
import wide_rank_cases as W
from factorizer_amd import _native
from factorizer_amd import functional as Fn
from oracle import cpu_ref as O

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _module(M, N, R, T, G, solver, u0, v0):
    nmf = ft.NMF(size=(M, N), rank=R, num_iters=T, num_grad_steps=G, init="uniform", solver=solver)
    nmf.load_state_dict({"init.u0": u0, "init.v0": v0})
    return nmf


def _run(nd, x, gy, M, N, R, T, G):
    """y, gx of the device module with every RuntimeWarning an error and the launch counter held to fz_gnmfx_launches"""
    lib = _native.lib()
    Gs = T if G is None else G
    xd = x.to(DEV).requires_grad_(True)
    n0 = _native.launch_count()
    with warnings.catch_warnings():
        warnings.simplefilter("error", RuntimeWarning)
        y = nd(xd)
    torch.cuda.synchronize()
    assert nd._wide == "gnmfx"
    assert _native.launch_count() - n0 == lib.fz_gnmfx_launches(M, N, R, T, Gs, 0)
    n1 = _native.launch_count()
    (gx,) = torch.autograd.grad(y, xd, gy.to(DEV))
    torch.cuda.synchronize()
    assert _native.launch_count() - n1 == lib.fz_gnmfx_launches(M, N, R, T, Gs, 1)
    return y, gx


@pytest.mark.parametrize("M,N,R,T,G,solver", W.PAIRS, ids=W.IDS)
def test_wide_rank_vs_float64(M, N, R, T, G, solver):
    ref = W.guard(M, N, R, T, G, solver)         # the inputs are well conditioned (asserted, never skipped)
    x, u0, v0, gy = W.inputs(M, N, R)
    assert Fn.gnmfx_supported(M, N, R, T, T if G is None else G)
    y, gx = _run(_module(M, N, R, T, G, solver, u0, v0).to(DEV), x, gy, M, N, R, T, G)
    tag = f"{M}x{N} R{R} T{T} G{G} {solver}"
    P.close(f"y {tag} (vs fp64 oracle)", y, ref["y64"], extra=ref["y_kink"])
    P.close(f"gx {tag} (vs fp64 oracle)", gx, ref["gx64"], extra=ref["gx_kink"])
    assert (y >= 0).all()


def test_decompose_and_factor_gradients():
    M, N, R, T, solver = 64, 1024, 7, 4, "hals"
    W.guard(M, N, R, T, None, solver)
    x, u0, v0, _ = W.inputs(M, N, R)
    nd = _module(M, N, R, T, None, solver, u0, v0).to(DEV)
    xd = x.to(DEV).requires_grad_(True)
    with warnings.catch_warnings():
        warnings.simplefilter("error", RuntimeWarning)
        u, v = nd.decompose(xd)
    uo, vo = O.nmf_decompose(x, u0, v0, T, solver)
    P.close("u", u, uo)
    P.close("v", v, vo)
    torch.manual_seed(5)
    gu, gv = torch.rand(u.shape), torch.rand(v.shape)
    (gxd,) = torch.autograd.grad([u, v], xd, [gu.to(DEV), gv.to(DEV)])
    xc = x.double().requires_grad_(True)          # the CPU module (composed path) in float64
    nc = _module(M, N, R, T, None, solver, u0, v0).double()
    uc, vc = nc.decompose(xc)
    (gxc,) = torch.autograd.grad([uc, vc], xc, [gu.double(), gv.double()])
    x32 = x.clone().requires_grad_(True)          # ... and in fp32: its own distance to float64
    u32, v32 = _module(M, N, R, T, None, solver, u0, v0).decompose(x32)
    (gx32,) = torch.autograd.grad([u32, v32], x32, [gu, gv])
    P.close("gx from (gu, gv)", gxd, gxc, extra=(gx32.double() - gxc).abs().max().item())


@pytest.mark.parametrize("M,N,R,solver", [(128, 2052, 13, "hals"), (512, 520, 26, "mu"), (16, 777, 5, "hals"),
                                          (64, 8200, 7, "hals")])
def test_bitwise_replay_and_batch_independence(M, N, R, solver):
    T = 4
    x, u0, v0, gy = W.inputs(M, N, R)
    nd = _module(M, N, R, T, None, solver, u0, v0).to(DEV)
    torch.manual_seed(3)
    x3 = torch.cat([x[:1], torch.rand(2, M, N)])             # matrix 0 with two unrelated neighbours
    gy3 = torch.cat([gy[:1], torch.rand(2, M, N)])
    outs = []
    for xs, gs in ((x3, gy3), (x3, gy3), (x[:1], gy[:1])):
        xd = xs.to(DEV).requires_grad_(True)
        y = nd(xd)
        (gx,) = torch.autograd.grad(y, xd, gs.to(DEV))
        outs.append((y.detach().view(torch.int32).cpu(), gx.view(torch.int32).cpu()))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])           # replay: identical bits
    assert torch.equal(outs[0][0][:1], outs[2][0]) and torch.equal(outs[0][1][:1], outs[2][1])   # batch of 3 vs batch of 1


def test_zero_rows_and_columns():
    """a block of zero columns, zero rows and one all-zero matrix (MU: eps keeps every ratio finite)"""
    M, N, R, T, solver = 128, 2052, 13, 4, "mu"
    x, u0, v0, gy = W.inputs(M, N, R)
    x = torch.cat([x, torch.zeros(1, M, N)])
    x[0, :, 1000:1100] = 0
    x[1, 60:70, :] = 0
    gy = torch.cat([gy, gy[:1]])
    y, gx = _run(_module(M, N, R, T, None, solver, u0, v0).to(DEV), x, gy, M, N, R, T, None)
    assert torch.isfinite(y).all() and torch.isfinite(gx).all()
    d = lambda t: t.double()
    y64 = O.nmf_forward(d(x), d(u0), d(v0), T, solver)
    gx64 = O.nmf_backward(d(x), d(u0), d(v0), d(gy), T, solver)
    yk = (O.nmf_forward(x, u0, v0, T, solver).double() - y64).abs().max().item()
    gk = (O.nmf_backward(x, u0, v0, gy, T, solver).double() - gx64).abs().max().item()
    P.close("y with zero blocks", y, y64, extra=yk)
    P.close("gx with zero blocks", gx, gx64, extra=gk)


def _against_cpu_module(model, x, what, input_grad=True, f64=False):
    """y, (gx) and every parameter gradient of `model` on the device against the same module on the CPU (composed
    path); no RuntimeWarning on the device.  f64: the CPU module runs in float64 and the fp32 CPU module's own distance
    to it is added to each bound (the reference's error, as in test_wide_rank_vs_float64)."""
    names = [n for n, _ in model.named_parameters()]

    def cpu(m, xin, gy):
        xc = xin.clone().requires_grad_(True)
        yc = m(xc)
        gy = torch.rand_like(yc) if gy is None else gy.to(yc.dtype)
        return yc, gy, torch.autograd.grad(yc, [xc, *m.parameters()], gy)

    y32, gy, g32 = cpu(model, x, None)
    yc, gc, extra = y32, g32, [0.0] * (len(g32) + 1)
    if f64:
        yc, _, gc = cpu(copy.deepcopy(model).double(), x.double(), gy)
        extra = [(a.double() - b).abs().max().item() for a, b in zip((y32, *g32), (yc, *gc))]
    model = model.to(DEV)
    xd = x.to(DEV).requires_grad_(True)
    n0 = _native.launch_count()
    with warnings.catch_warnings():
        warnings.simplefilter("error", RuntimeWarning)
        yd = model(xd)
        gd = torch.autograd.grad(yd, [xd, *model.parameters()], gy.to(DEV))
    assert _native.launch_count() > n0
    P.close(f"{what} y", yd, yc, extra=extra[0])
    for n, a, b, e in list(zip(["x", *names], gd, gc, extra[1:]))[0 if input_grad else 1:]:
        P.close(f"{what} d{n}", a, b, extra=e)
    return model


def test_block_with_rank_rule():
    """Matricize(num_heads=1, grid_size=1) at C = 64, 16^3: 64 x 4096, rank=None -> 7, inside a block (the comparison of
    tests/test_gpu_wide_nmf.py::test_num_heads_8_block_m_not_8)"""
    torch.manual_seed(1)
    blk = ft.FactorizerBlock(64, (16, 16, 16), reshape=(ft.Matricize, {"num_heads": 1, "grid_size": 1}), rank=None,
                             solver="mu")
    assert blk.fact.factorize.size == (64, 4096) and blk.fact.factorize.rank == 7
    blk = _against_cpu_module(blk, torch.rand(2, 64, 16, 16, 16), "block 64x4096 R7")
    assert blk.fact.factorize._wide == "gnmfx"


def _nmfs(model):
    return [m for m in model.modules() if isinstance(m, ft.NMF)]


def test_default_model_mu():
    """ft.Factorizer(4, 3, 32^3) as constructed but for solver="mu": stages 32 x 32 768 R 4 (the R <= 4 family),
    64 x 4096 R 7, 128 x 512 R 11, 256 x 64 R 6, 512 x 8 R 1 (the N = 8 edge) — all native, against the CPU module"""
    torch.manual_seed(2)
    model = ft.Factorizer(4, 3, (32, 32, 32), solver="mu")
    shapes = sorted({(*m.size, m.rank) for m in _nmfs(model)})
    assert shapes == [(32, 32768, 4), (64, 4096, 7), (128, 512, 11), (256, 64, 6), (512, 8, 1)], shapes
    # (output and parameter gradients; the input gradient also passes the stem convolution's, which is not this family's)
    model = _against_cpu_module(model, torch.rand(1, 4, 32, 32, 32), "default model (mu)", input_grad=False, f64=True)
    assert sorted({m._wide for m in _nmfs(model)}) == ["gnmf", "gnmfx"]


def test_default_model_as_constructed_hals():
    """The default constructor itself (HALS).  No value bound: at these ranks the reference's own HALS arithmetic is
    chaotic in fp32 on such activations (components die, b[r][r] + eps ~ eps, gate decisions flip: the fp32 oracle
    differs from the float64 oracle by tens of per cent, tests/wide_rank_cases.py), so no reference exists to compare
    with.  What holds: every NMF runs natively (no warning), the output is finite, and forward and backward replay bit
    for bit (compared as integers: gradients may legitimately be non-finite)."""
    torch.manual_seed(2)
    model = ft.Factorizer(4, 3, (32, 32, 32)).to(DEV)
    x = torch.rand(1, 4, 32, 32, 32)
    gy = torch.rand(1, 3, 32, 32, 32)
    runs = []
    for _ in range(2):
        xd = x.to(DEV).requires_grad_(True)
        with warnings.catch_warnings():
            warnings.simplefilter("error", RuntimeWarning)
            y = model(xd)
            grads = torch.autograd.grad(y, [xd, *model.parameters()], gy.to(DEV))
        assert torch.isfinite(y).all()
        runs.append([t.detach().contiguous().view(torch.int32).cpu() for t in (y, *grads)])
    assert all(m._wide in ("gnmf", "gnmfx") for m in _nmfs(model))
    for a, b in zip(*runs):
        assert torch.equal(a, b)
