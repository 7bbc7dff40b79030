"""-m gpu: the native cd and smu solvers (csrc/nmf_core.h SOLVER_CD / SOLVER_SMU) in every wave-program kernel family — the
standalone ft.NMF kernels (nmf_r*_cdsmu.hip), the split-N kernels for wide matrices (nmf_global.hip), the 8^3 fused core
(nmf_cf_fwd.hip, nmf_cf_bwd.hip) and the generic-patch fused core (nmf_pcf.hip) — against the reference's goldens (g8, g11) and the package's composed
path in float64.  Every test asserts that native kernels ran."""
import copy
import re
import warnings

import numpy as np
import pytest
import torch
from torch import nn

import factorizer_amd as ft
from factorizer_amd import _native
from factorizer_amd import functional as Fn

import parity as P
from test_nmf_solvers_cpu import _g11_names, composed

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


class Launches:
    """Asserts that the native library launched kernels inside the block."""

    def __enter__(self):
        self.n0 = _native.launch_count()
        return self

    def __exit__(self, *a):
        torch.cuda.synchronize()
        assert _native.launch_count() > self.n0, "native kernels were not launched"


def _kink(ref32, ref64):
    """fp32-vs-float64 disagreement of the composed path: the conditioning guard of the bounds below (30x, as in
    test_wave_program_emul.py::test_emul_vs_oracle_shapes)"""
    return 30.0 * (ref32.double() - ref64).abs().max().item()


def _mf(M, N, R, T, G, solver, u0, v0):
    mf = ft.MatrixFactorization((M, N), rank=R, init="uniform", solver=solver, num_iters=T, num_grad_steps=G)
    mf.init.u0.copy_(u0)
    mf.init.v0.copy_(v0)
    return mf.to(DEV)


def _check_standalone(name, x, u0, v0, T, G, solver, gy, guards=None):
    """`guards`: a list that receives (what, the guard, the bound of P.close without the guard) of every comparison"""
    M, N = x.shape[-2:]
    R = u0.shape[1]
    mf = _mf(M, N, R, T, G, solver, u0, v0)

    def close(what, got, ref64, ref32):
        if guards is not None:
            guards.append((what, _kink(ref32, ref64), 1e-4 * ref64.float().abs().max().item() + 1e-6))
        P.close(f"{name}: {what}", got, ref64, extra=_kink(ref32, ref64))

    y64, u64, v64, gx64 = composed(x, u0, v0, T, G, solver, gy=gy)
    y32, u32, v32, gx32 = composed(x, u0, v0, T, G, solver, gy=gy, dtype=torch.float32)
    xd = x.to(DEV).requires_grad_(True)
    with Launches():
        y = mf(xd)
        (gx,) = torch.autograd.grad(y, xd, gy.to(DEV))
    close("y", y, y64, y32)
    close("gx", gx, gx64, gx32)
    # decompose(): u and v, with gradients into both
    gu, gv = torch.rand_like(u64.float()) - 0.5, torch.rand_like(v64.float()) - 0.5
    _, _, _, gxd64 = composed(x, u0, v0, T, G, solver, gu=gu, gv=gv)
    _, _, _, gxd32 = composed(x, u0, v0, T, G, solver, gu=gu, gv=gv, dtype=torch.float32)
    xd = x.to(DEV).requires_grad_(True)
    with Launches():
        u, v = mf.decompose(xd)
        (gxd,) = torch.autograd.grad([u, v], xd, [gu.to(DEV), gv.to(DEV)])
    close("u", u, u64, u32)
    close("v", v, v64, v32)
    close("gx (decompose)", gxd, gxd64, gxd32)
    return mf


@pytest.mark.parametrize("name", _g11_names())
def test_standalone_g11(golden, name):
    g = golden("g11_solvers").case(name)
    solver = "cd" if name.startswith("cd") else "smu"
    T, G = (int(v) for v in re.search(r"_t(\d+)_g(\d+)$", name).groups())
    mf = _check_standalone(name, g["x"], g["u0"], g["v0"], T, G, solver, g["gy"])
    # the reference's own fp32 outputs, at the bound of the float64 comparison widened by the reference's own rounding
    y64, _, _, gx64 = composed(g["x"], g["u0"], g["v0"], T, G, solver, gy=g["gy"])
    xd = g["x"].to(DEV).requires_grad_(True)
    y = mf(xd)
    (gx,) = torch.autograd.grad(y, xd, g["gy"].to(DEV))
    P.close(f"{name}: y vs reference", y, g["y"], extra=_kink(g["y"], y64))
    P.close(f"{name}: gx vs reference", gx, g["gx"], extra=_kink(g["gx"], gx64))
    # run-to-run bitwise determinism
    y2 = mf(xd)
    (gx2,) = torch.autograd.grad(y2, xd, g["gy"].to(DEV))
    assert torch.equal(y, y2) and torch.equal(gx, gx2)


@pytest.mark.parametrize("name", ["cd", "smu"])
def test_standalone_g8(golden, name):
    """the reference's own cd / smu outputs of goldens g8 ((3, 8, 24), rank 2, 3 iterations): u, v, y, dL/dx"""
    g = golden("g8_solvers").case(name)
    torch.manual_seed(0)
    mf = ft.MatrixFactorization(size=(8, 24), rank=2, num_iters=3, solver=name,
                                init="normal" if name == "cd" else "uniform")
    mf.init.u0.copy_(g["u_init"][0])
    mf.init.v0.copy_(g["v_init"][0])
    mf = mf.to(DEV)
    x = g["x"].to(DEV).requires_grad_(True)
    with Launches():
        u, v = mf.decompose(x)
        y = mf(x)
        (gx,) = torch.autograd.grad(y, x, g["gy"].to(DEV))
    P.close("u", u, g["u"])
    P.close("v", v, g["v"])
    P.close("y", y, g["y"])
    P.close("gx", gx, g["gx"])


@pytest.mark.parametrize("solver", ["cd", "smu"])
@pytest.mark.parametrize("M,N,R", [(8, 512, 2), (8, 150, 1), (5, 100, 4)])
def test_standalone_bf16_storage(solver, M, N, R):
    """bf16 storage of X / Y / dL/dY / dL/dX, fp32 factors: against the fp32 native result, in units of 2^-8 (test_gpu_bf16.py)"""
    torch.manual_seed(M + N + R)
    x = torch.rand(64, M, N) if solver == "cd" else torch.randn(64, M, N)
    mf = _mf(M, N, R, 5, 5, solver, torch.rand(M, R), torch.rand(N, R))
    xb = x.to(DEV).to(torch.bfloat16)
    xf = xb.float().requires_grad_(True)
    gy = (torch.rand(64, M, N, device=DEV) - 0.5).to(torch.bfloat16)
    with Launches():
        yf = mf(xf)
        (gxf,) = torch.autograd.grad(yf, xf, gy.float())
        xb.requires_grad_(True)
        yb = mf(xb)
        (gxb,) = torch.autograd.grad(yb, xb, gy)
    assert yb.dtype == torch.bfloat16 and gxb.dtype == torch.bfloat16
    P.close("y (bf16 storage)", yb, yf, rel=2 * 2.0 ** -8, why="bf16 rounding of the stored output")
    P.close("gx (bf16 storage)", gxb, gxf, rel=2 * 2.0 ** -8, why="bf16 rounding of the stored gradient")


TABLE_SOLVERS = ("mu", "hals", "cd", "smu")
TABLE_SEED = 63   # of seeds 0..70 the one with the best-conditioned inputs: on the CPU every guard below is under a third of its bound


def _table_inputs(solver, R):
    """3 matrices of 5 x 40 (a partial workgroup; the first row of the shape table with padding in both extents), T = 3, G = 2"""
    torch.manual_seed(TABLE_SEED + 10 * TABLE_SOLVERS.index(solver) + R)
    x = torch.randn(3, 5, 40) if solver == "smu" else torch.rand(3, 5, 40)
    return x, torch.rand(5, R), torch.rand(40, R), torch.rand(3, 5, 40) - 0.5


@pytest.mark.parametrize("R", [1, 2, 3, 4])
@pytest.mark.parametrize("solver", TABLE_SOLVERS)
def test_launcher_table_fp32(solver, R):
    """every (solver unit, rank) of the launcher table of csrc/nmf.hip, both directions, fp32 storage: a swapped entry is another
    rank, solver or direction, i.e. other values.  The conditioning guard of every comparison stays below the bound it is
    added to, so it cannot hide that."""
    x, u0, v0, gy = _table_inputs(solver, R)
    assert Fn.nmf_supported(5, 40, R, 3, 2)
    guards = []
    _check_standalone(f"{solver} R{R}", x, u0, v0, 3, 2, solver, gy, guards=guards)
    assert len(guards) == 5
    for what, kink, base in guards:
        assert kink <= base, (solver, R, what, kink, base)


@pytest.mark.parametrize("R", [1, 2, 3, 4])
@pytest.mark.parametrize("solver", TABLE_SOLVERS)
def test_launcher_table_bf16(solver, R):
    """the bf16 half of the table: against the fp32 native result on the same rounded inputs, in units of 2^-8"""
    x, u0, v0, gy = _table_inputs(solver, R)
    mf = _mf(5, 40, R, 3, 2, solver, u0, v0)
    xb = x.to(DEV).to(torch.bfloat16)
    xf = xb.float().requires_grad_(True)
    gy = gy.to(DEV).to(torch.bfloat16)
    with Launches():
        yf = mf(xf)
        (gxf,) = torch.autograd.grad(yf, xf, gy.float())
        xb.requires_grad_(True)
        yb = mf(xb)
        (gxb,) = torch.autograd.grad(yb, xb, gy)
    assert yb.dtype == torch.bfloat16 and gxb.dtype == torch.bfloat16
    P.close("y (bf16 storage)", yb, yf, rel=2 * 2.0 ** -8, why="bf16 rounding of the stored output")
    P.close("gx (bf16 storage)", gxb, gxf, rel=2 * 2.0 ** -8, why="bf16 rounding of the stored gradient")


@pytest.mark.parametrize("solver", ["cd", "smu"])
@pytest.mark.parametrize("M,N", [(8, 4096), (16, 262144)])
@pytest.mark.parametrize("R", [1, 2, 3, 4])
def test_split_n_wide(solver, M, N, R):
    """shapes the wave-resident family refuses and the split-N kernels take (the reference's global Matricize)"""
    T, G = 5, 3
    assert not Fn.nmf_supported(M, N, R, T, G) and Fn.gnmf_supported(M, N, R, T, G)
    torch.manual_seed(M + R)
    x = torch.rand(2, M, N) if solver == "cd" else torch.randn(2, M, N)
    u0, v0 = torch.rand(M, R), torch.rand(N, R)
    gy = torch.rand_like(x) - 0.5
    mf = _mf(M, N, R, T, G, solver, u0, v0)
    y64, _, _, gx64 = composed(x, u0, v0, T, G, solver, gy=gy)
    y32, _, _, gx32 = composed(x, u0, v0, T, G, solver, gy=gy, dtype=torch.float32)
    timer = Fn.KernelTimer()
    Fn.set_timer(timer)
    try:
        xd = x.to(DEV).requires_grad_(True)
        y = mf(xd)
        (gx,) = torch.autograd.grad(y, xd, gy.to(DEV))
    finally:
        Fn.set_timer(None)
    ran = timer.summary()
    assert any(k.startswith("gnmf_fwd") for k in ran) and any(k.startswith("gnmf_bwd") for k in ran), sorted(ran)
    P.close("y", y, y64, extra=_kink(y32, y64))
    P.close("gx", gx, gx64, extra=_kink(gx32, gx64))


BLOCKS = {
    "p8": (16, (16, 16, 16), 8, "nmf_cf_"),
    "p4": (16, (8, 8, 8), 4, "nmf_pcf_"),
    "p565": (16, (10, 12, 10), (5, 6, 5), "nmf_pcf_"),
    "2d": (16, (16, 16), 4, "nmf_pcf_"),
}


@pytest.mark.parametrize("solver", ["cd", "smu"])
@pytest.mark.parametrize("R", [1, 2])
@pytest.mark.parametrize("geo", sorted(BLOCKS))
def test_block_on_the_fused_core(solver, R, geo):
    C, S, patch, fam = BLOCKS[geo]
    torch.manual_seed(R)
    blk = ft.FactorizerBlock(channels=C, spatial_size=S, norm=ft.LayerNorm, reshape=(ft.SWMatricize, {"head_dim": 8, "patch_size": patch}),
                             act=nn.ReLU, factorize=ft.NMF, rank=R, num_iters=5, init="uniform", solver=solver, mlp_ratio=2, dropout=0.0)
    x = torch.randn(2, C, *S)
    gy = torch.rand(2, C, *S) - 0.5
    refs = {}
    for dt in (torch.float64, torch.float32):
        b = copy.deepcopy(blk).to(dt)
        xx = x.to(dt).requires_grad_(True)
        yy = b(xx)
        refs[dt] = (yy.detach(), torch.autograd.grad(yy, [xx] + list(b.parameters()), gy.to(dt)))
    names = [k for k, _ in blk.named_parameters()]
    blk = blk.to(DEV)
    xd = x.to(DEV).requires_grad_(True)
    timer = Fn.KernelTimer()
    Fn.set_timer(timer)
    n0 = _native.launch_count()
    try:
        with warnings.catch_warnings():
            warnings.simplefilter("error", RuntimeWarning)      # any composed-ATen branch on device warns: none may be taken
            y = blk(xd)
            grads = torch.autograd.grad(y, [xd] + list(blk.parameters()), gy.to(DEV))
    finally:
        Fn.set_timer(None)
    ran = timer.summary()
    assert _native.launch_count() > n0
    assert any(k.startswith(fam + "fwd") for k in ran) and any(k.startswith(fam + "bwd") for k in ran), sorted(ran)
    assert not any(k.startswith(("swm_", "nmf_fwd", "nmf_bwd")) for k in ran), sorted(ran)
    y64, g64 = refs[torch.float64]
    y32, g32 = refs[torch.float32]
    P.close("y", y, y64, extra=_kink(y32, y64))
    for k, gr, r64, r32 in zip(["x"] + names, grads, g64, g32):
        P.close("grad:" + k, gr, r64, extra=_kink(r32, r64))


def test_c_abi_accepts_cd_smu_and_rejects_unknown_ids():
    lib = _native.lib()
    M, N, R, T, nmat = 8, 64, 2, 3, 4
    x = torch.rand(nmat, M, N, device=DEV)
    u0, v0 = torch.rand(M, R, device=DEV), torch.rand(N, R, device=DEV)
    y = torch.empty_like(x)
    s = _native.stream_ptr(x)
    n0 = _native.launch_count()
    for sid in (2, 3):
        rc = lib.fz_nmf_fwd(x.data_ptr(), u0.data_ptr(), v0.data_ptr(), y.data_ptr(), None, None, nmat, M, N, R, T, sid, 1e-16,
                            _native.STORE_F32, s)
        assert rc == 0, sid
    torch.cuda.synchronize()
    assert _native.launch_count() > n0
    rc = lib.fz_nmf_fwd(x.data_ptr(), u0.data_ptr(), v0.data_ptr(), y.data_ptr(), None, None, nmat, M, N, R, T, 7, 1e-16,
                        _native.STORE_F32, s)
    assert rc == -4        # FZ_E_ARG: bad solver
