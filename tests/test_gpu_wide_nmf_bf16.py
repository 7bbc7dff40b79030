"""-m gpu: the two split-N NMF families (csrc/nmf_global.hip: M <= 64, rank <= 4; csrc/nmf_global_rank.hip: ranks up to
32, up to 512 rows) on bf16 activation storage — `ft.NMF` on a bf16 input or under autocast.

"Only storage changes" is tested as a statement about bits: on bf16-representable inputs, y and gx of the bf16 run equal
the fp32 family's y and gx (same device, same values held in fp32 tensors) converted to bf16, compared as integers.  The
fp32 family is itself held to float64 by tests/test_gpu_wide_nmf.py and tests/test_gpu_wide_nmf_rank.py; so that this
file does not rest on the bit comparison alone, the bf16 results are also held to the float64 oracle on the rounded
inputs: one stored tensor x u = 2^-8, plus the fp32 oracle's own distance to float64 (tests/wide_bf16_cases.py)."""
import warnings

import pytest
import torch

import factorizer_amd as ft
import parity as P
import wide_bf16_cases as WB
import wide_rank_cases as W
from factorizer_amd import _native
from factorizer_amd import functional as Fn
from oracle import cpu_ref as O
from wide_bf16_cases import BF, bits, close, rb

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _module(M, N, R, T, G, solver, u0, v0):
    nmf = ft.NMF(size=(M, N), rank=R, num_iters=T, num_grad_steps=G, init="uniform", solver=solver)
    nmf.load_state_dict({"init.u0": u0, "init.v0": v0})
    return nmf.to(DEV)


def _launches(fam, M, N, R, T, Gs, backward):
    lib = _native.lib()
    if fam == "gnmfx":
        return lib.fz_gnmfx_launches(M, N, R, T, Gs, backward)
    want = (2 * T + 1 if T else 1) + ((2 * Gs + 1) if backward else 0)
    assert lib.fz_gnmf_launches(T, Gs, backward) == want
    return want


def _run(nd, xd, gyd, fam, T, G):
    """y, gx of the device module on device tensors (leaf `xd` is made here from a detached alias), every RuntimeWarning
    an error, the family and the launch counter asserted"""
    M, N = nd.size
    Gs = T if G is None else G
    xd = xd.detach().requires_grad_(True)
    n0 = _native.launch_count()
    with warnings.catch_warnings():
        warnings.simplefilter("error", RuntimeWarning)
        y = nd(xd)
    torch.cuda.synchronize()
    assert nd._wide == fam
    assert _native.launch_count() - n0 == _launches(fam, M, N, nd.rank, T, Gs, 0)
    n1 = _native.launch_count()
    (gx,) = torch.autograd.grad(y, xd, gyd)
    torch.cuda.synchronize()
    if Gs > 0:
        assert _native.launch_count() - n1 == _launches(fam, M, N, nd.rank, T, Gs, 1)
    else:
        assert _native.launch_count() == n1
    assert y.dtype == gx.dtype == xd.dtype
    return y.detach(), gx


def _bf16_and_fp32(nd, x, gy, fam, T, G):
    """(y, gx) in bf16 storage and of the fp32 family on the same (bf16-representable) values; the bits compared"""
    assert torch.equal(rb(x), x) and torch.equal(rb(gy), gy)
    y, gx = _run(nd, x.to(DEV, BF), gy.to(DEV, BF), fam, T, G)
    y32, gx32 = _run(nd, x.to(DEV), gy.to(DEV), fam, T, G)
    assert y.dtype == BF and gx.dtype == BF and y32.dtype == torch.float32
    assert (y.float() >= 0).all()
    ny = (bits(y) != bits(y32.to(BF))).sum().item()
    ng = (bits(gx) != bits(gx32.to(BF))).sum().item()
    print(f"bf16 vs rounded fp32 {fam} {tuple(x.shape)}: {ny} y and {ng} gx elements differ")
    assert ny == 0 and ng == 0, (ny, ng)
    return y, gx


# ---- 1. the rank family on every pair of the planted cases ---------------------------------------------------------------
@pytest.mark.parametrize("M,N,R,T,G,solver", W.PAIRS, ids=W.IDS)
def test_rank_family_bf16(M, N, R, T, G, solver):
    """N: 777 odd, 1030 = 2 mod 4, 2052 = 4 mod 8, 1024 / 520 / 512 = 0 mod 8, 64 below the thread count, 8200 past the
    one-thread-per-column switch; M 16 and 512; R 1 and 32"""
    ref = WB.guard(M, N, R, T, G, solver)
    x, u0, v0, gy = WB.inputs(M, N, R)
    assert Fn.gnmfx_supported(M, N, R, T, T if G is None else G)
    y, gx = _bf16_and_fp32(_module(M, N, R, T, G, solver, u0, v0), x, gy, "gnmfx", T, G)
    tag = f"{M}x{N} R{R} T{T} G{G} {solver} bf16"
    close(f"y {tag} (vs fp64 oracle)", y, ref["y64"], 1, extra=ref["y_kink"])
    close(f"gx {tag} (vs fp64 oracle)", gx, ref["gx64"], 1, extra=ref["gx_kink"])


# ---- 2. the R <= 4 family ---------------------------------------------------------------------------------------------
def _small_inputs(M, N, R):
    """the inputs of tests/test_gpu_wide_nmf.py::_run (a block of 40 zero columns), x and gy rounded to bf16"""
    torch.manual_seed(M * 1000 + N + R)
    x = torch.rand(2, M, N)
    x[0][:, : min(N, 40)] = 0
    u0, v0 = torch.rand(M, R), torch.rand(N, R)
    gy = torch.rand_like(x)
    return rb(x), u0, v0, rb(gy)


def _small(M, N, R, T, solver, G=None):
    x, u0, v0, gy = _small_inputs(M, N, R)
    y, gx = _bf16_and_fp32(_module(M, N, R, T, G, solver, u0, v0), x, gy, "gnmf", T, G)
    d = lambda t: t.double()
    y64 = O.nmf_forward(d(x), d(u0), d(v0), T, solver, G)
    gx64 = O.nmf_backward(d(x), d(u0), d(v0), d(gy), T, solver, G)
    yk = (O.nmf_forward(x, u0, v0, T, solver, G).double() - y64).abs().max().item()
    gk = (O.nmf_backward(x, u0, v0, gy, T, solver, G).double() - gx64).abs().max().item()
    tag = f"{M}x{N} R{R} T{T} G{G} {solver} bf16"
    close(f"y {tag} (vs fp64 oracle)", y, y64.float(), 1, extra=yk)
    close(f"gx {tag} (vs fp64 oracle)", gx, gx64.float(), 1, extra=gk)
    return gx


@pytest.mark.parametrize("solver", ["mu", "hals"])
@pytest.mark.parametrize("M,N,R", [(16, 4096, 1), (16, 3000, 3), (24, 2048, 4), (40, 1030, 2), (64, 1024, 1), (5, 777, 2)])
def test_small_rank_family_bf16(solver, M, N, R):
    """N % 4 == 0 (a thread owns four columns: 8-byte accesses) and not (777, 1030: single elements); M <= 16 (rows in
    registers) and above; a ragged last slab; a block of zero columns"""
    _small(M, N, R, 4, solver)


def test_small_rank_family_bf16_grad_steps():
    _small(16, 2048, 2, 5, "hals", G=2)
    gx = _small(16, 2048, 1, 3, "mu", G=0)
    assert gx.dtype == BF and not gx.any()


# ---- 3. a base pointer that is only 2-byte aligned -------------------------------------------------------------------------
POISON = -12288.0   # (a bf16 value)


def _off_by_one(t):
    """t's values as a contiguous bf16 view that starts one element into its storage, and the storage"""
    flat = torch.full((t.numel() + 2,), POISON, dtype=BF, device=DEV)
    flat[1:-1] = t.to(DEV, BF).flatten()
    v = flat[1:-1].view(t.shape)
    assert v.is_contiguous() and v.data_ptr() % 4 == 2
    return v, flat


def _entry_points(nd, x, gy, y, gx, fam, T):
    """fz_<fam>_fwd_act / _bwd_act straight into the given bf16 buffers (a test of where the kernels store)"""
    lib = _native.lib()
    M, N = nd.size
    R, nmat = nd.rank, x.numel() // (M * N)
    u0, v0 = nd.init.u0.contiguous(), nd.init.v0.contiguous()
    sid, eps, st = _native.SOLVER_ID[nd.solver.native_id], nd.solver.eps, _native.stream_ptr(x)
    ws = Fn._gnmf_ws(x, nmat, M, N, R, T, False, fam)
    _native.check(getattr(lib, f"fz_{fam}_fwd_act")(x.data_ptr(), u0.data_ptr(), v0.data_ptr(), y.data_ptr(), None, None,
                                                   nmat, M, N, R, T, sid, eps, _native.STORE_BF16, ws.data_ptr(), st), "fwd")
    ws = Fn._gnmf_ws(x, nmat, M, N, R, T, True, fam)
    _native.check(getattr(lib, f"fz_{fam}_bwd_act")(x.data_ptr(), u0.data_ptr(), v0.data_ptr(), gy.data_ptr(), None, None,
                                                   gx.data_ptr(), nmat, M, N, R, T, T, sid, eps, _native.STORE_BF16,
                                                   ws.data_ptr(), st), "bwd")
    torch.cuda.synchronize()


@pytest.mark.parametrize("fam,M,N,R,solver", [("gnmfx", 16, 777, 5, "hals"), ("gnmf", 24, 2048, 4, "mu"),
                                              ("gnmfx", 128, 2052, 13, "hals")])   # (N % 4 == 0 in the rank family too)
def test_unaligned_base(fam, M, N, R, solver):
    """x, gy, y and gx each one element into their storage: the same bits as in freshly allocated tensors, and the
    elements in front of and behind every matrix untouched"""
    T = 4
    x, u0, v0, gy = WB.inputs(M, N, R) if fam == "gnmfx" else _small_inputs(M, N, R)
    nd = _module(M, N, R, T, None, solver, u0, v0)
    y0, gx0 = _run(nd, x.to(DEV, BF), gy.to(DEV, BF), fam, T, None)            # freshly allocated: aligned
    assert y0.data_ptr() % 16 == 0 and gx0.data_ptr() % 16 == 0
    # through the module: x and gy unaligned (.contiguous() does not copy them), y and gx allocated by the library
    xv, xflat = _off_by_one(x)
    gv, gflat = _off_by_one(gy)
    y1, gx1 = _run(nd, xv, gv, fam, T, None)
    assert torch.equal(bits(y1), bits(y0)) and torch.equal(bits(gx1), bits(gx0))
    # through the entry points: y and gx unaligned too, with a poisoned element on either side
    yv, yflat = _off_by_one(torch.zeros_like(x))
    gxv, gxflat = _off_by_one(torch.zeros_like(x))
    _entry_points(nd, xv, gv, yv, gxv, fam, T)
    assert torch.equal(bits(yv), bits(y0)) and torch.equal(bits(gxv), bits(gx0))
    for flat in (xflat, gflat, yflat, gxflat):
        assert flat[0].item() == POISON and flat[-1].item() == POISON
    assert torch.equal(bits(xv), bits(x.to(BF))) and torch.equal(bits(gv), bits(gy.to(BF)))   # inputs are not written


# ---- 4. decompose -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fam,M,N,R,solver", [("gnmfx", 64, 1024, 7, "hals"), ("gnmf", 16, 2048, 2, "hals")])
def test_decompose_bf16(fam, M, N, R, solver):
    T = 4
    x, u0, v0, _ = WB.inputs(M, N, R) if fam == "gnmfx" else _small_inputs(M, N, R)
    nd = _module(M, N, R, T, None, solver, u0, v0)
    torch.manual_seed(5)
    gu, gv = torch.rand(2, M, R, device=DEV), torch.rand(2, N, R, device=DEV)
    outs = []
    for dt in (BF, torch.float32):
        xd = x.to(DEV, dt).requires_grad_(True)
        with warnings.catch_warnings():
            warnings.simplefilter("error", RuntimeWarning)
            u, v = nd.decompose(xd)
        assert nd._wide == fam and u.dtype == v.dtype == torch.float32
        (gx,) = torch.autograd.grad([u, v], xd, [gu, gv])
        assert gx.dtype == dt
        outs.append((u.detach(), v.detach(), gx))
    (ub, vb, gb), (uf, vf, gf) = outs
    i32 = lambda t: t.contiguous().view(torch.int32).cpu()
    assert torch.equal(i32(ub), i32(uf)) and torch.equal(i32(vb), i32(vf))      # the factors never leave fp32
    assert torch.equal(bits(gb), bits(gf.to(BF)))                               # gx: the fp32 run's, rounded once


# ---- 5. replay and batch independence -------------------------------------------------------------------------------------
@pytest.mark.parametrize("M,N,R,solver", [(128, 2052, 13, "hals"), (16, 777, 5, "hals")])
def test_bitwise_replay_and_batch_independence_bf16(M, N, R, solver):
    T = 4
    x, u0, v0, gy = WB.inputs(M, N, R)
    nd = _module(M, N, R, T, None, solver, u0, v0)
    torch.manual_seed(3)
    x3 = torch.cat([x[:1], torch.rand(2, M, N)])             # matrix 0 with two unrelated neighbours
    gy3 = torch.cat([gy[:1], torch.rand(2, M, N)])
    outs = []
    for xs, gs in ((x3, gy3), (x3, gy3), (x[:1], gy[:1])):
        y, gx = _run(nd, xs.to(DEV, BF), gs.to(DEV, BF), "gnmfx", T, None)
        outs.append((bits(y), bits(gx)))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])           # replay: identical bits
    assert torch.equal(outs[0][0][:1], outs[2][0]) and torch.equal(outs[0][1][:1], outs[2][1])   # batch of 3 vs batch of 1


# ---- 6. zero rows, zero columns, an all-zero matrix -----------------------------------------------------------------------
def test_zero_rows_and_columns_bf16():
    M, N, R, T, solver = 128, 2052, 13, 4, "mu"
    x, u0, v0, gy = WB.inputs(M, N, R)
    x = torch.cat([x, torch.zeros(1, M, N)])
    x[0, :, 1000:1100] = 0
    x[1, 60:70, :] = 0
    gy = torch.cat([gy, gy[:1]])
    y, gx = _bf16_and_fp32(_module(M, N, R, T, None, solver, u0, v0), x, gy, "gnmfx", T, None)
    assert torch.isfinite(y.float()).all() and torch.isfinite(gx.float()).all()


# ---- 7. a block -------------------------------------------------------------------------------------------------------
def test_block_with_rank_rule_bf16():
    """Matricize(num_heads=1, grid_size=1) at C = 64, 16^3: 64 x 4096, rank=None -> 7, inside a block on a bf16 input.
    y against the fp32 CPU module on the rounded input: 4 u, the bound tests/test_gpu_bf16.py holds the same six stored
    tensors of a block's forward to.  The gradients' distances are recorded, not bounded: how far bf16 storage of the NMF
    input moves MU R 7 gradients is a property of the configuration that nobody has measured."""
    torch.manual_seed(1)
    blk = ft.FactorizerBlock(64, (16, 16, 16), reshape=(ft.Matricize, {"num_heads": 1, "grid_size": 1}), rank=None,
                             solver="mu")
    assert blk.fact.factorize.size == (64, 4096) and blk.fact.factorize.rank == 7
    names = [n for n, _ in blk.named_parameters()]
    x = rb(torch.rand(2, 64, 16, 16, 16))
    gy = rb(torch.rand_like(x))
    xc = x.clone().requires_grad_(True)
    yc = blk(xc)
    gc = torch.autograd.grad(yc, [xc, *blk.parameters()], gy)
    blk = blk.to(DEV)
    xd = x.to(DEV, BF).requires_grad_(True)
    n0 = _native.launch_count()
    with warnings.catch_warnings():
        warnings.simplefilter("error", RuntimeWarning)
        yd = blk(xd)
        gd = torch.autograd.grad(yd, [xd, *blk.parameters()], gy.to(DEV, BF))
    torch.cuda.synchronize()
    assert _native.launch_count() > n0 and blk.fact.factorize._wide == "gnmfx"
    assert yd.dtype == BF and gd[0].dtype == BF and all(g.dtype == torch.float32 for g in gd[1:])
    assert torch.isfinite(yd.float()).all() and all(torch.isfinite(g.float()).all() for g in gd)
    close("block 64x4096 R7 bf16 y vs fp32 CPU module", yd, yc, 4)
    rel = lambda a, b: ((a.float().cpu() - b).abs().max() / (b.abs().max() + 1e-30)).item()
    P.note("block 64x4096 R7 mu: bf16 device gradients vs fp32 CPU module (relative to max|ref|, not bounded)",
           **{f"d{n}": rel(a, b) for n, a, b in zip(["x", *names], gd, gc)})


# ---- 8. the default model under autocast --------------------------------------------------------------------------------
@pytest.mark.parametrize("kw", [{}, {"solver": "mu"}], ids=["hals-as-constructed", "mu"])
def test_default_model_under_autocast(kw):
    """ft.Factorizer(4, 3, 32^3) inside torch.autocast(bfloat16), forward + backward, twice: every NMF native, bf16 finite
    output, identical bits.  No value bound for HALS, for the reason tests/test_gpu_wide_nmf_rank.py::
    test_default_model_as_constructed_hals gives (the reference's own HALS arithmetic is chaotic at these ranks)."""
    torch.manual_seed(2)
    model = ft.Factorizer(4, 3, (32, 32, 32), **kw).to(DEV)
    x = torch.rand(1, 4, 32, 32, 32)
    gy = torch.rand(1, 3, 32, 32, 32)
    nmfs = [m for m in model.modules() if isinstance(m, ft.NMF)]
    runs = []
    for _ in range(2):
        xd = x.to(DEV).requires_grad_(True)
        with warnings.catch_warnings():
            warnings.simplefilter("error", RuntimeWarning)
            with torch.autocast("cuda", dtype=BF):
                y = model(xd)
            grads = torch.autograd.grad(y, [xd, *model.parameters()], gy.to(DEV, y.dtype))
        assert y.dtype == BF and torch.isfinite(y.float()).all()
        assert all(m._wide in ("gnmf", "gnmfx") for m in nmfs), [m._wide for m in nmfs]
        as_int = lambda t: t.detach().contiguous().view(torch.int16 if t.dtype == BF else torch.int32).cpu()
        runs.append([as_int(t) for t in (y, *grads)])
    assert sorted({m._wide for m in nmfs}) == ["gnmf", "gnmfx"]
    for a, b in zip(*runs):
        assert torch.equal(a, b)
