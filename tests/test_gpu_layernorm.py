"""-m gpu: every path of csrc/ln.hip (fz_ln_fwd, fz_ln_bwd, fz_rowsum, the one- and two-stage fz_reduce_rows behind them)
against the float64 closed forms of tests/ln_cases.py, evaluated on the device.  Exact sweeps: dyadic inputs whose only correct
answer is the float64 one, asserted bit for bit (a dropped quad, a masked lane that is not masked, a wrong rounding mode of the
bf16 store all change bits).  Rounded sweeps: element-wise under the a-priori bounds of ln_cases, the achieved fraction
recorded.  The test ids name the kernel path: generic32 / generic64 / generic0 (ln_bwd_kernel<32|64|0>), slice_sub4 /
slice_sub1 (ln_bwd_slice_kernel, SUB = 4 | 1; 'stream' where CS / SUB > 16), split8 / split16 (ln_bwd_split_kernel<8|16>),
rows1 / rows2 (the one- / two-stage row reduction)."""
import ctypes
import warnings

import pytest
import torch
import torch.nn.functional as F

import factorizer_amd as ft
import ln_cases as LC
import parity as P
from factorizer_amd import _native
from factorizer_amd import pointwise as PW

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BF = torch.bfloat16
DT = sorted(LC.DTYPES)
FLAGS = [(True, True), (True, False), (False, True), (False, False)]     # (GADD, PART)


@pytest.fixture(scope="module")
def seam():
    return LC.sub_seam(_native.lib())


@pytest.fixture(scope="module")
def rowsum_seams():
    return LC.rowsum_seams(_native.lib().fz_rowsum_chunks)


class native:
    """asserts that the block launched native kernels and raised no composed-fallback warning"""

    def __enter__(self):
        self.n0 = _native.launch_count()
        self.w = warnings.catch_warnings()
        self.w.__enter__()
        warnings.simplefilter("error", RuntimeWarning)

    def __exit__(self, *exc):
        self.w.__exit__(*exc)
        if exc[0] is None:
            assert _native.launch_count() > self.n0


def bwd(gl, x, stats, g, gadd, part=True):
    """fz_ln_bwd: through PW._ln_backward, or (gparams = NULL) through the C ABI"""
    with native():
        if part:
            return PW._ln_backward(gl, x, stats, g, gadd)
        B, C, V = x.shape
        gx = torch.empty_like(x)
        with torch.cuda.device(x.device):
            rc = _native.lib().fz_ln_bwd(gl.data_ptr(), x.data_ptr(), stats.data_ptr(), g.data_ptr(), _native.ptr(gadd),
                                         gx.data_ptr(), None, None, B, C, V, _native.act_dtype(x), _native.stream_ptr(x))
        _native.check(rc, "fz_ln_bwd")
        return gx, None, None


def fwd(x, g, b, want_stats=True, eps=LC.EPS):
    B, C, V = x.shape
    y = torch.empty_like(x)
    stats = torch.full((B, 2, V), float("nan"), device=x.device) if want_stats else None
    with native(), torch.cuda.device(x.device):
        rc = _native.lib().fz_ln_fwd(x.data_ptr(), g.data_ptr(), b.data_ptr(), y.data_ptr(), _native.ptr(stats), B, C, V, eps,
                                     _native.act_dtype(x), _native.stream_ptr(x))
    _native.check(rc, "fz_ln_fwd")
    return y, stats


def check_exact_bwd(args, part=True, replay=False):
    gl, x, stats, g, gadd = args
    ref = LC.bwd64(gl, x, stats, g, gadd, out_dtype=x.dtype)
    assert ref["representable"] and float(ref["gg_terms"].max()) < 2 ** 22
    gx, gg, gb = bwd(gl, x, stats, g, gadd, part)
    assert gx.dtype == x.dtype and torch.equal(gx, ref["gx"]), f"gx: {int((gx != ref['gx']).sum())} elements differ"
    if part:
        assert gg.dtype == torch.float32 and torch.equal(gg.double(), ref["gg"]), "gγ"
        assert torch.equal(gb.double(), ref["gb"]), "gβ"
    if replay:
        again = bwd(gl, x, stats, g, gadd, part)
        assert all(a is None or torch.equal(a, b) for a, b in zip((gx, gg, gb), again))


# ------------------------------------------------------------------ (a) exact backward ------------------------------------
@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("B,V", LC.GENERIC_BV)
@pytest.mark.parametrize("C", LC.GENERIC_C)
def test_exact_bwd_generic32_generic64(seam, C, B, V, dtype):
    assert LC.bwd_path(C, B * V // 4, seam) == ("generic32" if C <= 32 else "generic64")
    for with_gadd in (True, False):
        check_exact_bwd(LC.exact_bwd(B, C, V, LC.DTYPES[dtype], with_gadd, device=DEV), replay=(C in (32, 48) and B == 3))


@pytest.mark.parametrize("dtype", DT)
def test_exact_bwd_generic32_grid_stride(dtype):
    """more than GRID_CAP_BWD · 256 quads: the register accumulators carry over a second grid-stride iteration"""
    quads = 262200
    assert quads > LC.GRID_CAP_BWD * 256
    check_exact_bwd(LC.exact_bwd(1, 3, 4 * quads, LC.DTYPES[dtype], True, device=DEV))


@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("C", [6, 48])
def test_exact_bwd_generic0_no_params(C, dtype):
    for B, V in [(3, 20), (2, 1028)]:
        for with_gadd in (True, False):
            check_exact_bwd(LC.exact_bwd(B, C, V, LC.DTYPES[dtype], with_gadd, device=DEV), part=False, replay=B == 3)


@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("B,V", LC.SLICE_BV)
@pytest.mark.parametrize("C", LC.SLICE_C)
def test_exact_bwd_slice_sub4_rows1(seam, C, B, V, dtype):
    assert LC.bwd_path(C, B * V // 4, seam) == "slice_sub4"
    for gadd, part in FLAGS:
        check_exact_bwd(LC.exact_bwd(B, C, V, LC.DTYPES[dtype], gadd, device=DEV), part=part, replay=(C == 128 and B == 3))


@pytest.mark.parametrize("dtype", DT)
def test_exact_bwd_slice_sub4_rows2(seam, dtype):
    B, C, V = 1, 64, 32820
    assert LC.partial_rows(C, V // 4, seam) == 513 and LC.bwd_path(C, V // 4, seam) == "slice_sub4"
    check_exact_bwd(LC.exact_bwd(B, C, V, LC.DTYPES[dtype], True, device=DEV), replay=True)


@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("at", ["seam", "seam+1"])
@pytest.mark.parametrize("C", [64, 128, 256])
def test_exact_bwd_slice_sub1(seam, C, at, dtype):
    """SUB = 1 from the seam on (C = 256: the streamed slice, CS / SUB = 32 > 16); seam + 1 quads leave a masked tail"""
    quads = seam + (at == "seam+1")
    assert LC.bwd_path(C, quads, seam) == "slice_sub1" and LC.bwd_path(C, seam - 1, seam) == "slice_sub4"
    check_exact_bwd(LC.exact_bwd(1, C, 4 * quads, LC.DTYPES[dtype], True, device=DEV), replay=(C == 64 and at == "seam+1"))


@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("gadd,part", FLAGS[1:], ids=["gadd_nopart", "nogadd_part", "nogadd_nopart"])
def test_exact_bwd_slice_sub1_flags(seam, gadd, part, dtype):
    check_exact_bwd(LC.exact_bwd(1, 128, 4 * (seam + 1), LC.DTYPES[dtype], gadd, device=DEV), part=part)


def test_exact_bwd_slice_sub1_stream_c512_bf16(seam):
    check_exact_bwd(LC.exact_bwd(1, 512, 4 * (seam + 1), BF, True, device=DEV))


@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("B,V", LC.SPLIT_BV)
@pytest.mark.parametrize("C", LC.SPLIT_C)
def test_exact_bwd_split8_split16(seam, C, B, V, dtype):
    assert LC.bwd_path(C, B * V // 4, seam) == ("split16" if C >= 256 else "split8")
    for with_gadd in (True, False):
        check_exact_bwd(LC.exact_bwd(B, C, V, LC.DTYPES[dtype], with_gadd, device=DEV), replay=(B == 3 and C in (96, 320)))
    check_exact_bwd(LC.exact_bwd(B, C, V, LC.DTYPES[dtype], True, seed=1, device=DEV), part=False)


@pytest.mark.parametrize("dtype", DT)
def test_exact_bwd_split8_rows2(seam, dtype):
    quads = 512 * 64 + 4
    assert LC.partial_rows(96, quads, seam) == 513
    check_exact_bwd(LC.exact_bwd(1, 96, 4 * quads, LC.DTYPES[dtype], True, device=DEV))


# ------------------------------------------------------------------ (b) exact forward -------------------------------------
def check_exact_fwd(x, g, b, want_stats=True):
    mu, rs, y64 = LC.fwd64(x, g, b)
    dmu, drs, dy = LC.fwd_bounds(x, g, b, x.dtype)
    y, stats = fwd(x, g, b, want_stats)
    fr = {"y": LC.fraction(y, y64, dy)}
    if want_stats:
        assert torch.equal(stats[:, 0].double(), mu), "mu"
        fr["rs"] = LC.fraction(stats[:, 1], rs, drs)
    assert all(v <= 1 for v in fr.values()), fr
    return fr


@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("C", LC.FWD_C)
def test_exact_fwd(C, dtype):
    for B, V in LC.GENERIC_BV + [(1, 60)]:
        check_exact_fwd(*LC.exact_fwd(B, C, V, LC.DTYPES[dtype], device=DEV))
    check_exact_fwd(*LC.exact_fwd(3, C, 20, LC.DTYPES[dtype], seed=1, device=DEV), want_stats=False)   # stats = NULL


@pytest.mark.parametrize("dtype", DT)
def test_exact_fwd_grid_stride(dtype):
    quads = 1048600
    assert quads > LC.GRID_CAP_FWD * 256
    check_exact_fwd(*LC.exact_fwd(1, 2, 4 * quads, LC.DTYPES[dtype], device=DEV))


# ------------------------------------------------------------------ (c) rounded forward and backward ----------------------
def _rounded_shapes(seam):
    return dict(LC.ROUNDED_SHAPES, slice_sub1=(1, 64, 4 * (seam + 1)), slice_sub1_stream_c256=(1, 256, 4 * (seam + 1)))


@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("path", sorted(LC.ROUNDED_SHAPES) + ["slice_sub1", "slice_sub1_stream_c256"])
@pytest.mark.parametrize("name", sorted(LC.ROUNDED))
def test_rounded(seam, name, path, dtype):
    dt = LC.DTYPES[dtype]
    B, C, V = _rounded_shapes(seam)[path]
    x, g, b, gl, gadd = LC.rounded(name, B, C, V, dt, device=DEV)
    mu, rs, y64 = LC.fwd64(x, g, b)
    dmu, drs, dy = LC.fwd_bounds(x, g, b, dt)
    y, st = fwd(x, g, b)
    fr = {"mu": LC.fraction(st[:, 0], mu, dmu), "rs": LC.fraction(st[:, 1], rs, drs), "y": LC.fraction(y, y64, dy)}
    del y64, dy
    stats = LC.stats_of(x)
    dgx, dgg, dgb, ref = LC.bwd_bounds(gl, x, stats, g, gadd, dt, LC.param_depth(C, B * V // 4, seam))
    gx, gg, gb = bwd(gl, x, stats, g, gadd)
    fr.update(gx=LC.fraction(gx, ref["gx"], dgx), gg=LC.fraction(gg, ref["gg"], dgg), gb=LC.fraction(gb, ref["gb"], dgb))
    print("fraction of the bound:", fr)
    P.note(f"layernorm {path} {name} {dtype}: fraction of the bound", **fr)
    for k, v in fr.items():
        assert v <= 1, f"{k}: {v:.3f} of the bound"


# ------------------------------------------------------------------ (d) the producers of the statistics -------------------
@pytest.mark.parametrize("producer", ["ln_fwd", "ln_linear"])
@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("C", [32, 96, 128, 512])
def test_statistics_producers(C, dtype, producer):
    dt = LC.DTYPES[dtype]
    for name in ("randn", "mean_30_std_half", "mean_1000"):
        B, V = 2, 1300
        x, g, b, _, _ = LC.rounded(name, B, C, V, dt, device=DEV)
        if producer == "ln_fwd":
            _, stats = fwd(x, g, b)
        else:
            w = torch.randn(C, C, 1, device=DEV) / C ** 0.5
            with native():
                y = PW.ln_linear(x.view(B, C, V, 1, 1).requires_grad_(True), g, b, LC.EPS, w, None, "none")
            stats = y.grad_fn.saved_tensors[1]
            assert stats.shape == (B, 2, V) and stats.dtype == torch.float32
        mu, rs, _ = LC.fwd64(x, g, b)
        dmu, drs = LC.stats_bounds(x)
        fr = {"mu": LC.fraction(stats[:, 0], mu, dmu), "rs": LC.fraction(stats[:, 1], rs, drs)}
        P.note(f"layernorm statistics of {producer} C={C} {name} {dtype}: fraction of the bound", **fr)
        assert all(v <= 1 for v in fr.values()), (name, fr)


# ------------------------------------------------------------------ (e) the fused dgrad + LayerNorm backward --------------
@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("C,Mz,B,V", [(32, 32, 2, 1300), (32, 64, 2, 1300), (64, 64, 2, 1300), (32, 32, 1, 512 * 512 + 4),
                                      (64, 64, 1, 256 * 513 + 4)],
                         ids=["c32_m32_partial_tile", "c32_m64_partial_tile", "c64_m64_partial_tile", "c32_rows2", "c64_rows2"])
def test_exact_dgrad_lnbwd(C, Mz, B, V, dtype):
    gz, w2, gl, x, stats, g, gadd = LC.exact_dgrad(B, C, Mz, V, LC.DTYPES[dtype], device=DEV)
    if V > 100000:
        d = _native.GemmDesc()
        d.M, d.Ncol, d.B = C, V, B
        assert _native.lib().fz_gemm_lnbwd_partials(ctypes.byref(d)) > 512
    ref = LC.bwd64(gl, x, stats, g, gadd, out_dtype=x.dtype)
    assert ref["representable"] and float(ref["gg_terms"].max()) < 2 ** 22
    with native():
        gx, gg, gb = PW._dgrad_lnbwd(gz, w2, x, stats, g, gadd)
    assert torch.equal(gx, ref["gx"]) and torch.equal(gg.double(), ref["gg"]) and torch.equal(gb.double(), ref["gb"])


# ------------------------------------------------------------------ (f) fz_rowsum, fz_reduce_rows --------------------------
@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("at", ["last_of_1", "first_of_2", "three_plus_4", "cap"])
def test_exact_rowsum(rowsum_seams, at, dtype):
    lib, V = _native.lib(), rowsum_seams[at]
    nchunk = lib.fz_rowsum_chunks(V)
    assert nchunk == {"last_of_1": 1, "first_of_2": 2, "three_plus_4": 3, "cap": rowsum_seams["top"]}[at]
    gen = torch.Generator(device=DEV).manual_seed(V)
    for B in (1, 3):
        for C in (1, 5):
            x = torch.randint(-3, 4, (B, C, V), generator=gen, device=DEV, dtype=torch.float32).to(LC.DTYPES[dtype])
            part = torch.full((B * nchunk * C,), float("nan"), device=DEV)
            out = torch.full((C,), float("nan"), device=DEV)
            with native(), torch.cuda.device(DEV):
                rc = lib.fz_rowsum(x.data_ptr(), part.data_ptr(), out.data_ptr(), B, C, V, _native.act_dtype(x), _native.stream_ptr(x))
            _native.check(rc, "fz_rowsum")
            assert torch.equal(out.double(), x.double().sum((0, 2))), (B, C)


@pytest.mark.parametrize("with_tmp", [True, False], ids=["tmp", "notmp"])
def test_exact_reduce_rows_rows1_rows2(with_tmp):
    lib = _native.lib()
    gen = torch.Generator(device=DEV).manual_seed(11)
    for rows in (1, 512, 513, 700, 4097):
        for n in (1, 33, 2 * 512):
            part = torch.randint(-3, 4, (rows, n), generator=gen, device=DEV, dtype=torch.float32)
            tmp = torch.full((64, n), float("nan"), device=DEV) if with_tmp else None
            out = torch.full((n,), float("nan"), device=DEV)
            with native(), torch.cuda.device(DEV):
                rc = lib.fz_reduce_rows(part.data_ptr(), rows, n, out.data_ptr(), _native.ptr(tmp), _native.stream_ptr(part))
            _native.check(rc, "fz_reduce_rows")
            assert torch.equal(out.double(), part.double().sum(0)), (rows, n)


# ------------------------------------------------------------------ (g) end to end -----------------------------------------
def _e2e_close(what, got, ref, dt, n_stores=1):
    """the project's bounds: 1e-4 of max|ref| in fp32; n_stores · 2^-8 of max|ref| with bf16 storage (tests/test_gpu_bf16.py)"""
    if dt == BF:
        P.close(what, got, ref, rel=n_stores * 2.0 ** -8,
                why=f"bf16 storage: {n_stores} stored tensor(s) x u = 2^-8 between input and this result")
    else:
        P.close(what, got, ref)


@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("path,B,C,S", [("generic32", 2, 32, (4, 4, 8)), ("generic64", 2, 48, (4, 4, 8)),
                                        ("slice_sub4", 2, 128, (4, 4, 4)), ("split8", 2, 96, (4, 4, 4)),
                                        ("split16", 2, 320, (2, 4, 4)), ("slice_sub1", 1, 64, None)])
def test_layernorm_module_end_to_end(seam, path, B, C, S, dtype):
    dt = LC.DTYPES[dtype]
    S = S or (4 * (seam + 1), 1, 1)
    torch.manual_seed(C)
    x = (torch.randn(B, C, *S) * 2 + 0.5).to(dt)
    gy = torch.randn(B, C, *S).to(dt)
    m = ft.LayerNorm(C)
    with torch.no_grad():
        m.norm.weight.copy_(torch.rand(C) + 0.5)
        m.norm.bias.copy_(torch.randn(C))
    x64 = x.double().requires_grad_(True)
    w64, b64 = (p.detach().double().requires_grad_(True) for p in (m.norm.weight, m.norm.bias))
    y64 = F.layer_norm(x64.movedim(1, -1), (C,), w64, b64, m.norm.eps).movedim(-1, 1)
    ref = (y64.detach(),) + torch.autograd.grad(y64, [x64, w64, b64], gy.double())
    m = m.to(DEV)
    xd = x.to(DEV).requires_grad_(True)
    with native():
        y = m(xd)
        got = (y.detach(),) + torch.autograd.grad(y, [xd, m.norm.weight, m.norm.bias], gy.to(DEV))
    assert y.dtype == dt and got[1].dtype == dt and got[2].dtype == torch.float32
    for k, a, r in zip(("y", "gx", "gγ", "gβ"), got, ref):
        _e2e_close(f"ft.LayerNorm {path} {dtype} {k}", a, r, dt)


@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("path,B,C,M,S", [("generic32", 2, 32, 64, (4, 4, 8)), ("slice_sub4", 2, 128, 64, (4, 4, 4)),
                                          ("split8", 2, 96, 32, (4, 4, 4))])
def test_ln_linear_end_to_end(path, B, C, M, S, dtype):
    dt = LC.DTYPES[dtype]
    torch.manual_seed(C + 1)
    x = (torch.randn(B, C, *S) * 2 + 0.5).to(dt)
    gy = torch.randn(B, M, *S).to(dt)
    ps = [torch.rand(C) + 0.5, torch.randn(C) * 0.3, torch.randn(M, C, 1) / C ** 0.5, torch.randn(M)]
    t64 = [t.double().requires_grad_(True) for t in [x] + ps]
    ln = F.layer_norm(t64[0].movedim(1, -1), (C,), t64[1], t64[2], LC.EPS)
    y64 = (ln @ t64[3].view(M, C).t() + t64[4]).movedim(-1, 1)
    ref = (y64.detach(),) + torch.autograd.grad(y64, t64, gy.double())
    td = [t.to(DEV).requires_grad_(True) for t in [x] + ps]
    with native():
        y = PW.ln_linear(td[0], td[1], td[2], LC.EPS, td[3], td[4], "none")
        got = (y.detach(),) + torch.autograd.grad(y, td, gy.to(DEV))
    # backward: gl (stored bf16) -> LayerNorm backward -> gx; the weight gradient sees LN(x) rounded to bf16
    for k, a, r, n in zip(("y", "gx", "gγ", "gβ", "gw", "gb"), got, ref, (1, 3, 2, 2, 2, 2)):
        _e2e_close(f"PW.ln_linear {path} {dtype} {k}", a, r.reshape(a.shape), dt, n)
