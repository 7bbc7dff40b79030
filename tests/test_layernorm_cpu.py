"""No GPU: the tools of tests/ln_cases.py are checked before they judge a kernel.  The exact generator is exact (fp32 in two
channel orders equals float64 bitwise, the bf16 expectation holds ties); an fp32 emulation of the kernels stays under the
bounds; every mutant of the oracle breaks them (bitwise on the exact cases); the seams read from the library are consistent and
the workspace covers every path of ln_bwd_launch; the entry points refuse bad arguments before touching a device."""
import ctypes
import json
import warnings

import pytest
import torch

import ln_cases as LC

BF = torch.bfloat16
SWEEP_C = sorted(set(LC.GENERIC_C + [3, 6] + list(LC.SLICE_C) + LC.SPLIT_C))
FRACTIONS = {}     # what profiles/layernorm.md quotes: printed by test_report_fractions


@pytest.fixture(scope="module")
def lib():
    from factorizer_amd import _native, build
    build.build(verbose=False)
    return _native.lib()


@pytest.fixture(scope="module")
def seam(lib):
    return LC.sub_seam(lib)


# ------------------------------------------------------------------ the exact generator ------------------------------------
def _exact_equal(args, dtype, lanes=1):
    gl, x, stats, g, gadd = args
    ref = LC.bwd64(gl, x, stats, g, gadd, out_dtype=dtype)
    assert ref["representable"] and float(ref["gg_terms"].max()) < 2 ** 22
    for reverse in (False, True):
        gx, gg, gb = LC.emulate_bwd(gl, x, stats, g, gadd, dtype, lanes=lanes, reverse=reverse)
        assert torch.equal(gx, ref["gx"]) and torch.equal(gg.double(), ref["gg"]) and torch.equal(gb.double(), ref["gb"])
    return ref


@pytest.mark.parametrize("dtype", sorted(LC.DTYPES))
@pytest.mark.parametrize("C", SWEEP_C)
def test_exact_generator_is_exact(C, dtype):
    dt = LC.DTYPES[dtype]
    for with_gadd in (True, False):
        args = LC.exact_bwd(2, C, 20, dt, with_gadd, seed=3)
        assert all(t is None or t.dtype == dt for t in (args[0], args[1], args[4]))
        _exact_equal(args, dt)
        if C >= 64:
            _exact_equal(args, dt, lanes=16 if C not in LC.SLICE_C and C >= 256 else 8)
        if with_gadd and dt == BF:       # exact ties of the store, towards both neighbours
            gx64 = LC.bwd64(*LC.exact_bwd(2, C, max(20, 4000 // C // 4 * 4), dt, True, seed=3))["gx"]
            assert LC.bf16_ties(gx64) >= gx64.numel() // 100
            rne, trunc = LC.store(gx64, BF), LC.store(gx64, BF, trunc=True)
            away = ((gx64.float().view(torch.int32) + 0x8000) & -65536).view(torch.float32).to(BF)   # round-half-away
            assert not torch.equal(rne, trunc) and not torch.equal(rne, away)
    if C in LC.FWD_C:
        x, g, b = LC.exact_fwd(2, C, 20, dt, seed=3)
        mu, rs, y = LC.fwd64(x, g, b)
        for reverse in (False, True):
            emu = LC.emulate_fwd(x, g, b, dt, reverse=reverse)
            assert torch.equal(emu[0].double(), mu)


@pytest.mark.parametrize("C,Mz", [(32, 32), (32, 64), (64, 64)])
def test_exact_dgrad_inputs_keep_the_exactness_condition(C, Mz):
    for dt in (torch.float32, BF):
        gz, w2, gl, x, stats, g, gadd = LC.exact_dgrad(2, C, Mz, 20, dt, seed=5)
        assert torch.equal(torch.einsum("mc,bmv->bcv", w2, gz.float()), gl.float())     # fp32 products and sums: exact
        assert int((w2 != 0).sum()) == C and gl.abs().max() <= 2 and gl.abs().max() > 0
        _exact_equal((gl, x, stats, g, gadd), dt)


def test_mutants_differ_bitwise_on_the_exact_cases():
    for C in (5, 64, 100, 1024):
        for dt in (torch.float32, BF):
            args = LC.exact_bwd(3, C, 20, dt, True, seed=4)
            ref = LC.bwd64(*args, out_dtype=dt)
            for m in LC.BWD_MUTANTS:
                if m == "bf16_trunc" and dt != BF:
                    continue
                if m in ("m1_drop_last", "m2_drop_last", "div_c_minus_1") and not LC.is_pow2(C):
                    continue                # the paired channels make both means 0 (ln_cases): nothing to get wrong there
                if m == "gamma_next" and not LC.is_pow2(C):
                    continue                # a pair shares |γ|: covered by the powers of two and the rounded cases
                mut = LC.bwd64(*args, mutant=m, out_dtype=dt)
                assert not all(torch.equal(mut[k], ref[k]) for k in ("gx", "gg", "gb")), (C, dt, m)


# ------------------------------------------------------------------ emulation and mutants against the bounds ---------------
def _bwd_fracs(got, ref, bounds):
    dgx, dgg, dgb = bounds
    return {"gx": LC.fraction(got[0], ref["gx"], dgx), "gg": LC.fraction(got[1], ref["gg"], dgg),
            "gb": LC.fraction(got[2], ref["gb"], dgb)}


def _applies(m, name, dt):
    if m == "bf16_trunc":
        return dt == BF
    if m == "one_pass_fp32":
        return name in LC.LARGE_MEAN
    if m == "eps_outside":
        return name == "var_near_eps"       # elsewhere eps / var is below the rounding of the variance itself
    return True


@pytest.mark.parametrize("dtype", sorted(LC.DTYPES))
@pytest.mark.parametrize("path", sorted(LC.ROUNDED_SHAPES))
@pytest.mark.parametrize("name", sorted(LC.ROUNDED))
def test_emulation_under_the_bound_and_mutants_over_it(seam, name, path, dtype):
    dt = LC.DTYPES[dtype]
    B, C, V = LC.ROUNDED_SHAPES[path]
    x, g, b, gl, gadd = LC.rounded(name, B, C, V, dt)
    # forward
    mu, rs, y = LC.fwd64(x, g, b)
    dmu, drs, dy = LC.fwd_bounds(x, g, b, dt)
    emu = LC.emulate_fwd(x, g, b, dt)
    fr = {"mu": LC.fraction(emu[0], mu, dmu), "rs": LC.fraction(emu[1], rs, drs), "y": LC.fraction(emu[2], y, dy)}
    for m in LC.FWD_MUTANTS:
        if _applies(m, name, dt):
            mm, mr, my = LC.fwd64(x, g, b, mutant=m)
            worst = max(LC.fraction(mm.float(), mu, dmu), LC.fraction(mr.float(), rs, drs),
                        LC.fraction(LC.store(my, dt, m == "bf16_trunc"), y, dy))
            FRACTIONS.setdefault("mutant fwd " + m, []).append(worst)
            assert worst > 1, f"forward mutant {m} passes: {worst:.3f} of the bound"
    # backward, on the rounded statistics the kernel reads
    stats = LC.stats_of(x)
    depth = LC.param_depth(C, B * V // 4, seam)
    dgx, dgg, dgb, ref = LC.bwd_bounds(gl, x, stats, g, gadd, dt, depth)
    got = LC.emulate_bwd(gl, x, stats, g, gadd, dt, lanes=LC.lanes_of(LC.bwd_path(C, B * V // 4, seam)))
    fr.update(_bwd_fracs(got, ref, (dgx, dgg, dgb)))
    for m in LC.BWD_MUTANTS:
        if _applies(m, name, dt):
            mut = LC.bwd64(gl, x, stats, g, gadd, mutant=m)
            worst = max(_bwd_fracs((LC.store(mut["gx"], dt, m == "bf16_trunc"), mut["gg"], mut["gb"]), ref,
                                   (dgx, dgg, dgb)).values())
            FRACTIONS.setdefault("mutant bwd " + m, []).append(worst)
            assert worst > 1, f"backward mutant {m} passes: {worst:.3f} of the bound"
    print("fraction of the bound:", fr)
    for k, v in fr.items():
        FRACTIONS.setdefault(f"emulation {k} {dtype}", []).append(v)
        assert v <= 1, f"{k}: {v:.3f} of the bound"


def test_report_fractions():
    """(runs after the sweep above) the emulation's worst fraction per output, and how close each mutant came to passing"""
    rep = {k: (max(v) if k.startswith("emulation") else min(v)) for k, v in sorted(FRACTIONS.items())}
    print(json.dumps(rep, indent=1))
    assert all(v <= 1 for k, v in rep.items() if k.startswith("emulation"))
    assert all(v > 1 for k, v in rep.items() if k.startswith("mutant"))


# ------------------------------------------------------------------ seams and workspace ------------------------------------
def test_seams_are_consistent(lib, seam):
    rows = lambda q: LC.ws_rows(lib, 1, 64, 4 * q)
    assert rows(seam - 1) == (seam - 1 + 15) // 16 + 64          # SUB = 4: a row per 16 quads
    assert rows(seam) == max((seam + 63) // 64, 1024) + 64       # SUB = 1: a row per 64 quads (floor: 1024 rows)
    assert seam % 64 == 1 and (seam + 1) % 64 != 0               # the first quad of a new 64-quad workgroup; seam + 1 has a tail
    for C in LC.SLICE_C:                                         # one seam for every slice width and any batch split
        assert LC.ws_rows(lib, 1, C, 4 * (seam - 1)) > LC.ws_rows(lib, 1, C, 4 * seam)
    s = LC.rowsum_seams(lib.fz_rowsum_chunks)
    L, S = s["L"], s["S"]
    assert [lib.fz_rowsum_chunks(v) for v in (L, L + 1, 3 * L + 5)] == [1, 2, (3 * L + 5) // S]
    assert [lib.fz_rowsum_chunks(s[k]) for k in ("last_of_1", "first_of_2", "three_plus_4", "cap")] == [1, 2, 3, s["top"]]
    assert s["top"] == 64 and all(s[k] % 4 == 0 for k in ("last_of_1", "first_of_2", "three_plus_4", "cap"))


def test_workspace_covers_every_path(lib, seam):
    for C in (1, 32, 33, 63, 64, 96, 100, 128, 256, 320, 512, 1024):
        for B in (1, 2, 3):
            for q in (1, 15, 16, 17, 1000, 16384, 16400, seam - 1, seam, seam + 1, 4 * seam, 300000):
                quads = B * q
                need = LC.partial_rows(C, quads, seam) + 64
                assert LC.ws_rows(lib, B, C, 4 * q) >= need, (B, C, q)
    assert LC.partial_rows(64, seam - 1, seam) == 2044 and LC.partial_rows(64, seam, seam) == 512


# ------------------------------------------------------------------ argument checks (dummy pointers, no device) -------------
def test_argument_checks(lib):
    from factorizer_amd import _native
    p = ctypes.c_void_p(64)
    F32 = _native.STORE_F32
    E_SHAPE, E_UNSUPPORTED, E_ARG = -1, -2, -4
    err = lib.fz_last_error_string
    fwd = lambda **k: lib.fz_ln_fwd(*[k.get(n, p) for n in ("x", "g", "b", "y", "stats")], k.get("B", 1), k.get("C", 8),
                                    k.get("V", 16), 1e-5, k.get("dt", F32), None)
    bwd = lambda **k: lib.fz_ln_bwd(*[k.get(n, p) for n in ("gl", "x", "stats", "g", "gadd", "gx", "gpar", "ws")], k.get("B", 1),
                                    k.get("C", 8), k.get("V", 16), k.get("dt", F32), None)
    for n in ("x", "g", "b", "y"):
        assert fwd(**{n: None}) == E_ARG and b"fz_ln_fwd: null pointer" in err()
    for n in ("gl", "x", "stats", "g", "gx"):
        assert bwd(**{n: None}) == E_ARG and b"fz_ln_bwd: null pointer" in err()
    for f, name in ((fwd, b"fz_ln_fwd"), (bwd, b"fz_ln_bwd")):
        for bad in (dict(B=-1), dict(C=0), dict(V=0)):
            assert f(**bad) == E_SHAPE and name + b": bad sizes" in err()
        assert f(V=18) == E_UNSUPPORTED and b"multiple of 4" in err()
        assert f(dt=7) == E_ARG and b"act_dtype" in err()
    assert bwd(ws=None) == E_ARG and b"workspace" in err()
    n0 = lib.fz_launch_count()
    assert fwd(B=0) == 0 and bwd(B=0) == 0 and fwd(B=0, stats=None) == 0 and bwd(B=0, gadd=None, gpar=None, ws=None) == 0
    assert lib.fz_launch_count() == n0
    red = lambda part=p, rows=4, n=8, out=p: lib.fz_reduce_rows(part, rows, n, out, None, None)
    for bad in (dict(part=None), dict(out=None), dict(rows=0), dict(n=0), dict(rows=1 << 31)):
        assert red(**bad) == E_ARG and b"fz_reduce_rows" in err()
    rs = lambda x=p, part=p, out=p, B=1, C=2, V=16, dt=F32: lib.fz_rowsum(x, part, out, B, C, V, dt, None)
    for bad in (dict(x=None), dict(part=None), dict(out=None)):
        assert rs(**bad) == E_ARG and b"fz_rowsum: null pointer" in err()
    for bad in (dict(B=0), dict(C=0), dict(V=0), dict(V=18)):
        assert rs(**bad) == E_SHAPE and b"fz_rowsum: bad sizes" in err()
    assert rs(dt=7) == E_ARG and b"act_dtype" in err()
    assert lib.fz_launch_count() == n0


# ------------------------------------------------------------------ host tensors -------------------------------------------
def test_layernorm_on_cpu_tensors_agrees_with_the_oracle():
    import factorizer_amd as ft
    from factorizer_amd import pointwise as PW
    x, g, b, _, _ = LC.rounded("mean_30_std_half", 2, 6, 64, torch.float32)
    mu, rs, y = LC.fwd64(x, g, b)
    _, _, dy = LC.fwd_bounds(x, g, b, torch.float32)
    m = ft.LayerNorm(6)
    with torch.no_grad():
        m.norm.weight.copy_(g)
        m.norm.bias.copy_(b)
    with warnings.catch_warnings():
        warnings.simplefilter("error", RuntimeWarning)         # a host tensor is no fallback of a device one: no warning
        got = [m(x.view(2, 6, 4, 4, 4)).reshape(2, 6, 64), PW.layernorm_cf(x.view(2, 6, 4, 4, 4), g, b, LC.EPS).reshape(2, 6, 64)]
    for t in got:
        assert LC.fraction(t, y, dy) <= 1
