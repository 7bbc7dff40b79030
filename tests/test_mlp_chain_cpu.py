"""No GPU: the tools of tests/mlp_cases.py are checked before they judge a kernel.  The oracle equals float64 autograd of the
composed layers; the exact generators meet their conditions and the library's GELU formula, emulated in fp32, is exact on them;
the split-product emulations and an fp32 emulation of the chain stay under the bounds on every rounded family; every mutant
breaks them (bitwise on the exact cases; on the rounded family named in MUTANT_FAMILY); the seams and refusals the GPU tests
rely on are the host library's own answers."""
import ctypes
import json
import math

import pytest
import torch
import torch.nn.functional as F

import ln_cases as LC
import mlp_cases as MC

BF = torch.bfloat16
FRACTIONS = {}
# the rounded family on which each mutant exceeds its bound (and the storage type, where only one shows it)
MUTANT_FAMILY = {"ragged_last_quad_dropped": "same_sign", "tile_cap_skipped": "same_sign", "tile_cap_twice": "same_sign",
                 "prefetch_last_from_tile0": "randn", "dw1_no_affine": "randn", "no_residual": "randn", "tanh_gelu": "gelu_tails",
                 "gelu_grad_no_xpdf": "gelu_tails", "fp32_z1": "gelu_tails", "one_pass_var": "mean_1000",
                 "one_level_fewer": "same_sign"}


@pytest.fixture(scope="module")
def lib():
    from factorizer_amd import _native, build
    build.build(verbose=False)
    return _native.lib()


# ------------------------------------------------------------------ the oracle against float64 autograd --------------------
@pytest.mark.parametrize("C,H", [(32, 64), (32, 128), (64, 128)])
def test_oracle_equals_float64_autograd(C, H):
    B, V = 2, 12
    p = MC.rounded_chain("randn", B, C, H, V, torch.float32, pre=True, head=3)
    t = {k: v.double().requires_grad_(True) for k, v in p.items() if v is not None}
    lin = lambda w, x, b: torch.einsum("mk,bkv->bmv", w, x) + b.view(1, -1, 1)
    x1 = t["x"] + lin(t["wo"], t["a"], t["bo"])
    ln = F.layer_norm(x1.movedim(1, -1), (C,), t["g"], t["b"], MC.EPS).movedim(-1, 1)
    z1 = lin(t["w1"], ln, t["b1"])
    x2 = x1 + lin(t["w2"], F.gelu(z1), t["b2"])
    logits = lin(t["wh"], x2, t["bh"])
    ref = MC.fwd64(p)
    for k, v in (("x1", x1), ("ln", ln), ("z1", z1), ("x2", x2), ("logits", logits)):
        assert (ref[k] - v.detach()).abs().max() <= 1e-12 * max(1.0, float(v.detach().abs().max())), k
    # backward from x1 on (the inputs the kernel reads: z1, stats)
    x1l = x1.detach().requires_grad_(True)
    ln = F.layer_norm(x1l.movedim(1, -1), (C,), t["g"], t["b"], MC.EPS).movedim(-1, 1)
    z1l = lin(t["w1"], ln, t["b1"])
    z1l.retain_grad()
    x2 = x1l + lin(t["w2"], F.gelu(z1l), t["b2"])
    gs = torch.autograd.grad(x2, [z1l, x1l, t["g"], t["b"], t["w1"], t["b1"], t["w2"], t["b2"]], t["g2"].detach())
    stats = torch.stack([ref["mu"], ref["rs"]], 1)
    got = MC.bwd64(p["g2"].double(), z1l.detach(), x1l.detach(), stats, p["g"], p["b"], p["w1"], p["w2"])
    for k, v in zip(("gz1", "gx1", "gg", "gb", "gw1", "gb1", "gw2", "gb2"), gs):
        assert (got[k] - v).abs().max() <= 1e-12 * max(1.0, float(v.abs().max())), k


@pytest.mark.parametrize("ln", [False, True], ids=["out_proj", "in_proj"])
def test_dw_oracle_equals_float64_autograd(ln):
    B, V, C = 2, 12, 32
    gr, w, q, g, b, stats, gadd = MC.rounded_dw("randn", B, V, torch.float32, ln)
    qd, wd = q.double().requires_grad_(True), w.double().requires_grad_(True)
    lin = lambda w, x: torch.einsum("mk,bkv->bmv", w, x)
    if ln:
        gd, bd = g.double().requires_grad_(True), b.double().requires_grad_(True)
        y = lin(wd, F.layer_norm(qd.movedim(1, -1), (C,), gd, bd, MC.EPS).movedim(-1, 1))
        gx, gw, gg, gbt = torch.autograd.grad(y, [qd, wd, gd, bd], gr.double())
        mu = q.double().mean(1, keepdim=True)
        st64 = torch.cat([mu, ((q.double() - mu).pow(2).mean(1, keepdim=True) + MC.EPS).rsqrt()], 1)
        got = MC.dw64(gr, w, q, (g, b), st64, gadd)
        want = {"y": gx + gadd.double(), "gw": gw, "gg": gg, "gbt": gbt, "gb": gr.double().sum((0, 2))}
    else:
        bias = torch.zeros(C, dtype=torch.float64, requires_grad=True)
        y = lin(wd, qd) + bias.view(1, -1, 1)
        gx, gw, gb = torch.autograd.grad(y, [qd, wd, bias], gr.double())
        got = MC.dw64(gr, w, q)
        want = {"y": gx, "gw": gw, "gb": gb}
    for k, v in want.items():
        assert (got[k] - v).abs().max() <= 1e-12 * max(1.0, float(v.abs().max())), k


# ------------------------------------------------------------------ the GELU formula and d_erf -----------------------------
def test_library_gelu_formula_is_exact_at_16_and_d_erf_is_the_measured_one():
    z = torch.tensor([-16.0, 16.0])
    ge, gp = MC.emu_gelu(z), MC.emu_gelu_grad(z)
    assert ge.tolist() == [0.0, 16.0] and math.copysign(1.0, float(ge[0])) == -1.0 and gp.tolist() == [0.0, 1.0]
    assert torch.equal(ge.double(), MC.gelu64(z.double())) and torch.equal(gp.double(), MC.flush(MC.gelu_grad64(z.double())))
    assert float(MC.emu_gelu_grad(torch.tensor([-8.0]))) != 0.0          # ±8 would not do
    m = MC.measure_d_erf()
    print("d_erf measured", m)
    assert 1.5e-7 < m <= MC.D_ERF_MEASURED < 1.25 * m and MC.D_ERF == 2 * MC.D_ERF_MEASURED
    zz = torch.linspace(-12, 12, 200001, dtype=torch.float64).float()
    assert LC.fraction(MC.emu_gelu(zz), MC.gelu64(zz.double()), LC.SLACK * MC.dgelu(zz.double())) <= 1
    assert LC.fraction(MC.emu_gelu_grad(zz), MC.gelu_grad64(zz.double()), LC.SLACK * MC.dgelu_grad(zz.double())) <= 1
    assert float((MC.gelu_grad64(zz.double())).abs().max()) < MC.GELU_LIP


# ------------------------------------------------------------------ the exact generators -----------------------------------
@pytest.mark.parametrize("dtype", sorted(MC.DTYPES))
@pytest.mark.parametrize("C,H", [(32, 64), (32, 128), (64, 128)])
def test_exact_generator_is_exact(C, H, dtype):
    dt = MC.DTYPES[dtype]
    args = MC.exact_mlp_bwd(3, C, H, 260, dt, seed=2)
    assert all(t.dtype == dt for t in args[:3])
    ref = MC.bwd64(*args, out_dtype=dt)
    MC.check_exact(ref)
    assert float(ref["gl"].abs().max()) <= 2 and float(ref["gh"].abs().max()) <= 2 and torch.equal(ref["gl"], ref["gl"].round())
    assert float(ref["gw1"].abs().max()) > 0 and float(ref["gw2"].abs().max()) > 0 and float(ref["gz1"].float().abs().max()) > 0
    for mode, sum_mode in (("fp32", "fp32"), ("three", "two"), ("three", "fp32")):     # every product mode: the same bits
        emu = MC.emulate_bwd(*args, dt, mode, sum_mode)
        for k in ("gz1", "gx1"):
            assert torch.equal(emu[k], ref[k]), (k, mode)
        for k in ("gg", "gb", "gw1", "gb1", "gw2", "gb2"):
            assert torch.equal(emu[k].double(), ref[k]), (k, mode, sum_mode)


@pytest.mark.parametrize("dtype", sorted(MC.DTYPES))
@pytest.mark.parametrize("ln", [False, True], ids=["out_proj", "in_proj"])
def test_exact_dw_generator_is_exact(ln, dtype):
    dt = MC.DTYPES[dtype]
    gr, w, q, g, b, stats, gadd = MC.exact_dw(3, 260, dt, ln, seed=2)
    ref = MC.dw64(gr, w, q, (g, b) if ln else None, stats, gadd, out_dtype=dt)
    MC.check_exact(ref)
    assert float(ref["gl"].abs().max()) <= 2 and float(ref["gw"].abs().max()) > 0


def test_mutants_differ_bitwise_on_the_exact_cases():
    cap = 4
    for dt in (torch.float32, BF):
        args = MC.exact_mlp_bwd(cap + 2, 32, 64, 260, dt, seed=4)
        ref = MC.bwd64(*args, out_dtype=dt)
        keys = ("gz1", "gx1", "gg", "gb", "gw1", "gb1", "gw2", "gb2")
        for m in MC.BWD_MUTANTS:
            mut = MC.bwd64(*args, mutant=m, cap=cap, out_dtype=dt)
            same = all(torch.equal(mut[k], ref[k]) for k in keys)
            assert same == (m in ("tanh_gelu", "gelu_grad_no_xpdf")), (dt, m)      # (those two: mlp_cases.BWD_MUTANTS)
        for ln in (False, True):
            gr, w, q, g, b, stats, gadd = MC.exact_dw(cap + 2, 260, dt, ln, seed=4)
            a = (gr, w, q, (g, b) if ln else None, stats, gadd)
            ref = MC.dw64(*a, out_dtype=dt)
            for m in MC.TILE_MUTANTS + (["dw1_no_affine", "no_residual"] if ln else []):
                mut = MC.dw64(*a, mutant=m, cap=cap, out_dtype=dt)
                assert not all(torch.equal(mut[k], ref[k]) for k in ("y", "gw", "gb")), (dt, ln, m)


# ------------------------------------------------------------------ product modes ------------------------------------------
@pytest.mark.parametrize("name", MC.FAMILIES)
def test_split_products_under_their_bound_and_one_level_fewer_over_it(name):
    """u_prod of the module docstring: K = 32 and 64 channel products and a 256-voxel sum, fp32 operands of every family"""
    p = MC.rounded_chain(name, 1, 32, 64, 260, torch.float32)
    ops = [(p["w1"], p["x"][0]), (p["w2"], (p["w1"] @ p["x"][0])), (p["g2"][0, :, :256], p["x"][0, :, :256].t().contiguous())]
    for mode in ("fp32", "three", "two"):
        worst, worst_fewer = 0.0, 0.0
        for a, b in ops:
            ref, bound = a.double() @ b.double(), MC.dot_bound(a, b, mode)
            worst = max(worst, LC.fraction(MC.emu_dot(a, b, mode), ref, bound))
            if mode != "fp32":
                worst_fewer = max(worst_fewer, LC.fraction(MC.emu_dot(a, b, mode, fewer=True), ref, bound))
        FRACTIONS.setdefault(f"emulation dot {mode}", []).append(worst)
        assert worst <= 1, (mode, worst)
        if mode != "fp32" and name == MUTANT_FAMILY["one_level_fewer"]:
            FRACTIONS.setdefault(f"mutant one_level_fewer @{mode}", []).append(worst_fewer)
            assert worst_fewer > 1, (mode, worst_fewer)


# ------------------------------------------------------------------ the chain emulation against the bounds -----------------
ARMS = [(32, 64, "fp32", "fp32"), (32, 64, "three", "two"), (32, 128, "three", "fp32"), (64, 128, "three", "fp32")]


def _fr(got, ref, d, keys):
    return {k: LC.fraction(got[k], ref[k], d[k]) for k in keys if k in got and k in d}


@pytest.mark.parametrize("dtype", sorted(MC.DTYPES))
@pytest.mark.parametrize("C,H,mode,sum_mode", ARMS, ids=[f"c{a[0]}_h{a[1]}_{a[2]}_{a[3]}" for a in ARMS])
@pytest.mark.parametrize("name", MC.FAMILIES)
def test_emulation_under_the_bound_and_mutants_over_it(name, C, H, mode, sum_mode, dtype):
    dt = MC.DTYPES[dtype]
    cap, B, V = 2, 2, 260            # 4 tiles: tile `cap` exists
    p = MC.rounded_chain(name, B, C, H, V, dt, pre=True, head=3)
    # forward: the oracle reads the emulation's stored x1 and x2, as it reads the device's
    emu = MC.emulate_fwd(p, dt, mode)
    ref = MC.fwd64(p, x1_stored=emu["x1"], x2_stored=emu["x2"])
    ref["x1"] = MC.fwd64(p)["x1"]
    d = MC.fwd_bounds(p, emu["x1"], ref, dt, mode)
    fkeys = ("x1", "mu", "rs", "z1", "x2", "logits")
    fr = {"fwd " + k: v for k, v in _fr(emu, ref, d, fkeys).items()}
    for m in MC.FWD_MUTANTS:
        if MUTANT_FAMILY[m] == name:
            mut = MC.fwd64(p, x1_stored=emu["x1"], x2_stored=emu["x2"], mutant=m)
            mut["x1"] = MC.fwd64(p, mutant=m)["x1"]
            worst = max(_fr({k: (MC.store(mut[k], dt) if k in ("x1", "z1", "x2", "logits") else mut[k]) for k in fkeys}, ref, d, fkeys).values())
            FRACTIONS.setdefault("mutant " + m + " @fwd", []).append(worst)
            assert worst > 1, f"forward mutant {m} passes on {name}: {worst:.3f} of the bound"
    # backward: of the stored z1 and the rounded statistics the kernel reads
    x1, z1 = emu["x1"], emu["z1"]
    stats = torch.stack([emu["mu"], emu["rs"]], 1).contiguous()
    a = (p["g2"], z1, x1, stats, p["g"], p["b"], p["w1"], p["w2"])
    depth = max(MC.depth_rows(4), MC.depth_carried(4, cap))
    dn_rel, gadd_rel = MC.two_level_rel(sum_mode, dt)
    d, ref = MC.bwd_bounds(*a, dt, mode, sum_mode, depth, dn_rel=dn_rel, gadd_rel=gadd_rel)
    bkeys = ("gz1", "gx1", "gg", "gb", "gw1", "gb1", "gw2", "gb2")
    fr.update({"bwd " + k: v for k, v in _fr(MC.emulate_bwd(*a, dt, mode, sum_mode), ref, d, bkeys).items()})
    for m in MC.BWD_MUTANTS + ["fp32_z1"]:
        if MUTANT_FAMILY[m] != name or (m == "fp32_z1" and dt != BF):
            continue
        if m == "fp32_z1":       # the oracle given the pre-activation before its bf16 store
            z32 = MC.emulate_fwd(p, torch.float32, mode)["z1"]
            mut = MC.bwd64(p["g2"], z32, *a[2:])
        else:
            mut = MC.bwd64(*a, mutant=m, cap=cap)
        worst = max(_fr({k: (MC.store(mut[k], dt) if k in ("gz1", "gx1") else mut[k]) for k in bkeys}, ref, d, bkeys).values())
        FRACTIONS.setdefault("mutant " + m + " @bwd", []).append(worst)
        assert worst > 1, f"backward mutant {m} passes on {name}: {worst:.3f} of the bound"
    print("fraction of the bound:", fr)
    for k, v in fr.items():
        FRACTIONS.setdefault(f"emulation {k} {dtype}", []).append(v)
        assert v <= 1, f"{k}: {v:.3f} of the bound"


@pytest.mark.parametrize("dtype", sorted(MC.DTYPES))
@pytest.mark.parametrize("ln", [False, True], ids=["out_proj", "in_proj"])
@pytest.mark.parametrize("name", MC.FAMILIES)
def test_dw_emulation_under_the_bound_and_mutants_over_it(name, ln, dtype):
    dt = MC.DTYPES[dtype]
    cap, B, V = 2, 2, 260
    gr, w, q, g, b, stats, gadd = MC.rounded_dw(name, B, V, dt, ln)
    a = (gr, w, q, (g, b) if ln else None, stats, gadd)
    d, ref = MC.dw_bounds(*a, dt, MC.depth_carried(4, cap))
    gl = MC._emm(w.t(), gr, "fp32")
    flat = lambda t: t.float().permute(1, 0, 2).reshape(t.shape[1], -1)
    emu = {"gb": MC._vsum(gr)}
    if ln:
        emu["y"], emu["gg"], emu["gbt"] = LC.emulate_bwd(gl, q, stats, g, gadd, dt)
        n = (q.float() - stats[:, 0:1]) * stats[:, 1:2]
        emu["gw"] = g.view(1, -1) * (flat(gr) @ flat(n).t()) + b.view(1, -1) * emu["gb"].view(-1, 1)
    else:
        emu["y"], emu["gw"] = gl.to(dt), flat(gr) @ flat(q).t()
    keys = ("y", "gw", "gb", "gg", "gbt")
    fr = _fr(emu, ref, d, keys)
    for k, v in fr.items():
        FRACTIONS.setdefault(f"emulation dw {k} {dtype}", []).append(v)
        assert v <= 1, f"{k}: {v:.3f} of the bound"
    for m in MC.TILE_MUTANTS + (["dw1_no_affine", "no_residual"] if ln else []):
        if MUTANT_FAMILY[m] == name:
            mut = MC.dw64(*a, mutant=m, cap=cap)
            worst = max(_fr({k: (MC.store(v, dt) if k == "y" else v) for k, v in mut.items()}, ref, d, keys).values())
            FRACTIONS.setdefault("mutant " + m + " @dw", []).append(worst)
            assert worst > 1, f"gemm_dw mutant {m} passes on {name}: {worst:.3f} of the bound"


def test_every_mutant_is_judged_on_a_named_family():
    assert set(MUTANT_FAMILY) == set(MC.BWD_MUTANTS + MC.FWD_MUTANTS + ["fp32_z1", "one_level_fewer"])
    assert set(MUTANT_FAMILY.values()) <= set(MC.FAMILIES)


def test_report_fractions():
    """(runs after the sweeps above) the emulation's worst fraction per output, and how close each mutant came to passing"""
    rep = {k: (max(v) if k.startswith("emulation") else min(v)) for k, v in sorted(FRACTIONS.items())}
    print(json.dumps(rep, indent=1))
    assert all(v <= 1 for k, v in rep.items() if k.startswith("emulation"))
    assert all(v > 1 for k, v in rep.items() if k.startswith("mutant"))


# ------------------------------------------------------------------ seams and refusals (host library, no device) -----------
def test_seam_arithmetic_against_the_library(lib):
    from factorizer_amd import _native
    cw, cd = MC.cap_of_rows(lib.fz_mlp_wgrad_rows), MC.cap_of_rows(lib.fz_gemm_dw_rows)
    assert cw == MC.CAP_512 and cd == MC.CAP_512
    for cap in (MC.CAP_512, MC.CAP_768):
        for name, B, V, nt in MC.seam_bv(cap):
            assert MC.tiles(lib, B, V) == nt, name
            for C, H in ((32, 64), (32, 128), (64, 128)):
                assert lib.fz_mlp_supported(C, H, V) == 1
            rows = lib.fz_mlp_wgrad_rows(B, V)
            assert rows == min(nt, cw) == lib.fz_gemm_dw_rows(B, V)
            assert lib.fz_mlp_wgrad_workspace_bytes(B, V) >= 2 * rows * (4096 + 96 + 64) * 4     # kWgRow: S2 | S1 | db2, db1 | gln
            assert lib.fz_gemm_dw_workspace_bytes(B, V) >= rows * (1024 + 32 + 64) * 4           # kDwRow: S | sg | gln
    S = _native.PRODUCTS_SPLIT_BF16
    for name, B, V, nt in MC.PAIR_BV:
        assert MC.tiles(lib, B, V) == nt and nt % 2 == 0, name
        assert lib.fz_mlp_pre_supported(64, 128, V, S) == ((V + 255) // 256 % 2 == 0), name
    assert [nt // 2 for _, _, _, nt in MC.PAIR_BV[3:]] == [MC.CAP_PAIRS, MC.CAP_PAIRS + 1, 2 * MC.CAP_PAIRS + 1]
    b, v0, v1 = MC.tile_cols(1, 120)
    assert (b, v0, v1) == (1, 0, 120)                       # B = 2, V = 120: the pair (0, 1) lies in two samples
    assert [MC.tile_cols(t, 516)[0] for t in range(6)] == [0, 0, 0, 1, 1, 1]         # the pair (2, 3) straddles
    assert lib.fz_mlp_pre_supported(32, 64, 260, S) == 1 and lib.fz_mlp_pre_supported(32, 128, 260, S) == 0
    assert lib.fz_mlp_pre_supported(32, 64, 260, _native.PRODUCTS_FP32_MFMA) == 0
    assert lib.fz_mlp_pre_supported(64, 128, 120, S) == 0 and lib.fz_mlp_supported(32, 64, 18) == 0


def test_refusals_the_gpu_tests_rely_on(lib):
    from factorizer_amd import _native
    E_UNSUPPORTED = -2
    p = 64
    d = _native.MlpDesc()
    d.products, d.act_dtype = _native.PRODUCTS_SPLIT_BF16, _native.STORE_F32
    for f in ("w1", "w2", "b1", "b2", "ln_g", "ln_b", "stats", "z1", "out", "pre_in", "pre_w", "pre_b", "pre_res", "pre_out"):
        setattr(d, f, p)
    d.mode, d.B, d.C, d.H, d.V, d.ln_eps = 0, 1, 64, 128, 120, 1e-5          # PRE at C = 64 with an odd tile count
    n0 = lib.fz_launch_count()
    assert lib.fz_mlp_chain(ctypes.byref(d), None) == E_UNSUPPORTED and b"fz_mlp_pre_supported" in lib.fz_last_error_string()
    d = _native.MlpDesc()
    d.products, d.act_dtype = _native.PRODUCTS_SPLIT_BF16, _native.STORE_F32
    for f in ("inp", "w1", "w2", "ln_g", "ln_b", "stats", "z1", "x1", "out", "gln", "wpart", "gw1", "gb1", "gw2", "gb2", "glp"):
        setattr(d, f, p)
    d.mode, d.B, d.C, d.H, d.V = 2, 1, 64, 128, 256                          # mode 2 at C = 64
    assert lib.fz_mlp_chain(ctypes.byref(d), None) == E_UNSUPPORTED and b"C == 32" in lib.fz_last_error_string()
    assert lib.fz_launch_count() == n0
