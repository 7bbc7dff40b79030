"""No GPU: the tools of tests/gemm_cases.py and the host side of fz_gemm.

The float64 oracle against torch's own float64 operators (conv1d, conv3d, conv2d, conv_transpose3d, conv_transpose2d, layer_norm,
autograd for the LayerNorm-backward epilogue); the exactness conditions of the exact inputs; an fp32 and a split-bf16 emulation
under the a-priori bounds and every mutant of the oracle over them; the case table held to fz_gemm_plan — the library's own dry
run of its dispatcher — and to the literal table of every form the launchers can select; the dense layers of the README model
and of the BASELINE.json configs at their full sizes planned from shapes alone, each onto a tested form; and the descriptors
fz_gemm refuses before any launch."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

import gemm_cases as G
import ln_cases as LC

CPU_MAX = 1 << 21          # elements of the largest tensor a case may have to be evaluated on the CPU here
SMALL = [c for c in G.CASES if G.elements(c) <= CPU_MAX]


@pytest.fixture(scope="module")
def lib():
    from factorizer_amd import _native, build
    build.build(verbose=False)
    return _native.lib()


def small(name):
    c = G.BY_NAME[name]
    assert G.elements(c) <= CPU_MAX, name
    return c


# ------------------------------------------------------------------ the oracle against torch --------------------------------
def _torch_ref(c, t):
    """float64 result of the same layer from torch's operators"""
    A = G._weights(c, t)
    xs = [x.double() for x in t["x"]]
    B = xs[0].shape[0]
    x = torch.cat(xs, 1) if len(xs) == 2 else xs[0]
    bias = t["bias"].double() if c.bias else None
    if c.loader == "s2d":
        return _torch_epilogue(c, t, F.conv3d(x.view(B, c.Cin, c.D, c.H, c.W), A.view(c.M, c.Cin, 2, 2, 2), bias, stride=2).flatten(2))
    if c.loader == "k3":
        return _torch_epilogue(c, t, F.conv3d(x.view(B, c.Cin, c.D, c.H, c.W), A.view(c.M, c.Cin, 3, 3, 3), bias, padding=1).flatten(2))
    if c.loader == "s2d_2d":
        return _torch_epilogue(c, t, F.conv2d(x.view(B, c.Cin, c.H, c.W), A.view(c.M, c.Cin, 2, 2), bias, stride=2).flatten(2))
    if c.loader == "k3_2d":
        return _torch_epilogue(c, t, F.conv2d(x.view(B, c.Cin, c.H, c.W), A.view(c.M, c.Cin, 3, 3), bias, padding=1).flatten(2))
    if c.ln:
        x = F.layer_norm(x.transpose(1, 2), (c.K,), t["ln_g"].double(), t["ln_b"].double(), LC.EPS).transpose(1, 2)
    if c.bact:
        x = F.gelu(x) if c.bact == G.GELU else F.relu(x)
    if c.bmul:
        x = x * (t["bmul"].double() > 0)
    if c.epi == "d2s":
        O = c.M // 8
        w = A.view(O, 8, c.K).permute(2, 0, 1).reshape(c.K, O, 2, 2, 2)
        y = F.conv_transpose3d(x.view(B, c.K, *c.grid), w, bias, stride=2).flatten(2)
        return y + t["res"].double() if c.res else y
    if c.epi == "d2s_2d":
        O = c.M // 4
        w = A.view(O, 4, c.K).permute(2, 0, 1).reshape(c.K, O, 2, 2)
        y = F.conv_transpose2d(x.view(B, c.K, *c.grid), w, bias, stride=2).flatten(2)
        return y + t["res"].double() if c.res else y
    return _torch_epilogue(c, t, F.conv1d(x, A.unsqueeze(-1), bias))


def _torch_epilogue(c, t, y):
    if c.eact:
        y = F.gelu(y) if c.eact == G.GELU else F.relu(y)
    if c.emul is not None:
        e = t["emul"].double().requires_grad_(True)
        a = {0: e, G.RELU: F.relu(e), G.GELU: F.gelu(e)}[c.emul]
        y = y * torch.autograd.grad(a.sum(), e)[0]
    return y + t["res"].double() if c.res else y


TORCH_AT = ["bx_plain_mb2_n2", "bx_plain_mb1_n2_wt", "bx_gelu_mb1_n2", "bx_d2s_mb1_n2", "bx_ln_mb1", "bx_bmul_mb1", "bx_s2d_mb1_wt",
            "bx_c0_16", "bxk_emul_gelu", "res_k2_m1", "res_c0_k15", "res_k16_m40", "res_pf1_gelu", "res_eact_emul_relu",
            "res_pf1_relu", "res_respf_gelu", "res_d2s_k32", "res_d2s_relu", "str_s2d", "str_s2d_ks4_cin33", "str_s2d_2d", "str_s2d_2d_cin5", "str_s2d_2d_ks4_cin65", "str_k3_mb1", "str_k3_2d_mb1",
            "str_d2s_mb1", "str_d2s_2d_mb1", "head_m3"]


@pytest.mark.parametrize("name", TORCH_AT)
def test_oracle_against_torch(name):
    c = small(name)
    t = G.rounded(c, "randn", torch.float32)
    ref, want = G.ref64(c, t), _torch_ref(c, t)
    assert ref["y"].shape == want.shape
    scale = float(ref["terms"].max())
    assert float((ref["y"] - want).abs().max()) <= 1e-13 * scale, name
    if c.stats:
        mu = torch.cat([x.double() for x in t["x"]], 1).mean(1)
        assert torch.allclose(ref["mu"], mu, rtol=0, atol=1e-14) and float(ref["rs"].min()) > 0


@pytest.mark.parametrize("name", ["res_lnbwd_k32", "res_lnbwd_k64_gadd", "chain64_lnb"])
def test_lnbwd_oracle_against_autograd(name):
    c = small(name)
    t = G.rounded(c, "randn", torch.float32)
    ref = G.ref64(c, t)
    x = t["lnb_x"].double().requires_grad_(True)
    g = t["lnb_g"].double().requires_grad_(True)
    b = torch.zeros(c.M, dtype=torch.float64, requires_grad=True)
    # (the statistics the epilogue reads are the fp32-rounded ones: normalise with them, as the forward did)
    mu, rs = t["lnb_stats"][:, 0:1].double(), t["lnb_stats"][:, 1:2].double()
    gl = torch.einsum("mk,bkn->bmn", G._weights(c, t), t["x"][0].double())
    n = (x - mu) * rs
    gg, gb = torch.autograd.grad(n.detach() * g.view(1, -1, 1) + b.view(1, -1, 1), (g, b), gl)
    assert torch.allclose(ref["gg"], gg, rtol=1e-12, atol=1e-12) and torch.allclose(ref["gb"], gb, rtol=1e-12, atol=1e-12)
    y = F.layer_norm(x.transpose(1, 2), (c.M,), g, None, LC.EPS).transpose(1, 2)
    gx = torch.autograd.grad(y, x, gl)[0] + (t["lnb_gadd"].double() if c.gadd else 0)
    # autograd differentiates through float64 statistics, the oracle takes the stored fp32 ones: equal to fp32 rounding
    assert float((ref["y"] - gx).abs().max()) <= 1e-5 * float(gx.abs().max())


# ------------------------------------------------------------------ exact inputs --------------------------------------------
@pytest.mark.parametrize("c", [c for c in SMALL if G.has_exact(c)], ids=repr)
def test_exact_conditions(c):
    t = G.exact(c, torch.float32)
    ref = G.ref64(c, t)
    G.check_exact(c, t, ref)
    tb = G.exact(c, G.BF)           # bf16 storage holds the same values
    for k in t:
        a, b = (t[k], tb[k]) if k != "x" else (torch.cat(t[k], 1), torch.cat(tb[k], 1))
        assert torch.equal(a.double(), b.double()), (c.name, k)
    if c.epi != "lnbwd":            # the emulation of the kernels is exact on them too, in every product mode
        for prod in ("fp32", "three"):
            assert torch.equal(G.emulate(c, t, prod, torch.float32).double(), ref["y"]), (c.name, prod)
        assert torch.equal(G.emulate(c, tb, "three", G.BF), G.stored(c, ref, G.BF)), c.name


def test_gelu_is_exact_at_16():
    import mlp_cases as MC
    z = torch.tensor([16.0, -16.0])
    assert MC.emu_gelu(z).tolist() == [16.0, -0.0] and MC.emu_gelu_grad(z).tolist() == [1.0, 0.0]


# ------------------------------------------------------------------ emulation under the bounds, mutants over them -----------
EMU_AT = [n for n in G.ROUNDED_AT if G.elements(G.BY_NAME[n]) <= CPU_MAX and G.BY_NAME[n].epi != "lnbwd"]


@pytest.mark.parametrize("name", EMU_AT)
def test_emulation_within_bounds(name):
    c = G.BY_NAME[name]
    for mode in c.modes:
        dtype, prod, _ = G.MODES[mode]
        for fam in G.families_of(c):
            t = G.rounded(c, fam, dtype)
            bd, ref = G.bounds(c, t, mode, dtype)
            f = G.fraction(G.emulate(c, t, prod, dtype, pivot=c.ln and G.ln_order(c, mode) == "pivot"), ref["y"], bd["y"])
            assert f <= 1, (name, mode, fam, f)


def test_one_split_level_fewer_leaves_the_bound():
    c = G.BY_NAME["bx_plain_mb2_n4"]
    t = G.rounded(c, "same_sign", torch.float32)
    bd, ref = G.bounds(c, t, "fp32_split", torch.float32)
    assert G.fraction(G.emulate(c, t, "three", torch.float32, fewer=True), ref["y"], bd["y"]) > 1


@pytest.mark.parametrize("mutant", list(G.MUTANTS))
def test_mutants_are_caught(mutant):
    exact_at, rounded_at = G.MUTANTS[mutant]
    key = {"stats_rstd_as_var": "rs"}.get(mutant, "y")
    if exact_at is None:
        assert mutant in G.NO_EXACT
    else:
        assert mutant not in G.NO_EXACT
        c = small(exact_at)
        t = G.exact(c, torch.float32)
        ref = G.ref64(c, t)
        G.check_exact(c, t, ref)
        assert not torch.equal(G.ref64(c, t, mutant)[key], ref[key]), (mutant, exact_at)
    c = small(rounded_at)
    for mode in c.modes:
        dtype = G.MODES[mode][0]
        t = G.rounded(c, "randn", dtype)
        bd, ref = G.bounds(c, t, mode, dtype)
        got = G.ref64(c, t, mutant)[key]
        f = G.fraction(got if key != "y" else G.store(got, dtype), ref[key], bd[key])
        assert f > 1, (mutant, rounded_at, mode, f)


# ------------------------------------------------------------------ forms ---------------------------------------------------
def test_every_case_reaches_the_form_recorded_for_it(lib):
    assert set(G.REACHED) == {(c.name, m) for c in G.CASES for m in c.modes}
    wrong = {k: (G.plan(lib, G.BY_NAME[k[0]], k[1]), v) for k, v in G.REACHED.items() if G.plan(lib, G.BY_NAME[k[0]], k[1]) != v}
    assert not wrong, wrong


def test_the_table_reaches_every_form_the_launchers_can_select():
    got = {G.form_of(v) for v in G.REACHED.values()}
    assert got == G.FORMS, (sorted(G.FORMS - got), sorted(got - G.FORMS))


def test_seams_of_the_table():
    """what the issue asks of the shapes, read off the library's answers"""
    R = lambda n, m: G.REACHED[(n, m)]
    # tune = 0 on either side of the K-split rule and of the streaming form's 512-workgroup steps
    assert R("bxk_auto_4096", "fp32_split").startswith("bxk ") and R("bx_auto_4100", "fp32_split").startswith("bx_stream ")
    assert R("bxk_auto_8192_k512", "fp32_split").startswith("bxk ") and R("bx_auto_8192_k256", "fp32_split").startswith("bx_stream ")
    assert G.grid_of(R("bx_auto_n4_mb2", "fp32_split")) == (512, 1) and "mb2 nacc4" in R("bx_auto_n4_mb2", "fp32_split")
    assert "mb2 nacc2" in R("bx_auto_n2_mb2", "fp32_split") and "mb1 nacc2" in R("bx_auto_n2_mb1", "fp32_split")
    # mb = 2 falls back where mblocks % mb != 0; nine row blocks: RB = 8 and a second grid.y group
    assert "mb1" in R("bx_m96", "fp32_split") and G.BY_NAME["bx_m96"].tune % 10 == 2
    assert "rb=8" in R("res_m288", "fp32_mfma") and G.grid_of(R("res_m288", "fp32_mfma"))[1] == 2
    # the padded 1-D grid: 2 and 8 row-block groups, tile counts that are and are not multiples of 8
    for fam in ("bx", "str"):
        mode = "fp32_split" if fam == "bx" else "fp32_mfma"
        for g, tb in ((2, 64), (2, 65), (8, 71)):
            c = G.BY_NAME[f"{fam}_grid1d_g{g}_t{tb}"]
            assert G.grid_of(R(c.name, mode)) == ((tb + 7) // 8 * 8 * g, 1), c.name
    # the persistent kernel's threshold
    assert R("p32_4096_ln", "fp32_mfma").startswith("p32 ") and not R("p32_4095_not_taken", "fp32_mfma").startswith("p32")
    c = G.BY_NAME["p32_b3_ln_m3"]
    assert c.N % 128 and c.B * ((c.N + 127) // 128) >= 4096 and R(c.name, "fp32_mfma").startswith("p32 pf2")
    # every other tensor of the table stays below 10 MB in fp32 ... but for the threshold cases named here
    big = {c.name for c in G.CASES if 4 * G.elements(c) > 10e6}
    assert big <= {"bx_auto_n4_mb2", "bx_auto_n2_mb2", "bx_auto_n2_mb1", "bxk_auto_8192_k512", "p32_4095_not_taken", "p32_4096_ln",
                   "p32_b3_ln_m3", "p32_plain_eact"}, big


# ------------------------------------------------------------------ the workloads plan onto tested forms --------------------
def _model_layers(B, S, widths=(32, 64, 128, 256, 512), cin=4, cout=3):
    """the dense layers of a Factorizer U-shape by the call sites of factorizer_amd/pointwise.py, forward and input gradients,
    as shape-only cases: (B, S^3 or S = (D, H, W) volume; C doubles and the grid halves per stage; MLP hidden = 2 C)"""
    D, H, Wd = (S, S, S) if isinstance(S, int) else S
    out = [G.Case("stem", "k3", B=B, M=widths[0], Cin=cin, grid=(D, H, Wd)),
           G.Case("head", B=B, M=cout, Cin=widths[0], N=D * H * Wd)]
    for s, C in enumerate(widths):
        d, h, w = D >> s, H >> s, Wd >> s
        V, Hd = d * h * w, 2 * C
        L = lambda name, **kw: out.append(G.Case(f"s{s}_{name}", B=B, N=V, **kw))
        L("in_proj", M=C, Cin=C, ln=True, stats=True, eact=G.RELU, bias=False)
        L("out_proj", M=C, Cin=C)
        L("out_proj_res", M=C, Cin=C, res=True)
        L("fc1", M=Hd, Cin=C, ln=True, stats=True)
        L("fc2", M=C, Cin=Hd, bact=G.GELU, res=True)
        L("fc2_nores", M=C, Cin=Hd, bact=G.GELU)
        L("dgrad_fc2", M=Hd, Cin=C, w_t=1, emul=G.GELU, bias=False)
        L("dgrad_plain", M=C, Cin=C, w_t=1, bias=False)
        L("dgrad_fc1", M=C, Cin=Hd, w_t=1, bias=False)
        L("dgrad_gate", M=C, Cin=C, w_t=1, bmul=True, bias=False)
        if C <= 64:
            L("dgrad_lnbwd", epi="lnbwd", M=C, Cin=C, w_t=1, gadd=True)
            if C == 32:
                L("dgrad_lnbwd_fc1", epi="lnbwd", M=C, Cin=Hd, w_t=1, gadd=True)
                L("dgrad_lnbwd_nogadd", epi="lnbwd", M=C, Cin=C, w_t=1)
        if s + 1 < len(widths):
            C2, g2 = widths[s + 1], (d // 2, h // 2, w // 2)
            out.append(G.Case(f"s{s}_down", "s2d", B=B, M=C2, Cin=C, grid=g2))
            out.append(G.Case(f"s{s}_down_dgrad", epi="d2s", B=B, M=8 * C, Cin=C2, grid=g2, w_t=1, res=True, bias=False))
            out.append(G.Case(f"s{s}_up", epi="d2s", B=B, M=8 * C, Cin=C2, grid=g2, w_t=1))
            out.append(G.Case(f"s{s}_up_dgrad", "s2d", B=B, M=C2, Cin=C, grid=g2, bias=False))
            L("cat", M=C, Cin=2 * C, c0=C)
            L("cat_dgrad", M=C, Cin=C, w_t=1, pad=C, bias=False)
    return out


WORKLOADS = {   # README model / BASELINE.json configs[2], [3]: batch 2, 128^3; configs[1]: one C = 32 block at 128^3; configs[4]: batch 4,
    # 160 x 192 x 160, bf16 storage
    "swin_128_b2": (2, 128, ("fp32_split", "fp32_mfma")),
    "block_128_b1": (1, 128, ("fp32_split",)),
    "brats_160x192x160_b4_bf16": (4, (160, 192, 160), ("bf16",)),
}


@pytest.mark.parametrize("name", list(WORKLOADS))
def test_workloads_plan_onto_tested_forms(lib, name):
    B, S, modes = WORKLOADS[name]
    tested_any = {G.form_of(v) for v in G.REACHED.values()}
    untested = {}
    for c in _model_layers(B, S):
        for mode in modes:
            rc, text = G.plan_desc(lib, G.desc_of(c, mode))
            assert rc == 0, (c.name, mode, lib.fz_last_error_string())
            if G.form_of(text) not in tested_any:
                untested[(c.name, mode)] = text
    assert not untested, untested


# ------------------------------------------------------------------ refusals, before any launch -----------------------------
ARG, SHAPE, UNSUPPORTED = -4, -1, -2


def _codes():
    import re
    import os
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "factorizer_hip.h")).read()
    return {k: int(v) for k, v in re.findall(r"#define (FZ_E_[A-Z]+)\s+\(?(-?\d+)\)?", src)}


def test_error_codes_match_the_header():
    c = _codes()
    assert (c["FZ_E_ARG"], c["FZ_E_SHAPE"], c["FZ_E_UNSUPPORTED"]) == (ARG, SHAPE, UNSUPPORTED)


def _refused(lib, c, mode, want, word, **edit):
    """both fz_gemm_plan and fz_gemm itself refuse the edited descriptor with `want` (dummy pointers: a launch would fault here)"""
    d = G.desc_of(c, mode)
    for k, v in edit.items():
        if k == "x1":
            d.x[1] = v
        else:
            setattr(d, k, v)
    rc, text = G.plan_desc(lib, d)
    assert rc == want and text == "" and word in lib.fz_last_error_string(), (c.name, edit, rc, lib.fz_last_error_string())
    n0 = lib.fz_launch_count()
    assert lib.fz_gemm(ctypes.byref(d), None) == want and word in lib.fz_last_error_string()
    assert lib.fz_launch_count() == n0


def test_refusals(lib):
    B = G.BY_NAME
    for mode in ("fp32_mfma", "fp32_split"):
        two, one = B["bx_c0_16"], B["bx_tile_one"]
        _refused(lib, two, mode, ARG, b"x[1]", x1=None)
        for c0 in (0, -1, two.Cin, two.Cin + 1):
            _refused(lib, two, mode, UNSUPPORTED, b"c0", c0=c0)
        for c0 in (1, 16, one.Cin - 1, one.Cin + 1, -1):
            _refused(lib, one, mode, UNSUPPORTED, b"c0", c0=c0)
        for c in (B["bx_d2s_mb1_n2"], B["res_d2s_k32"], B["str_d2s_mb1"]):
            # (the resident kernel took LayerNorm + depth-to-space and dropped the W·β term: store_block's d2s form has none)
            _refused(lib, c, mode, UNSUPPORTED, b"depth-to-space", ln=1, ln_g=G.PTR, ln_b=G.PTR)
            _refused(lib, c, mode, UNSUPPORTED, b"depth-to-space", eact=G.RELU)
            _refused(lib, c, mode, UNSUPPORTED, b"depth-to-space", emul=G.PTR, emul_kind=G.RELU)
        for c in (one, B["res_k16_m40"], B["str_small_k16"], B["head_m3"]):
            _refused(lib, c, mode, UNSUPPORTED, b"stats_out", stats_out=G.PTR)
        # the rest of the (loader, epilogue) x field grid: what no kernel of that pairing reads
        for c in (B["str_s2d"], B["bx_s2d_mb1"], B["str_k3_mb1"]):
            _refused(lib, c, mode, UNSUPPORTED, b"input activation", bact=G.GELU)
            _refused(lib, c, mode, UNSUPPORTED, b"loader", ln=1, ln_g=G.PTR, ln_b=G.PTR)
            _refused(lib, c, mode, UNSUPPORTED, b"bmul", bmul=G.PTR, bmul_kind=G.RELU)
            _refused(lib, c, mode, UNSUPPORTED, b"loader", nsrc=2, x1=G.PTR, c0=2)
        for c in (B["str_s2d_2d"], B["str_k3_2d_mb1"], B["str_d2s_2d_mb1"]):
            for edit in (dict(eact=G.RELU), dict(emul=G.PTR), dict(bact=G.RELU), dict(ln=1, ln_g=G.PTR, ln_b=G.PTR), dict(stats_out=G.PTR),
                         dict(bmul=G.PTR, bmul_kind=G.RELU), dict(nsrc=2, x1=G.PTR, c0=2)):
                _refused(lib, c, mode, ARG, b"2-D", **edit)
        _refused(lib, B["str_s2d_2d"], mode, SHAPE, b"2-D", res=G.PTR)
        _refused(lib, B["str_k3_2d_mb1"], mode, SHAPE, b"2-D", res=G.PTR)
        _refused(lib, B["res_bmul"], mode, UNSUPPORTED, b"bmul", bact=G.RELU)
        _refused(lib, B["res_bmul"], mode, UNSUPPORTED, b"bmul", ln=1, ln_g=G.PTR, ln_b=G.PTR)
        _refused(lib, B["res_bmul"], mode, UNSUPPORTED, b"bmul", bmul_kind=G.GELU)
        # LayerNorm + input activation: the resident (pf 3) and the persistent kernel computed W (γ ∘ act(x̂)) + W β for it
        for c in (B["res_pf2_stats"], B["p32_4096_ln"], B["bx_ln_mb1"]):
            _refused(lib, c, mode, UNSUPPORTED, b"behind the LayerNorm", bact=G.GELU)
            _refused(lib, c, mode, UNSUPPORTED, b"behind the LayerNorm", bact=G.RELU)
        _refused(lib, B["res_pf2_stats"], mode, ARG, b"ln_g", ln_g=None)
        _refused(lib, B["res_pf2_stats"], mode, ARG, b"ln_g", ln_b=None)
        _refused(lib, one, mode, ARG, b"FZ_ACT", bact=3)
        _refused(lib, one, mode, ARG, b"FZ_ACT", eact=-1)
        _refused(lib, one, mode, ARG, b"FZ_ACT", emul=G.PTR, emul_kind=5)
        _refused(lib, one, mode, UNSUPPORTED, b"one source", src_mode=1)
        _refused(lib, one, mode, UNSUPPORTED, b"one source", nsrc=3)
        lnb = B["res_lnbwd_k32"]
        for edit in (dict(bias=G.PTR), dict(res=G.PTR), dict(eact=G.RELU), dict(emul=G.PTR), dict(ln=1, ln_g=G.PTR, ln_b=G.PTR), dict(lnb_x=None),
                     dict(M=40)):
            _refused(lib, lnb, mode, UNSUPPORTED, b"LayerNorm-backward", **edit)
        _refused(lib, B["chain64_lnb"], mode, UNSUPPORTED, b"added gradient", lnb_gadd=None)
        for act in (G.RELU, G.GELU):      # the 64-channel chain reads no input activation (the M = 32 form applies it: res_lnbwd_k32_relu)
            _refused(lib, B["chain64_lnb"], mode, UNSUPPORTED, b"no input activation", bact=act)
        # where a streaming kernel would have to combine two prologues, or take the ReLU prologue it does not compile
        _refused(lib, B["str_none_mb1_n1"], mode, UNSUPPORTED, b"ReLU input prologue", bact=G.RELU)
        _refused(lib, B["str_d2s_mb1"], mode, UNSUPPORTED, b"depth-to-space", bact=G.GELU)


def test_plan_launches_nothing_and_leaves_no_flag_behind(lib):
    c = G.BY_NAME["bx_tile_one"]
    n0 = lib.fz_launch_count()
    text = G.plan(lib, c, "fp32_split")
    assert text == G.REACHED[(c.name, "fp32_split")] and lib.fz_launch_count() == n0
    assert lib.fz_gemm_plan(None, None, 0) == ARG
    # B = 0: nothing to launch, FZ_OK and no form, as fz_gemm
    d = G.desc_of(c, "fp32_split")
    d.B = 0
    assert G.plan_desc(lib, d) == (0, "") and lib.fz_gemm(ctypes.byref(d), None) == 0 and lib.fz_launch_count() == n0
    # a short buffer is filled up to its capacity
    buf = ctypes.create_string_buffer(8)
    assert lib.fz_gemm_plan(ctypes.byref(G.desc_of(c, "fp32_split")), buf, 8) == 0 and buf.value == b"bx_stre"


def test_lnbwd_partial_rows(lib):
    for name, rows in (("res_lnbwd_k32", 2 * 2), ("chain64_lnb", 2 * 2)):
        c = G.BY_NAME[name]
        assert lib.fz_gemm_lnbwd_partials(ctypes.byref(G.desc_of(c, "fp32_mfma"))) == rows == G.grid_of(G.REACHED[(name, "fp32_mfma")])[0]
