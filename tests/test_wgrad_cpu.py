"""No GPU: the tools of tests/wgrad_cases.py are themselves checked.  The index-formula oracle of every loader agrees with the
framework's float64 convolution weight gradients; every exact case meets the conditions under which the float64 answer is the
only correct fp32 one; the restated seams (use_fast, pick_chunks, the finish form) agree with fz_wgrad_workspace_bytes and with
the literal table of reached paths, and no listed path lacks a case; every mutant changes its designated exact case and leaves
the a-priori bound on its rounded case; an fp32 emulation of the kernels stays inside the bounds; and fz_wgrad refuses the
descriptor fields its kernels do not honour before anything touches a device."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

import wgrad_cases as W
from factorizer_amd import _native
from factorizer_amd import pointwise as PW

F64 = torch.float64
_REFS = {}


def exact_ref(c):
    """(inputs, reference) of the exact case, computed once"""
    if c.name not in _REFS:
        t = W.exact(c, torch.float32)
        _REFS[c.name] = (t, W.ref64(c, t))
    return _REFS[c.name]


def _rand(*s):
    return torch.randn(*s, dtype=F64)


# ------------------------------------------------------------------ oracle against the framework --------------------------
def test_oracle_equals_the_framework_conv_weight_gradients():
    torch.manual_seed(3)
    close = lambda a, b: torch.testing.assert_close(a, b, rtol=1e-12, atol=1e-12)
    B, Cin, O = 2, 3, 5
    # k3, zero padding 1, on a grid whose 32-column tiles wrap rows and planes
    c = W.Case("k3", "k3", B=B, M=O, Cin=Cin, grid=(2, 3, 12))
    x, gy = _rand(B, Cin, 2, 3, 12), _rand(B, O, 2, 3, 12)
    r = W.ref64(c, {"p": gy.reshape(B, O, -1), "q": [x.reshape(B, Cin, -1)]})
    close(r["gw"].reshape(O, Cin, 3, 3, 3), torch.nn.grad.conv3d_weight(x, (O, Cin, 3, 3, 3), gy, padding=1))
    close(r["gb"], gy.sum((0, 2, 3, 4)))
    c = W.Case("k3_2d", "k3_2d", B=B, M=O, Cin=Cin, grid=(5, 12))
    x, gy = _rand(B, Cin, 5, 12), _rand(B, O, 5, 12)
    r = W.ref64(c, {"p": gy.reshape(B, O, -1), "q": [x.reshape(B, Cin, -1)]})
    close(r["gw"].reshape(O, Cin, 3, 3), torch.nn.grad.conv2d_weight(x, (O, Cin, 3, 3), gy, padding=1))
    # s2d in the k2s2 conv's role: P = gy on the coarse grid, Q = s2d(x)
    c = W.Case("s2d", "s2d", B=B, M=O, Cin=Cin, grid=(2, 3, 4))
    x, gy = _rand(B, Cin, 4, 6, 8), _rand(B, O, 2, 3, 4)
    r = W.ref64(c, {"p": gy.reshape(B, O, -1), "q": [x.reshape(B, Cin, -1)]})
    close(r["gw"].reshape(O, Cin, 2, 2, 2), torch.nn.grad.conv3d_weight(x, (O, Cin, 2, 2, 2), gy, stride=2))
    # ... and in the transposed conv's: P = x on the coarse grid, Q = s2d(gy), GW[c][(o, td, th, tw)]
    c = W.Case("s2d_t", "s2d", B=B, M=Cin, Cin=O, grid=(2, 3, 4), gbias=False)
    xc, gyf = _rand(B, Cin, 2, 3, 4), _rand(B, O, 4, 6, 8)
    wt = _rand(Cin, O, 2, 2, 2).requires_grad_(True)
    (gwt,) = torch.autograd.grad(F.conv_transpose3d(xc, wt, stride=2), [wt], gyf)
    r = W.ref64(c, {"p": xc.reshape(B, Cin, -1), "q": [gyf.reshape(B, O, -1)]})
    close(r["gw"].reshape(Cin, O, 2, 2, 2), gwt)
    c = W.Case("s2d_2d", "s2d_2d", B=B, M=O, Cin=Cin, grid=(3, 4))
    x, gy = _rand(B, Cin, 6, 8), _rand(B, O, 3, 4)
    r = W.ref64(c, {"p": gy.reshape(B, O, -1), "q": [x.reshape(B, Cin, -1)]})
    close(r["gw"].reshape(O, Cin, 2, 2), torch.nn.grad.conv2d_weight(x, (O, Cin, 2, 2), gy, stride=2))
    c = W.Case("s2d_2d_t", "s2d_2d", B=B, M=Cin, Cin=O, grid=(3, 4), gbias=False)
    xc, gyf = _rand(B, Cin, 3, 4), _rand(B, O, 6, 8)
    wt = _rand(Cin, O, 2, 2).requires_grad_(True)
    (gwt,) = torch.autograd.grad(F.conv_transpose2d(xc, wt, stride=2), [wt], gyf)
    r = W.ref64(c, {"p": xc.reshape(B, Cin, -1), "q": [gyf.reshape(B, O, -1)]})
    close(r["gw"].reshape(Cin, O, 2, 2), gwt)
    # plain with a two-source concat, ReLU'd input, ReLU-gated gradient: the Conv1d(k = 1) of relu(cat(x1, x2)) under a ReLU
    c = W.Case("cat", B=B, M=O, Cin=7, N=20, c0=3, qact=W.RELU, pmul=W.RELU)
    x1, x2, gy = _rand(B, 3, 20), _rand(B, 4, 20), _rand(B, O, 20)
    w, bias = _rand(O, 7, 1).requires_grad_(True), _rand(O).requires_grad_(True)
    y = F.conv1d(torch.relu(torch.cat([x1, x2], 1)), w, bias)
    gw, gb = torch.autograd.grad(torch.relu(y), [w, bias], gy)
    r = W.ref64(c, {"p": gy, "pmul": y.detach(), "q": [x1, x2]})
    close(r["gw"], gw[:, :, 0])
    close(r["gb"], gb)
    # LayerNorm statistics, GELU and the fold against autograd of W·gelu-free LN: z = W (γ x̂ + β) + b
    c = W.Case("ln", B=B, M=O, Cin=6, N=20, stats=True, ln=True)
    x, gy = _rand(B, 6, 20), _rand(B, O, 20)
    g, b = _rand(6), _rand(6)
    mu = x.mean(1, keepdim=True)
    rs = ((x - mu) ** 2).mean(1, keepdim=True).add(1e-5).rsqrt()
    w = _rand(O, 6, 1).requires_grad_(True)
    (gw,) = torch.autograd.grad(F.conv1d((x - mu) * rs * g.view(1, -1, 1) + b.view(1, -1, 1), w), [w], gy)
    r = W.ref64(c, {"p": gy, "q": [x], "stats": torch.cat([mu, rs], 1), "ln_g": g, "ln_b": b})
    close(r["gw"], gw[:, :, 0])
    c = W.Case("gelu", B=B, M=O, Cin=6, N=20, qact=W.GELU, pmul=W.GELU)
    e = F.conv1d(F.gelu(x), w)
    (gw,) = torch.autograd.grad(F.gelu(e), [w], gy)
    r = W.ref64(c, {"p": gy, "pmul": e.detach(), "q": [x]})
    close(r["gw"], gw[:, :, 0])


# ------------------------------------------------------------------ exactness ---------------------------------------------
@pytest.mark.parametrize("c", [c for c in W.ALL_CASES if c.B > 0], ids=repr)
def test_exact_preconditions(c):
    t, ref = exact_ref(c)
    W.check_exact(c, t, ref)
    tb = W.exact(c, W.BF)              # the same values under bf16 storage
    assert tb["p"].dtype == W.BF and torch.equal(tb["p"].float(), t["p"])
    assert all(torch.equal(a.float(), b) for a, b in zip(tb["q"], t["q"]))
    if c.pmul:
        assert torch.equal(tb["pmul"].float(), t["pmul"])
    if c.qact == W.GELU:               # the library's own GELU formula, operation by operation in fp32, is exact on ±16
        q = torch.cat(t["q"], 1)
        assert torch.equal(W.MC.emu_gelu(q).double(), W.MC.flush(W.MC.gelu64(q.double())))
    if c.pmul == W.GELU:
        assert torch.equal(W.MC.emu_gelu_grad(t["pmul"]).double(), W.MC.flush(W.MC.gelu_grad64(t["pmul"].double())))
    if c.stats and c.B > 1:            # statistics differ per sample and per column
        assert not torch.equal(t["stats"][0], t["stats"][1]) and not torch.equal(t["stats"][:, :, 0], t["stats"][:, :, 1])


def test_largest_tensor_is_small():
    for c in W.ALL_CASES:
        assert 4 * max(c.B, 1) * max(c.M * c.N, c.Cin * c.Vq) < 10 << 20, c.name


# ------------------------------------------------------------------ seams -------------------------------------------------
def test_restated_seams_equal_the_library_and_the_literal_table():
    lib = _native.lib()
    assert sorted(W.REACHED) == sorted(c.name for c in W.ALL_CASES)
    print()
    for c in W.ALL_CASES:
        p = W.plan(c)
        print(f"{c.name:32s} {c.loader:7s} {p[0]:8s} {p[1]:6s} finish {p[2]} nchunk {p[3]:4d} tiles/chunk {p[4]}")
        assert p == W.REACHED[c.name], c.name
        assert W.lib_nchunk(lib, c) == p[3], c.name
        assert p[3] == ((W.total_tiles(c) + p[4] - 1) // p[4] + 3) // 4
    for c in W.CASES:
        if c.name.startswith("out_"):      # one term of use_fast away from the register-operand kernel, and told apart from it
            assert W.plan(c)[0] == "generic" and W.plan(c, fast=True)[3] != W.plan(c)[3], c.name
    # ... and each of those fails exactly one term
    terms = {"out_m96": lambda c: c.M % 64, "out_k80": lambda c: c.K % 64, "out_n36": lambda c: c.N % 32, "out_c0_12": lambda c: c.c0 % 8,
             "out_pmul": lambda c: c.pmul, "out_stats_relu": lambda c: c.stats and c.qact}
    for name, term in terms.items():
        c = W.BY_NAME[name]
        assert term(c) and sum(bool(f(c)) for f in terms.values()) == 1, name


def test_every_listed_path_has_a_case():
    got = W.reached_paths(W.ALL_CASES)
    for what, want in W.PATHS.items():
        assert not want - got[what], (what, want - got[what])
    R = W.REACHED
    # chunking, for both kernels: 1, 3, 4, 5 tiles; units_target and one more; a walk across samples; three tiles a wave
    for k in "gf":
        assert [W.total_tiles(W.BY_NAME[f"{k}_tiles{n}"]) for n in ("1", "3", "4", "5_idle_waves")] == [1, 3, 4, 5]
        assert R[f"{k}_units_target"][4] == 1 and R[f"{k}_units_target+1"][4] == 2
        assert W.total_tiles(W.BY_NAME[f"{k}_units_target+1"]) % 2 == 1          # the last unit is short
    for name in ("g_tpc3_crosses_samples", "f_tpc2_crosses_samples"):
        c = W.BY_NAME[name]
        assert ((c.N + 31) // 32) % R[name][4] != 0 and R[name][4] >= 2
    assert R["g_tpc3_crosses_samples"][4] >= 3 and R["f_tpc3_m128"][4] >= 3
    # finish forms: chunk counts on both sides of every stride of the form's loops
    by_form = {w: {v[3] for n, v in R.items() if v[2] == w} for w in range(4)}
    assert {1, 33, 97, 129, 257, 512} <= by_form[0]
    assert {1, 4, 5, 16, 17, 65, 129, 256} <= by_form[2]
    assert {1, 3, 4, 5, 64} <= by_form[1] and {1, 3, 4, 5, 16} <= by_form[3]
    for w, stem in ((0, "fin0"), (2, "fin2"), (1, "fin1"), (3, "fin3")):
        cs = [c for c in W.CASES if c.name.startswith(stem) and R[c.name][2] == w]
        assert any(c.ln and c.gbias for c in cs) and any(c.ln and not c.gbias for c in cs) and any(c.acc for c in cs), stem
        assert any(c.ln and c.acc for c in cs) and any(not c.ln for c in cs), stem
    assert R["fin3_n5_offset_is_wide1"][2] == 1 and R["fin3_n5"][2] == 3 and R["fin1_n65_is_mid"][2] == 2
    # loaders: coarse grids (1,2,2), (2,2,6), Wo = 2, both roles; k3 with D = 1, W in {4, 12, 20}, Cin in {1, 3, 4}
    s2d = [c for c in W.CASES if c.loader == "s2d"]
    assert {(c.D // 2, c.Ho, c.Wo) for c in s2d} >= {(1, 2, 2), (2, 2, 6)} and any(c.Wo == 2 and c.N > 4 for c in s2d)
    assert any(c.gbias for c in s2d) and any(not c.gbias for c in s2d)
    k3 = [c for c in W.CASES if c.loader == "k3"]
    assert any(c.D == 1 for c in k3) and {c.W for c in k3} >= {4, 12, 20} and {c.Cin for c in k3} >= {1, 3, 4}
    assert any(c.N > 32 and 32 % c.W and 32 % (c.H * c.W) for c in k3)           # a tile wraps rows and planes
    # concat: a multiple of 8 on the register-operand kernel; not a multiple of 8, and c0 = 4, on the generic one
    cat = {c.name: c for c in W.CASES if c.c0}
    assert any(R[n][0] == "fast" and c.c0 % 8 == 0 for n, c in cat.items())
    assert any(R[n][0] == "generic" and c.c0 % 8 and c.c0 != 4 for n, c in cat.items()) and any(c.c0 == 4 for c in cat.values())
    # groups: 2, 3 and 4 problems, different grids, mixed prologues, an empty member, a member off the register-operand kernel
    assert {len(ms) for _, ms in W.GROUPS} == {2, 3, 4}
    for name, ms in W.GROUPS:
        fast = [R[m.name][0] == "fast" and m.B > 0 for m in ms]
        assert all(fast) == (name in ("grp2", "grp3", "grp4")), name
        if all(fast):
            assert len({(m.M, m.K, m.B * m.N) for m in ms}) == len(ms) and len({W.prologue_of(m) for m in ms}) >= 2


# ------------------------------------------------------------------ mutants -----------------------------------------------
@pytest.mark.parametrize("mutant", [m for m, (e, _) in W.MUTANTS.items() if e], ids=str)
def test_mutant_changes_its_exact_case(mutant):
    c = W.BY_NAME[W.MUTANTS[mutant][0]]
    t, ref = exact_ref(c)
    mut = W.ref64(c, t, mutant)
    differs = not torch.equal(mut["gw"], ref["gw"]) or (c.gbias and not torch.equal(mut["gb"], ref["gb"]))
    assert differs, mutant


def _fractions(c, t, mode, dtype, gw, gb):
    bd, ref = W.bounds(c, t, mode, dtype)
    f = {"gw": W.fraction(gw, ref["gw"], bd["gw"])}
    if c.gbias:
        f["gb"] = W.fraction(gb, ref["gb"], bd["gb"])
    return f


@pytest.mark.parametrize("family", W.FAMILIES)
@pytest.mark.parametrize("mutant", list(W.MUTANTS), ids=str)
def test_mutant_leaves_the_bound_on_its_rounded_case(mutant, family):
    c = W.BY_NAME[W.MUTANTS[mutant][1]]
    for mode, (dtype, prod) in W.MODES.items():
        t = W.rounded(c, family, dtype)
        mut = W.ref64(c, t, mutant)
        f = _fractions(c, t, prod, dtype, mut["gw"], mut["gb"])
        assert max(f.values()) > 1, (mutant, mode, f)


@pytest.mark.parametrize("name", ["f_m64_k64", "g64x64_m96_k80_n36", "fin2_n4", "fin2_n17", "k3_w12_cin3"])
def test_one_split_level_fewer_leaves_the_bound(name):
    """two levels where the kernels multiply three: on operands whose low parts all have one sign the dropped terms add up.
    (Judged where a wave walks one tile, depth 39 to 69, at 1.7 to 3.2 times the bound: the bound is the worst case of a
    sequential sum and grows with the depth, at the 103 terms of f_units_target+1 the two-level products lose 0.7 of it.)"""
    c = W.BY_NAME[name]
    t = W.rounded(c, "same_sign", torch.float32)
    gw, gb = W.emulate(c, t, "three", torch.float32, fewer=True)
    assert _fractions(c, t, "three", torch.float32, gw, gb)["gw"] > 1
    gw, gb = W.emulate(c, t, "three", torch.float32)
    assert _fractions(c, t, "three", torch.float32, gw, gb)["gw"] <= 1


# ------------------------------------------------------------------ emulation inside the bounds ---------------------------
@pytest.mark.parametrize("mode", list(W.MODES))
@pytest.mark.parametrize("name", W.ROUNDED_AT)
def test_emulated_kernels_stay_inside_the_bounds(name, mode):
    c = W.BY_NAME[name]
    dtype, prod = W.MODES[mode]
    for family in W.FAMILIES:
        t = W.rounded(c, family, dtype)
        gw, gb = W.emulate(c, t, prod, dtype)
        f = _fractions(c, t, prod, dtype, gw, gb)
        assert max(f.values()) <= 1, (family, f)


# ------------------------------------------------------------------ refusals ----------------------------------------------
PLAIN = dict(loader=0, Cin=8, K=8, M=16, N=64, Vq=64)
S2D = dict(loader=PW.LOAD_S2D, Cin=8, K=64, M=16, D=4, H=4, W=8, Ho=2, Wo=4, N=16, Vq=128)
K3 = dict(loader=PW.LOAD_K3, Cin=2, K=54, M=16, D=2, H=4, W=8, N=64, Vq=64)
REFUSED = [
    ("no source", dict(PLAIN, nsrc=0)), ("three sources", dict(PLAIN, nsrc=3)), ("src_mode", dict(PLAIN, src_mode=1)),
    ("s2d two sources", dict(S2D, nsrc=2, c0=4)), ("s2d statistics", dict(S2D, stats=256)), ("s2d activation", dict(S2D, qact=1)),
    ("k3 two sources", dict(K3, nsrc=2, c0=1)), ("k3 statistics", dict(K3, stats=256)), ("k3 activation", dict(K3, qact=2)),
    ("split at 0", dict(PLAIN, nsrc=2, c0=0)), ("split at Cin", dict(PLAIN, nsrc=2, c0=8)), ("split beyond Cin", dict(PLAIN, nsrc=2, c0=9)),
    ("negative split", dict(PLAIN, nsrc=2, c0=-1)),
    # one source with a split: the generic loader would read the null q[1] for channels >= c0, or stride q[0] by c0 channels
    ("one source split inside", dict(PLAIN, c0=4)), ("one source split beyond", dict(PLAIN, c0=9)), ("one source negative split", dict(PLAIN, c0=-1)),
]


def _wgrad_desc(**kw):
    d = _native.WgradDesc()
    d.p = d.q[0] = d.gw = 256            # never dereferenced: every case below is refused by the host checks
    d.nsrc, d.B = 1, 1
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def _refusal_desc(kw):
    d = _wgrad_desc(**kw)
    if kw.get("nsrc") == 2:
        d.q[1] = 256
    return d


@pytest.mark.parametrize("what,kw", REFUSED, ids=[r[0] for r in REFUSED])
@pytest.mark.parametrize("store", ["fp32", "bf16"])
def test_fz_wgrad_refuses_what_its_kernels_ignore(what, kw, store):
    lib = _native.lib()
    d = _refusal_desc(kw)
    d.act_dtype = _native.STORE_F32 if store == "fp32" else _native.STORE_BF16
    assert lib.fz_wgrad(ctypes.byref(d), ctypes.c_void_p(256), None) == -2, lib.fz_last_error_string()   # FZ_E_UNSUPPORTED
    assert b"fz_wgrad" in lib.fz_last_error_string()
    # ... and as a member of a group, before anything is launched
    ok = _wgrad_desc(**PLAIN)
    ok.act_dtype = d.act_dtype
    descs = (ctypes.POINTER(_native.WgradDesc) * 2)(ctypes.pointer(d), ctypes.pointer(ok))
    wss = (ctypes.c_void_p * 2)(256, 256)
    assert lib.fz_wgrad_group(descs, wss, 2, None) == -2 and b"fz_wgrad" in lib.fz_last_error_string()


def test_fz_wgrad_still_takes_what_the_package_passes():
    """the descriptors of wgrad_cases (one per shape the package builds) pass the host checks up to the launch: with B = 0
    fz_wgrad returns FZ_OK after wgrad_plan without touching the device"""
    lib = _native.lib()
    for c in W.ALL_CASES:
        d = W.desc_of(c)
        d.B = 0
        assert lib.fz_wgrad(ctypes.byref(d), ctypes.c_void_p(256), None) == 0, (c.name, lib.fz_last_error_string())
    d = W.desc_of(W.BY_NAME["f_cat_c0_24"])
    d.q[1] = None
    d.B = 0
    assert lib.fz_wgrad(ctypes.byref(d), ctypes.c_void_p(256), None) == -4     # FZ_E_ARG: a null second source
