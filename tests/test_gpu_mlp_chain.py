"""-m gpu: every dispatch arm of the chained MLP (fz_mlp_chain: csrc/mlp_chain32.hip, mlp_chain64.hip, mlp_chain_wg.hip) and of
the fused input + weight gradient (fz_gemm_dw: csrc/gemm_dw.hip) against the float64 closed forms of tests/mlp_cases.py,
evaluated on the device, at the seams of the persistent tile walk: 1 tile of 4 columns, one full tile, a full and a 4-column tile,
and cap, cap + 1 and 2 cap + 1 tiles of every launcher's resident-workgroup cap (reached by the batch count at V = 4 / 260; the
tile count is asserted against the cap before each launch).  Exact sweeps (backward arms): inputs whose only correct answer is
the float64 one, bit for bit — a skipped or doubled tile, a prefetch from the wrong tile, a dropped quad, accumulators that do
not carry over, a partial row that does not reach the row reduction all change bits.  Rounded sweeps (every arm, every input
family of mlp_cases.FAMILIES): element-wise under the a-priori bounds, the achieved fraction recorded.  The test ids name the arm:
  chain32  fwd_fp32_mfma_h64 | fwd_split_h64 | fwd_split_h64_pre | ..._pre_head<M>[_nobias] | fwd_h128 | bwd_h64 | bwd_h128
  chain64  p512_fwd | p512_fwd_pre | p512_bwd (512 threads, pairs of tiles) | p256_{fwd,bwd}_odd_tiles | p256_{fwd,bwd}_fp32_mfma
  chain_wg h64_two_level | h64_fp32_mfma | h128_split | h128_fp32_mfma (both halves, the glp buffer)
  gemm_dw  out_proj_bias | in_proj_ln_gadd;  chain64_lnb: the 64 -> 64 dgrad + LayerNorm backward at the same seams"""
import pytest
import torch

import ln_cases as LC
import mlp_cases as MC
import parity as P
from factorizer_amd import _native
from factorizer_amd import pointwise as PW

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BF = torch.bfloat16
DT = sorted(MC.DTYPES)
DEFAULT, SPLIT, FP32 = _native.PRODUCTS_DEFAULT, _native.PRODUCTS_SPLIT_BF16, _native.PRODUCTS_FP32_MFMA
PNAME = {DEFAULT: "default", SPLIT: "split_bf16", FP32: "fp32_mfma"}


def is_split(products):
    return products == SPLIT or (products == DEFAULT and _native.lib().fz_gemm_bx_enable(-1) != 0)


def odd(seams):
    return [s for s in seams if s[3] % 2 == 1]


S512, S768 = MC.seam_bv(MC.CAP_512), MC.seam_bv(MC.CAP_768)
# arm -> C, H, what runs, the products it is reached with, its cap (in tiles, or pairs for p512), its seams, and the product
# modes of its bounds: `mode` of the channel GEMMs, `sums` of the weight-gradient passes (mlp_cases.U_PROD)
ARMS = {
    "chain32_fwd_fp32_mfma_h64": dict(C=32, H=64, run="fwd", products=[FP32], cap=MC.CAP_768, seams=S768, mode="fp32"),
    "chain32_fwd_split_h64": dict(C=32, H=64, run="fwd", products=[DEFAULT, SPLIT], cap=MC.CAP_512, seams=S512, mode="three"),
    "chain32_fwd_split_h64_pre": dict(C=32, H=64, run="pre", products=[DEFAULT, SPLIT], cap=MC.CAP_512, seams=S512, mode="three"),
    "chain32_fwd_h128": dict(C=32, H=128, run="fwd", products=[DEFAULT, SPLIT, FP32], cap=MC.CAP_512, seams=S512, mode="fp32"),
    "chain32_bwd_h64": dict(C=32, H=64, run="bwd", products=[DEFAULT, SPLIT, FP32], cap=MC.CAP_768, seams=S768, mode="fp32"),
    "chain32_bwd_h128": dict(C=32, H=128, run="bwd", products=[DEFAULT, SPLIT, FP32], cap=MC.CAP_512, seams=S512, mode="fp32"),
    "chain64_p512_fwd": dict(C=64, H=128, run="fwd", products=[DEFAULT, SPLIT], cap=MC.CAP_PAIRS, seams=MC.PAIR_BV, mode="three", pairs=True),
    "chain64_p512_fwd_pre": dict(C=64, H=128, run="pre", products=[DEFAULT, SPLIT], cap=MC.CAP_PAIRS, seams=MC.PAIR_BV, mode="three", pairs=True),
    "chain64_p512_bwd": dict(C=64, H=128, run="bwd", products=[DEFAULT, SPLIT], cap=MC.CAP_PAIRS, seams=MC.PAIR_BV, mode="three", pairs=True),
    "chain64_p256_fwd_odd_tiles": dict(C=64, H=128, run="fwd", products=[DEFAULT, SPLIT], cap=MC.CAP_512, seams=odd(S512), mode="three"),
    "chain64_p256_bwd_odd_tiles": dict(C=64, H=128, run="bwd", products=[DEFAULT, SPLIT], cap=MC.CAP_512, seams=odd(S512), mode="three"),
    "chain64_p256_fwd_fp32_mfma": dict(C=64, H=128, run="fwd", products=[FP32], cap=MC.CAP_512, seams=S512, mode="fp32"),
    "chain64_p256_bwd_fp32_mfma": dict(C=64, H=128, run="bwd", products=[FP32], cap=MC.CAP_512, seams=S512, mode="fp32"),
    "chain_wg_h64_two_level": dict(C=32, H=64, run="wg", products=[DEFAULT, SPLIT], cap=MC.CAP_512, seams=S512, mode="three", sums="two"),
    "chain_wg_h64_fp32_mfma": dict(C=32, H=64, run="wg", products=[FP32], cap=MC.CAP_512, seams=S512, mode="fp32", sums="fp32"),
    "chain_wg_h128_split": dict(C=32, H=128, run="wg", products=[DEFAULT, SPLIT], cap=MC.CAP_512, seams=S512, mode="three", sums="fp32"),
    "chain_wg_h128_fp32_mfma": dict(C=32, H=128, run="wg", products=[FP32], cap=MC.CAP_512, seams=S512, mode="fp32", sums="fp32"),
}
for _m in (1, 3, 4):
    for _bias in (True, False):
        ARMS[f"chain32_fwd_split_h64_pre_head{_m}" + ("" if _bias else "_nobias")] = dict(
            ARMS["chain32_fwd_split_h64_pre"], head=_m, head_bias=_bias, products=[SPLIT])
FWD_ARMS = [k for k, a in ARMS.items() if a["run"] in ("fwd", "pre")]
BWD_ARMS = [k for k, a in ARMS.items() if a["run"] in ("bwd", "wg")]
BKEYS = {"bwd": ("gz1", "gx1", "gg", "gb"), "wg": ("gx1", "gg", "gb", "gw1", "gb1", "gw2", "gb2")}


def arm_products():
    return [pytest.param(k, p, id=f"{k}-{PNAME[p]}") for k, a in ARMS.items() for p in a["products"]]


def check_seam(arm, products, seam):
    """the (B, V) of a seam: its tile count against the arm's cap and the form the dispatch takes, from the library's answers"""
    a, lib = ARMS[arm], _native.lib()
    name, B, V, nt = seam
    assert MC.tiles(lib, B, V) == nt and PW._mlp_chain_ok(a["C"], a["H"], V)
    work, cap = (nt // 2, a["cap"]) if a.get("pairs") else (nt, a["cap"])
    want = {"cap": cap, "cap+1": cap + 1, "2cap+1": 2 * cap + 1, "cap+2_v260": cap + 2, "cap_pairs": cap, "cap+1_pairs": cap + 1,
            "2cap+1_pairs": 2 * cap + 1}.get(name)
    assert want is None or work == want, (name, work, cap)
    if a["C"] == 64:         # chain64_launch: p512 = split products and an even tile count
        assert (is_split(products) and nt % 2 == 0) == bool(a.get("pairs")), (arm, nt)
    if a["run"] == "wg":
        assert lib.fz_mlp_wgrad_rows(B, V) == min(nt, cap) and PW._mlp_wgrad_fused_ok(a["C"], a["H"], V)
    if a["C"] == 32 and a["run"] == "fwd" and a["H"] == 64:
        assert is_split(products) == (cap == MC.CAP_512)
    if a["run"] == "pre":
        assert PW._outproj_mlp_ok(a["C"], a["H"], V)
    return B, V, nt


def launched(n0, exactly=None):
    n = _native.launch_count() - n0
    assert n >= 1 if exactly is None else n == exactly, n


def run_bwd(kind, args):
    g2, z1, x1, st, g, b, w1, w2 = args
    n0 = _native.launch_count()
    if kind == "bwd":
        out = dict(zip(BKEYS["bwd"], PW._mlp_bwd_chain(g2, z1, w1, w2, x1, st, g)))
    else:
        out = dict(zip(BKEYS["wg"], PW._mlp_bwd_chain_wgrad(g2, z1, w1, w2, x1, st, g, b)))
    launched(n0)
    return out


def run_fwd(a, p):
    """dict x2, z1, st (+ x1, logits) of one forward launch"""
    n0 = _native.launch_count()
    if a["run"] == "fwd":
        o = dict(zip(("x2", "z1", "st"), PW._mlp_fwd_chain(p["x"], p["g"], p["b"], MC.EPS, p["w1"], p["b1"], p["w2"], p["b2"])))
    else:
        head = (p["wh"], p["bh"]) if "wh" in p else None
        o = dict(zip(("x1", "x2", "z1", "st", "logits"), PW._outproj_mlp_fwd_chain(
            p["a"], p["wo"], p["bo"], p["x"], p["g"], p["b"], MC.EPS, p["w1"], p["b1"], p["w2"], p["b2"], head=head)))
    launched(n0, exactly=1)
    return o


def same(a, b):
    return all(torch.equal(a[k], b[k]) for k in a)


# ------------------------------------------------------------------ (a) exact backward, every seam ------------------------
@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("arm,products", [p for p in arm_products() if p.values[0] in BWD_ARMS])
def test_exact_backward(arm, products, dtype):
    a, dt = ARMS[arm], MC.DTYPES[dtype]
    for seam in a["seams"]:
        B, V, nt = check_seam(arm, products, seam)
        args = MC.exact_mlp_bwd(B, a["C"], a["H"], V, dt, device=DEV)
        ref = MC.bwd64(*args, out_dtype=dt)
        MC.check_exact(ref)
        with _native.use_products(products):
            got = run_bwd(a["run"], args)
            if seam[0] in ("v260", "2cap+1", "2cap+1_pairs"):
                assert same(got, run_bwd(a["run"], args)), (seam[0], "replay")
        for k in BKEYS[a["run"]]:
            r = ref[k] if k in ("gz1", "gx1") else ref[k].float()
            assert got[k].dtype == r.dtype and got[k].shape == r.shape, k
            assert torch.equal(got[k], r), f"{seam[0]} (B {B}, V {V}, {nt} tiles) {k}: {int((got[k] != r).sum())} of {r.numel()} elements differ"


@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("form", ["out_proj_bias", "in_proj_ln_gadd"])
def test_exact_gemm_dw(form, dtype):
    lib, dt, ln = _native.lib(), MC.DTYPES[dtype], form == "in_proj_ln_gadd"
    cap = MC.cap_of_rows(lib.fz_gemm_dw_rows)
    for name, B, V, nt in MC.seam_bv(cap):
        assert MC.tiles(lib, B, V) == nt and lib.fz_gemm_dw_rows(B, V) == min(nt, cap) and PW._dw_fused_ok(32, V)
        gr, w, q, g, b, st, gadd = MC.exact_dw(B, V, dt, ln, device=DEV)
        ref = MC.dw64(gr, w, q, (g, b) if ln else None, st, gadd, out_dtype=dt)
        MC.check_exact(ref)
        run = (lambda: PW._gemm_dw(gr, w, q, ln=(g, b), stats=st, gadd=gadd)) if ln else (lambda: PW._gemm_dw(gr, w, q, want_bias=True))
        n0 = _native.launch_count()
        y, gw, gb, gg, gbt = run()
        launched(n0)
        got = {"y": y, "gw": gw, "gb": gb, "gg": gg, "gbt": gbt}
        for k in ("y", "gw") + (("gg", "gbt") if ln else ("gb",)):
            r = ref[k] if k == "y" else ref[k].float()
            assert torch.equal(got[k], r), f"{name} (B {B}, V {V}, {nt} tiles) {k}: {int((got[k] != r).sum())} elements differ"
        if name in ("v260", "2cap+1"):
            assert all(x is None or torch.equal(x, y2) for x, y2 in zip((y, gw, gb, gg, gbt), run()))


@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("products", [SPLIT, FP32], ids=["split_bf16", "fp32_mfma"])
def test_exact_chain64_lnb_seams(products, dtype):
    """chain64_lnb_launch (the SINGLE form of gemm_chain64_kernel behind PW._dgrad_lnbwd at 64 -> 64) at the seams of its cap"""
    lib, dt = _native.lib(), MC.DTYPES[dtype]
    for name, B, V, nt in S512:
        assert MC.tiles(lib, B, V) == nt
        gz, w2, gl, x, st, g, gadd = LC.exact_dgrad(B, 64, 64, V, dt, device=DEV)
        ref = LC.bwd64(gl, x, st, g, gadd, out_dtype=dt)
        assert ref["representable"] and float(ref["gg_terms"].max()) < 2 ** 22
        n0 = _native.launch_count()
        with _native.use_products(products):
            gx, gg, gb = PW._dgrad_lnbwd(gz, w2, x, st, g, gadd)
        launched(n0)
        assert torch.equal(gx, ref["gx"]) and torch.equal(gg.double(), ref["gg"]) and torch.equal(gb.double(), ref["gb"]), name


# ------------------------------------------------------------------ (b) rounded, every arm and family ---------------------
def _close(what, got, ref, dt, stores=1):
    if dt == BF:
        P.close(what, got, ref, rel=stores * 2.0 ** -8, why=f"bf16 storage: {stores} stored rounding(s) of 2^-8 between the inputs and this tensor")
    else:
        P.close(what, got, ref)


def _rounded_seams(a):
    at = MC.ROUNDED_AT_PAIRS if a.get("pairs") else MC.ROUNDED_AT
    if a["seams"] is not S512 and a["seams"] is not S768 and not a.get("pairs"):     # the odd-tile arms: 1, cap + 1, 2 cap + 1 tiles
        at = ("v4", "cap+1", "2cap+1")
    return [s for s in a["seams"] if s[0] in at]


@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("arm,products", [p for p in arm_products() if p.values[0] in FWD_ARMS])
def test_rounded_forward(arm, products, dtype):
    a, dt = ARMS[arm], MC.DTYPES[dtype]
    pre = a["run"] == "pre"
    worst = {}
    for seam in _rounded_seams(a):
        B, V, nt = check_seam(arm, products, seam)
        for fam in MC.FAMILIES:
            p = MC.rounded_chain(fam, B, a["C"], a["H"], V, dt, pre=pre, head=a.get("head", 0), head_bias=a.get("head_bias", True), device=DEV)
            with _native.use_products(products):
                o = run_fwd(a, p)
                if fam == "randn":
                    assert same({k: v for k, v in o.items() if v is not None}, {k: v for k, v in run_fwd(a, p).items() if v is not None})
            ref = MC.fwd64(p, x1_stored=o.get("x1"), x2_stored=o["x2"] if "wh" in p else None)
            xin = o["x1"] if pre else p["x"]
            if pre:
                ref["x1"] = MC.fwd64(p)["x1"]
            d = MC.fwd_bounds(p, xin, ref, dt, a["mode"])
            got = {"x1": o.get("x1"), "mu": o["st"][:, 0], "rs": o["st"][:, 1], "z1": o["z1"], "x2": o["x2"], "logits": o.get("logits")}
            fr = {k: LC.fraction(v, ref[k], d[k]) for k, v in got.items() if v is not None}
            print(arm, seam[0], fam, "fraction of the bound:", fr)
            for k, v in fr.items():
                worst[(fam, k)] = max(worst.get((fam, k), 0.0), v)
            bad = {k: v for k, v in fr.items() if v > 1}
            assert not bad, f"{seam[0]} {fam}: {bad} of the bound"
            # mean_1000: an fp32 mean of C numbers near 1000 errs by up to C u 1000 = 2e-3 of the unit spread before any other
            # arithmetic (the emulation of mlp_cases reaches 1.2e-4 of max|z1|): 1e-4 of a max norm is below what fp32
            # statistics resolve there, and the element-wise bound above is the check
            for k in ("x1", "z1", "x2", "logits"):
                if got[k] is not None and fam != "mean_1000":
                    _close(f"{arm} {PNAME[products]} {dtype} {seam[0]} {fam} {k}", got[k], ref[k], dt)
    for fam in MC.FAMILIES:
        P.note(f"mlp chain {arm} {PNAME[products]} {dtype} {fam}: worst fraction of the bound", **{k: v for (f, k), v in worst.items() if f == fam})


@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("arm,products", [p for p in arm_products() if p.values[0] in BWD_ARMS])
def test_rounded_backward(arm, products, dtype):
    a, dt, lib = ARMS[arm], MC.DTYPES[dtype], _native.lib()
    worst = {}
    for seam in _rounded_seams(a):
        B, V, nt = check_seam(arm, products, seam)
        depth = MC.depth_rows(nt) if a["run"] == "bwd" else MC.depth_carried(nt, lib.fz_mlp_wgrad_rows(B, V))
        for fam in MC.FAMILIES:
            p = MC.rounded_chain(fam, B, a["C"], a["H"], V, dt, device=DEV)
            with _native.use_products(products):
                x2, z1, st = PW._mlp_fwd_chain(p["x"], p["g"], p["b"], MC.EPS, p["w1"], p["b1"], p["w2"], p["b2"])
                args = (p["g2"], z1, p["x"], st, p["g"], p["b"], p["w1"], p["w2"])      # the stored z1 and statistics: inputs
                got = run_bwd(a["run"], args)
            sums = a.get("sums", "fp32")
            dn_rel, gadd_rel = MC.two_level_rel(sums, dt)
            d, ref = MC.bwd_bounds(*args, dt, a["mode"], sums, depth, gz1_stored=a["run"] == "bwd", dn_rel=dn_rel, gadd_rel=gadd_rel)
            fr = {k: LC.fraction(got[k], ref[k], d[k]) for k in BKEYS[a["run"]]}
            print(arm, seam[0], fam, "fraction of the bound:", fr)
            for k, v in fr.items():
                worst[(fam, k)] = max(worst.get((fam, k), 0.0), v)
            bad = {k: v for k, v in fr.items() if v > 1}
            assert not bad, f"{seam[0]} {fam}: {bad} of the bound"
            for k in BKEYS[a["run"]]:
                _close(f"{arm} {PNAME[products]} {dtype} {seam[0]} {fam} {k}", got[k], ref[k], dt if k in ("gz1", "gx1") else torch.float32)
    for fam in MC.FAMILIES:
        P.note(f"mlp chain {arm} {PNAME[products]} {dtype} {fam}: worst fraction of the bound", **{k: v for (f, k), v in worst.items() if f == fam})


@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("form", ["out_proj_bias", "in_proj_ln_gadd"])
def test_rounded_gemm_dw(form, dtype):
    lib, dt, ln = _native.lib(), MC.DTYPES[dtype], form == "in_proj_ln_gadd"
    cap = MC.cap_of_rows(lib.fz_gemm_dw_rows)
    worst = {}
    for name, B, V, nt in [s for s in MC.seam_bv(cap) if s[0] in MC.ROUNDED_AT]:
        rows = lib.fz_gemm_dw_rows(B, V)
        assert MC.tiles(lib, B, V) == nt and rows == min(nt, cap) and PW._dw_fused_ok(32, V)
        for fam in MC.FAMILIES:
            gr, w, q, g, b, st, gadd = MC.rounded_dw(fam, B, V, dt, ln, device=DEV)
            n0 = _native.launch_count()
            y, gw, gb, gg, gbt = PW._gemm_dw(gr, w, q, ln=(g, b), stats=st, gadd=gadd) if ln else PW._gemm_dw(gr, w, q, want_bias=True)
            launched(n0)
            d, ref = MC.dw_bounds(gr, w, q, (g, b) if ln else None, st, gadd, dt, MC.depth_carried(nt, rows))
            got = {"y": y, "gw": gw, "gb": gb, "gg": gg, "gbt": gbt}
            fr = {k: LC.fraction(v, ref[k], d[k]) for k, v in got.items() if v is not None}
            print(form, name, fam, "fraction of the bound:", fr)
            for k, v in fr.items():
                worst[(fam, k)] = max(worst.get((fam, k), 0.0), v)
            bad = {k: v for k, v in fr.items() if v > 1}
            assert not bad, f"{name} {fam}: {bad} of the bound"
            for k, v in got.items():
                if v is not None:
                    _close(f"gemm_dw {form} {dtype} {name} {fam} {k}", v, ref[k], dt if k == "y" else torch.float32)
    for fam in MC.FAMILIES:
        P.note(f"gemm_dw {form} {dtype} {fam}: worst fraction of the bound", **{k: v for (f, k), v in worst.items() if f == fam})


# ------------------------------------------------------------------ (c) one launch against two ----------------------------
@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("arm", ["chain32_fwd_split_h64_pre", "chain64_p512_fwd_pre"])
def test_one_launch_against_two(arm, dtype):
    """the out-projection inside the chain launch against act_linear_res followed by the chain: each x1 inside its bound around
    the float64 x1 (so the two within the sum of the bounds), and each chain inside its bounds around the oracle of its own stored x1"""
    a, dt = ARMS[arm], MC.DTYPES[dtype]
    seam = [s for s in a["seams"] if s[0] in ("cap+1", "cap+1_pairs")][0]
    B, V, nt = check_seam(arm, SPLIT, seam)
    C = a["C"]
    for fam in ("randn", "mean_30_std_half", "same_sign"):
        p = MC.rounded_chain(fam, B, C, a["H"], V, dt, pre=True, device=DEV)
        with _native.use_products(SPLIT):
            one = run_fwd(a, p)
            x1b = torch.empty_like(p["a"])
            PW._gemm([p["a"]], p["wo"], x1b, B=B, Cin=C, Vin=V, M=C, K=C, Ncol=V, bias=p["bo"], res=p["x"], name="act_linear_res")
            two = dict(zip(("x2", "z1", "st"), PW._mlp_fwd_chain(x1b, p["g"], p["b"], MC.EPS, p["w1"], p["b1"], p["w2"], p["b2"])))
        two["x1"] = x1b
        x1_64 = MC.fwd64(p)["x1"]
        for o in (one, two):
            ref = MC.fwd64(p, x1_stored=o["x1"])
            ref["x1"] = x1_64
            d = MC.fwd_bounds(p, o["x1"], ref, dt, "three")
            got = {"x1": o["x1"], "mu": o["st"][:, 0], "rs": o["st"][:, 1], "z1": o["z1"], "x2": o["x2"]}
            fr = {k: LC.fraction(v, ref[k], d[k]) for k, v in got.items()}
            assert all(v <= 1 for v in fr.values()), (fam, fr)
        assert LC.fraction(one["x1"], two["x1"].double(), 2 * d["x1"]) <= 1
