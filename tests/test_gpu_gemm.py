"""-m gpu: every kernel form fz_gemm's dispatcher can launch (csrc/gemm.hip, gemm_bx.hip, gemm_bxk.hip, gemm_stream.hip,
gemm_p32.hip, the 64-channel LayerNorm-backward chain and the head) against the float64 oracle of tests/gemm_cases.py, evaluated
on the device, through ctypes.  For every case the form fz_gemm_plan reports — the dispatcher's own dry run — must be the one
recorded in the table before fz_gemm runs.  Exact sweeps: small-integer inputs whose only correct answer is the float64 one,
asserted bit for bit in fp32 storage on the fp32 MFMAs, in fp32 storage as six split-bf16 products and in bf16 storage (a
swapped tap, a bias row of the wrong index, a dropped column or row block, a concat split one channel off all change bits),
and every `tune` value gives the bits of `tune = 0`.  Rounded sweeps: element-wise under the a-priori bounds of gemm_cases, the
achieved fraction of the bound recorded.  No descriptor here is one the host code refuses (tests/test_gemm_cpu.py has those)."""
import ctypes

import pytest
import torch

import gemm_cases as G
import parity as P
from factorizer_amd import _native

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
_INPUTS, _REFS = {}, {}
PAIRS = [(c, m) for c in G.CASES for m in c.modes]
_id = lambda v: v if isinstance(v, str) else repr(v)


def exact_inputs(c, dtype):
    key = (c.name, dtype)
    if key not in _INPUTS:
        if G.elements(c) > 1 << 22:          # the few threshold cases: not kept
            return G.exact(c, dtype, DEV)
        _INPUTS[key] = G.exact(c, dtype, DEV)
    return _INPUTS[key]


def exact_ref(c, t):
    """the float64 reference of an exact case (the same values in both storage types), computed once on the device"""
    if G.elements(c) > 1 << 22:
        return G.ref64(c, t)
    if c.name not in _REFS:
        _REFS[c.name] = G.ref64(c, t)
    return _REFS[c.name]


def launch(c, t, mode, tune=None):
    """fz_gemm of one case through ctypes: dict y [, stats, part] after the planned form was held to the table"""
    lib = _native.lib()
    dtype = G.MODES[mode][0]
    out = {"y": torch.full(c.yshape, float("nan"), device=DEV, dtype=dtype)}
    ptrs = {"x0": t["x"][0].data_ptr(), "w": t["w"].data_ptr(), "y": out["y"].data_ptr()}
    if c.nsrc == 2:
        ptrs["x1"] = t["x"][1].data_ptr()
    for k in ("bias", "ln_g", "ln_b", "bmul", "res", "emul", "lnb_x", "lnb_stats", "lnb_g", "lnb_gadd"):
        if k in t:
            ptrs[k] = t[k].data_ptr()
    if c.stats:
        out["stats"] = torch.full((max(c.B, 1), 2, c.N), float("nan"), device=DEV)
        ptrs["stats"] = out["stats"].data_ptr()
    if c.epi == "lnbwd":
        ptrs["lnb_part"] = 8         # (sized below from the descriptor)
    d = G.desc_of(c, mode, ptrs)
    if tune is not None:
        d.tune = tune
    if c.epi == "lnbwd":
        rows = int(lib.fz_gemm_lnbwd_partials(ctypes.byref(d)))
        out["part"] = torch.full((rows, 2 * c.M), float("nan"), device=DEV)
        d.lnb_part = out["part"].data_ptr()
    if tune is None:
        rc, text = G.plan_desc(lib, d)
        assert rc == 0 and text == G.REACHED[(c.name, mode)], (c.name, mode, rc, text, G.REACHED[(c.name, mode)])
        if c.epi == "lnbwd":
            assert G.grid_of(text)[0] == (min(rows, 512) if c.M == 64 else rows)     # one partial row per resident workgroup
    n0 = _native.launch_count()
    with torch.cuda.device(DEV):
        rc = lib.fz_gemm(ctypes.byref(d), _native.stream_ptr(t["w"]))
    assert rc == 0, (c.name, mode, lib.fz_last_error_string())
    assert _native.launch_count() > n0
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:        # a device fault: nothing more is started on the card by this session
        pytest.exit(f"{c.name} {mode} [{G.REACHED[(c.name, mode)]}]: {e}", returncode=3)
    return out


def _same(a, b):
    return torch.equal(a, b) or torch.equal(a.double(), b.double())    # (-0 and +0 compare equal: gelu(-16) = -0)


def assert_exact(c, ref, out, dtype, what=""):
    want = G.stored(c, ref, dtype)
    got = out["y"]
    assert got.dtype == dtype and got.shape == want.shape
    assert torch.equal(got.double(), want.double()), \
        f"{c.name} {what}: {int((got.double() != want.double()).sum())} of {got.numel()} elements differ"
    if c.epi == "lnbwd":
        tot = out["part"].double().sum(0)
        assert torch.equal(tot[:c.M], ref["gg"]) and torch.equal(tot[c.M:], ref["gb"]), c.name


def check_rounded(c, t, mode, out, family):
    dtype = G.MODES[mode][0]
    bd, ref = G.bounds(c, t, mode, dtype)
    f = {"y": G.fraction(out["y"], ref["y"], bd["y"])}      # (against the unrounded reference: the bound holds the half unit of bf16)
    if c.stats:
        f["mu"] = G.fraction(out["stats"][:, 0], ref["mu"], bd["mu"])
        f["rs"] = G.fraction(out["stats"][:, 1], ref["rs"], bd["rs"])
    if c.epi == "lnbwd":
        tot = out["part"].double().sum(0)
        f["gg"], f["gb"] = G.fraction(tot[:c.M], ref["gg"], bd["gg"]), G.fraction(tot[c.M:], ref["gb"], bd["gb"])
    form = G.form_of(G.REACHED[(c.name, mode)])
    P.note("gemm_rounded", case=c.name, family=family, mode=mode, form=form, **{f"frac_{k}": v for k, v in f.items()})
    print(f"{c.name} {family} {mode} [{form}]: " + ", ".join(f"{k} {v:.3f} of the bound" for k, v in f.items()))
    for k, v in f.items():
        assert v <= 1, f"{c.name} {family} {mode} [{form}]: {k} at {v:.3f} of its bound"


# ------------------------------------------------------------------ exact -------------------------------------------------
@pytest.mark.parametrize("c,mode", [(c, m) for c, m in PAIRS if G.has_exact(c)], ids=_id)
def test_exact(c, mode):
    dtype = G.MODES[mode][0]
    t = exact_inputs(c, dtype)
    ref = exact_ref(c, t)
    out = launch(c, t, mode)
    assert_exact(c, ref, out, dtype)
    again = launch(c, t, mode)                       # replay: the same bits
    assert all(_same(out[k], again[k]) for k in out), c.name


@pytest.mark.parametrize("mode", ["fp32_split", "bf16"])
def test_results_do_not_depend_on_tune(mode):
    """the header's claim for `tune`: every value gives the bits of the library's own choice (on exact inputs: the float64 answer)"""
    dtype = G.MODES[mode][0]
    tunes = [0, 300] + [100 + 10 * na + mb for na in (2, 4) for mb in (1, 2)] + [200 + 10 * na + mb for na in (1, 2) for mb in (1, 2)]
    for name in ("bx_plain_mb2_n4", "bx_gelu_mb2_n4", "bx_d2s_mb2_n2", "bx_bmul_mb2", "bx_s2d_mb2", "bx_m96", "bx_c0_48", "bxk_emul_gelu",
                 "bx_k96", "bx_k32_bf16"):         # (the trailing half chunk: K = 96, and K = 32 on bf16 storage)
        c = G.BY_NAME[name]
        if mode not in c.modes:
            continue
        t = exact_inputs(c, dtype)
        ref = exact_ref(c, t)
        for tune in tunes:
            assert_exact(c, ref, launch(c, t, mode, tune=tune), dtype, f"tune {tune}")


# ------------------------------------------------------------------ rounded -----------------------------------------------
ROUNDED = [(G.BY_NAME[n], m) for n in G.ROUNDED_AT for m in G.BY_NAME[n].modes]
ROUNDED += [(c, m) for c, m in PAIRS if not G.has_exact(c) and c.name not in G.ROUNDED_AT]


@pytest.mark.parametrize("c,mode", ROUNDED, ids=_id)
def test_rounded(c, mode):
    dtype = G.MODES[mode][0]
    fams = G.families_of(c) if c.name in G.ROUNDED_AT else ["randn"]
    for family in fams:
        t = G.rounded(c, family, dtype, DEV)
        out = launch(c, t, mode)
        check_rounded(c, t, mode, out, family)
        if family == "randn":
            again = launch(c, t, mode)
            assert all(_same(out[k], again[k]) for k in out), (c.name, "replay")
