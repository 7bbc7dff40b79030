"""-m gpu: every path of csrc/wgrad.hip (wgrad_kernel, wgrad_fast_kernel, wgrad_fast_group_kernel) and of the FK_WGRAD finish
jobs of csrc/finish.h against the float64 oracle of tests/wgrad_cases.py, evaluated on the device, through pointwise._wgrad /
_wgrad_group.  Exact sweeps: small-integer inputs whose only correct fp32 answer is the float64 one, asserted bit for bit in
fp32 storage on the fp32 MFMAs, in fp32 storage as six split-bf16 products, and in bf16 storage (a dropped tail tile, a tile
counted twice at a chunk boundary, a tap read across a padded face, another sample's statistics, a lost β·gb all change bits).
Rounded sweeps: element-wise under the a-priori bounds of wgrad_cases, the achieved fraction of the bound recorded.  The case
names say which seam a case sits on; tests/test_wgrad_cpu.py holds the table to the library's own chunk counts."""
import pytest
import torch

import parity as P
import wgrad_cases as W
from factorizer_amd import _native
from factorizer_amd import pointwise as PW

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
PRODUCTS = {"fp32": _native.PRODUCTS_FP32_MFMA, "three": _native.PRODUCTS_SPLIT_BF16, "bf16": _native.PRODUCTS_DEFAULT}
_REFS, _INPUTS = {}, {}


def exact_inputs(c, mode):
    """the exact inputs of a case in the mode's storage type, made once (no launch writes them; 0.4 GB over the whole table)"""
    key = (c.name, W.MODES[mode][0])
    if key not in _INPUTS:
        _INPUTS[key] = W.exact(c, key[1], DEV)
    return _INPUTS[key]


def exact_ref(c):
    """the float64 reference of an exact case (the same values in both storage types), computed once on the device"""
    if c.name not in _REFS:
        _REFS[c.name] = W.ref64(c, exact_inputs(c, "fp32_mfma"))
    return _REFS[c.name]


def launch(c, t, mode):
    """fz_wgrad of one case: (gw, gbias or None)"""
    gw, gb = W.outputs(c, t, DEV)
    n0 = _native.launch_count()
    with _native.use_products(PRODUCTS[W.MODES[mode][1]]):
        PW._wgrad(t["p"], t["q"], gw, **W.launch_kwargs(c, t, gw, gb))
    assert _native.launch_count() > n0
    return gw, gb


def launch_group(members, ts, mode):
    outs = [W.outputs(c, t, DEV) for c, t in zip(members, ts)]
    problems = [(t["p"], t["q"], gw, W.launch_kwargs(c, t, gw, gb)) for c, t, (gw, gb) in zip(members, ts, outs)]
    n0 = _native.launch_count()
    with _native.use_products(PRODUCTS[W.MODES[mode][1]]):
        PW._wgrad_group(problems, "wgrad_group_test")
    assert _native.launch_count() > n0
    return outs


def assert_exact(c, ref, gw, gb):
    assert gw.dtype == torch.float32 and torch.equal(gw.double(), ref["gw"]), \
        f"{c.name} gw: {int((gw.double() != ref['gw']).sum())} of {gw.numel()} elements differ"
    if c.gbias:
        assert torch.equal(gb.double(), ref["gb"]), f"{c.name} gbias: {int((gb.double() != ref['gb']).sum())} elements differ"


# ------------------------------------------------------------------ exact -------------------------------------------------
@pytest.mark.parametrize("mode", list(W.MODES))
@pytest.mark.parametrize("c", W.CASES, ids=repr)
def test_exact_single(c, mode):
    t = exact_inputs(c, mode)
    gw, gb = launch(c, t, mode)
    assert_exact(c, exact_ref(c), gw, gb)


@pytest.mark.parametrize("mode", list(W.MODES))
@pytest.mark.parametrize("name", W.GROUP_NAMES)
def test_exact_group(name, mode):
    """fz_wgrad_group against float64, member by member; an empty member's outputs stay as they were"""
    members = dict(W.GROUPS)[name]
    ts = [exact_inputs(c, mode) for c in members]
    outs = launch_group(members, ts, mode)
    for c, (gw, gb) in zip(members, outs):
        if c.B == 0:
            assert torch.isnan(gw).all() and torch.isnan(gb).all()
        else:
            assert_exact(c, exact_ref(c), gw, gb)


@pytest.mark.parametrize("mode", list(W.MODES))
def test_exact_cases_replay_bit_identically(mode):
    for c in W.CASES:
        t = exact_inputs(c, mode)
        a, b = launch(c, t, mode), launch(c, t, mode)
        assert torch.equal(a[0], b[0]) and (a[1] is None or torch.equal(a[1], b[1])), c.name
    for name, members in W.GROUPS:
        ts = [exact_inputs(c, mode) for c in members]
        a, b = launch_group(members, ts, mode), launch_group(members, ts, mode)
        for c, x, y in zip(members, a, b):
            if c.B > 0:
                assert torch.equal(x[0], y[0]) and (x[1] is None or torch.equal(x[1], y[1])), c.name


# ------------------------------------------------------------------ rounded -----------------------------------------------
def check_rounded(c, t, mode, gw, gb, family):
    dtype, prod = W.MODES[mode]
    bd, ref = W.bounds(c, t, prod, dtype)
    f = {"gw": W.fraction(gw, ref["gw"], bd["gw"])}
    if c.gbias:
        f["gb"] = W.fraction(gb, ref["gb"], bd["gb"])
    kernel, blk, wide, nchunk, tpc = W.plan(c)
    P.note("wgrad_rounded", case=c.name, family=family, mode=mode, path=f"{kernel} {c.loader} {blk} finish{wide}", nchunk=nchunk,
           tiles_per_chunk=tpc, **{f"frac_{k}": v for k, v in f.items()})
    print(f"{c.name} {family} {mode}: " + ", ".join(f"{k} {v:.3f} of the bound" for k, v in f.items()))
    for k, v in f.items():
        assert v <= 1, f"{c.name} {family} {mode}: {k} at {v:.3f} of its bound"


@pytest.mark.parametrize("mode", list(W.MODES))
@pytest.mark.parametrize("family", W.FAMILIES)
@pytest.mark.parametrize("name", W.ROUNDED_AT)
def test_rounded_single(name, family, mode):
    c = W.BY_NAME[name]
    t = W.rounded(c, family, W.MODES[mode][0], DEV)
    gw, gb = launch(c, t, mode)
    check_rounded(c, t, mode, gw, gb, family)


@pytest.mark.parametrize("mode", list(W.MODES))
@pytest.mark.parametrize("family", W.FAMILIES)
def test_rounded_group(family, mode):
    members = dict(W.GROUPS)["grp4"]
    ts = [W.rounded(c, family, W.MODES[mode][0], DEV) for c in members]
    for c, t, (gw, gb) in zip(members, ts, launch_group(members, ts, mode)):
        check_rounded(c, t, mode, gw, gb, family)
