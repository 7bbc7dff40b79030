"""-m gpu: the native group norm with its fused activation (csrc/gnorm.hip through ft.group_norm / ft.GroupNorm) against
F.group_norm + activation and its autograd in float64 on the CPU, on the inputs the kernel sees, at the bounds of
tests/gnorm_cases.py; the launch counts; the exact properties (a constant group, repeats, independence of the batch and of the
address); the composed device branches."""
import importlib
import warnings

import pytest
import torch
import torch.nn.functional as F
from torch import nn

import factorizer_amd as ft
import gnorm_cases as GC
import parity as P
from factorizer_amd import _native, composed

GN = importlib.import_module("factorizer_amd.group_norm")

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def seam_sizes():
    L = _native.lib()
    return GC.seams(L.fz_gnorm_one_pass_max(), L.fz_gnorm_chunks)


def run(x, G, w, b, gy, act, slope=GC.SLOPE):
    """forward and backward on the device through the public function; asserts the launches"""
    xd = GC.to_device(x, DEV).requires_grad_(True)
    wd, bd = (None if p is None else p.to(DEV).requires_grad_(True) for p in (w, b))
    cg, V = x.shape[1] // G, x[0, 0].numel()
    L = _native.lib()
    n0 = _native.launch_count()
    with warnings.catch_warnings():
        warnings.simplefilter("error", RuntimeWarning)
        y = ft.group_norm(xd, G, wd, bd, GC.EPS, act, slope)
        assert _native.launch_count() - n0 == L.fz_gnorm_launches(cg, V, 0, 0)
        grads = torch.autograd.grad(y, [xd] + [p for p in (wd, bd) if p is not None], gy.to(DEV))
    assert _native.launch_count() - n0 == L.fz_gnorm_launches(cg, V, 0, 0) + L.fz_gnorm_launches(cg, V, 1, int(w is not None))
    assert y.dtype == x.dtype and grads[0].dtype == x.dtype and y.is_contiguous()
    out = {"y": y.detach(), "gx": grads[0]}
    if w is not None:
        assert grads[1].dtype == grads[2].dtype == torch.float32
        out.update(gw=grads[1], gb=grads[2])
    return out, xd


@pytest.mark.parametrize("act", GC.ACTS, ids=GC.ACT_IDS)
@pytest.mark.parametrize("affine", [False, True], ids=["plain", "affine"])
@pytest.mark.parametrize("dtype", sorted(GC.DTYPES))
@pytest.mark.parametrize("name", GC.CASES)
def test_against_float64(seam_sizes, name, dtype, affine, act):
    dt = GC.DTYPES[dtype]
    x, G, w, b, gy = GC.make(name, dt, affine, seam_sizes)
    got, xd = run(x, G, w, b, gy, act)
    if name == "storage_offset_odd_v":
        assert xd.is_contiguous() and xd.data_ptr() % 16 != 0
    if name == "permuted":
        assert not xd.is_contiguous()
    GC.check(got, GC.reference(x, G, w, b, gy, act), dt,
             note=lambda r: P.note(f"group norm {name} {dtype} {'affine' if affine else 'plain'} {act}: fraction of the bound", **r))


@pytest.mark.parametrize("dtype", sorted(GC.DTYPES))
def test_explicit_negative_slope(dtype):
    dt = GC.DTYPES[dtype]
    x, G, w, b, gy = GC.make("cg3_odd_v", dt, True, None)
    got, _ = run(x, G, w, b, gy, "leaky_relu", 0.2)
    GC.check(got, GC.reference(x, G, w, b, gy, "leaky_relu", 0.2), dt)


@pytest.mark.parametrize("act", GC.ACTS, ids=GC.ACT_IDS)
@pytest.mark.parametrize("dtype", sorted(GC.DTYPES))
def test_exact_properties(dtype, act):
    dt = GC.DTYPES[dtype]
    # a constant group at 1e6: y == act(β) exactly, a finite gx within the bound
    x = torch.full((2, 6, 1367), 1e6).to(dt)
    gy = GC._randn(x.shape, 31).to(dt)
    g = torch.Generator().manual_seed(7)
    w, b = 1 + 0.5 * torch.randn(6, generator=g), torch.randn(6, generator=g)
    got, _ = run(x, 2, w, b, gy, act)
    assert torch.equal(got["y"].cpu(), GC.activation(b.double(), act).to(dt).view(1, 6, 1).expand_as(x))
    r = GC.ratio_elementwise(got["gx"], GC.reference(x, 2, w, b, gy, act, constant=True)["gx"], dt)
    P.note(f"group norm constant group {dtype} {act}: gx fraction of the bound", gx=r)
    assert r <= 1.0
    for name in ("cg3_odd_v", "odd_v_two_launch"):                    # the one-launch and the two-launch path
        x, G, w, b, gy = GC.make(name, dt, True, None)
        one, _ = run(x, G, w, b, gy, act)
        two, _ = run(x, G, w, b, gy, act)
        assert all(torch.equal(one[k], two[k]) for k in ("y", "gx", "gw", "gb")), name
        # x[1:2] alone (a tensor of its own, at another address) gives the bits it gives in the batch
        part, _ = run(x[1:2].clone(), G, w, b, gy[1:2].clone(), act)
        assert torch.equal(one["y"][1:2], part["y"]) and torch.equal(one["gx"][1:2], part["gx"]), name
        # one element off the alignment: the bits of the aligned tensor
        flat = torch.zeros(1 + x.numel(), dtype=dt)
        flat[1:] = x.reshape(-1)
        off, xo = run(flat[1:].view(x.shape), G, w, b, gy, act)
        assert xo.data_ptr() % 16 != 0
        assert all(torch.equal(one[k], off[k]) for k in ("y", "gx", "gw", "gb")), name


def test_module_and_unbatched_shapes():
    torch.manual_seed(1)
    m = ft.GroupNorm(8, 32).to(DEV)
    x = torch.randn(2, 32, 5, 6, 7, device=DEV)
    n0 = _native.launch_count()
    y = m(x)
    assert _native.launch_count() - n0 == 1
    ref = F.group_norm(x.double().cpu(), 8, m.weight.detach().double().cpu(), m.bias.detach().double().cpu(), m.eps)
    assert GC.ratio_elementwise(y.detach(), ref, torch.float32) <= 1.0
    with pytest.raises(RuntimeError):
        ft.group_norm(x, 5)                                           # what the framework raises


# ------------------------------------------------------------------ composed branches -------------------------------------
@pytest.mark.parametrize("case", ["fp16", "fp64", "bf16_params"])
def test_composed_branches_warn_once_and_equal_the_framework(case):
    torch.manual_seed(2)
    mine, theirs = ft.GroupNorm(4, 8).to(DEV), nn.GroupNorm(4, 8).to(DEV)
    x = torch.randn(2, 8, 5, 6, 7, device=DEV)
    if case == "fp16":
        x, mine, theirs = x.half(), mine.half(), theirs.half()
    elif case == "fp64":
        x, mine, theirs = x.double(), mine.double(), theirs.double()
    else:
        x, mine, theirs = x.bfloat16(), mine.bfloat16(), theirs.bfloat16()
    composed._warned.clear()
    n0 = _native.launch_count()
    with pytest.warns(RuntimeWarning, match="outside the native kernel set"):
        y = mine(x)
    with warnings.catch_warnings():
        warnings.simplefilter("error", RuntimeWarning)               # once
        y2 = mine.forward_act(x, "leaky_relu", 0.1)
    assert _native.launch_count() == n0
    assert torch.equal(y, theirs(x)) and torch.equal(y2, F.leaky_relu(theirs(x), 0.1))
