"""CPU checks of the native group norm (factorizer_amd/group_norm.py, csrc/gnorm.hip, csrc/gnorm_core.h): the host emulation
tests/emul/emul_gnorm.cpp — the kernels' own visiting order, channel arithmetic, reductions and formulas — against float64 at the
bounds of tests/gnorm_cases.py; the host-side argument checks of the entry points; the module on CPU tensors."""
import ctypes
import importlib
import os
import subprocess
import warnings

import pytest
import torch
import torch.nn.functional as F
from torch import nn

import factorizer_amd as ft
import gnorm_cases as GC

GN = importlib.import_module("factorizer_amd.group_norm")

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "emul", "emul_gnorm.cpp")
LIB = os.path.join(HERE, "emul", "_fz_emul_gnorm.so")
CORES = [os.path.join(os.path.dirname(HERE), "factorizer_amd", "csrc", f) for f in ("gnorm_core.h", "inorm_core.h")]
_vp, _i, _i64, _d = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_double


@pytest.fixture(scope="module")
def emu():
    if not os.path.exists(LIB) or os.path.getmtime(LIB) < max(os.path.getmtime(f) for f in [SRC] + CORES):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-o", LIB, SRC])
    lib = ctypes.CDLL(LIB)
    lib.emu_gnorm_chunks.argtypes = [_i, _i64]
    lib.emu_gnorm_fwd.argtypes = [_vp] * 5 + [_i64, _i, _i, _i64, _d, _i, _d, _i]
    lib.emu_gnorm_bwd.argtypes = [_vp] * 8 + [_i64, _i, _i, _i64, _i, _d, _i]
    lib.emu_gnorm_fwd.restype = lib.emu_gnorm_bwd.restype = None
    return lib


@pytest.fixture(scope="module")
def seam_sizes(emu):
    return GC.seams(emu.emu_gnorm_one_pass_max(), emu.emu_gnorm_chunks)


def _bits(t):
    t = t.contiguous()
    return t.view(torch.int16) if t.dtype == torch.bfloat16 else t


def emu_run(emu, x, G, w, b, gy, act, slope=GC.SLOPE):
    x = x.contiguous()
    B, C = x.shape[0], x.shape[1]
    V = x.numel() // (B * C)
    dt = int(x.dtype == torch.bfloat16)
    xb, gb_ = _bits(x), _bits(gy)
    y, gx = torch.empty_like(xb), torch.empty_like(xb)
    stats = torch.empty(B * G, 2, dtype=torch.float64)
    p = lambda t: None if t is None else t.data_ptr()  # noqa: E731
    a = GN.ACTS[act]
    emu.emu_gnorm_fwd(p(xb), p(w), p(b), p(y), p(stats), B, C, G, V, GC.EPS, a, slope, dt)
    gw = torch.empty(C) if w is not None else None
    gb = torch.empty(C) if b is not None else None
    emu.emu_gnorm_bwd(p(xb), p(gb_), p(w), p(b), p(stats), p(gx), p(gw), p(gb), B, C, G, V, a, slope, dt)
    out = {"y": y.view(x.dtype).view(x.shape), "gx": gx.view(x.dtype).view(x.shape), "stats": stats}
    if w is not None:
        out.update(gw=gw, gb=gb)
    return out


# ---------------------------------------------------------------- the emulation against float64 ---------------------------
@pytest.mark.parametrize("act", GC.ACTS, ids=GC.ACT_IDS)
@pytest.mark.parametrize("affine", [False, True], ids=["plain", "affine"])
@pytest.mark.parametrize("dtype", sorted(GC.DTYPES))
@pytest.mark.parametrize("name", GC.CASES)
def test_emulation_against_float64(emu, seam_sizes, name, dtype, affine, act):
    dt = GC.DTYPES[dtype]
    x, G, w, b, gy = GC.make(name, dt, affine, seam_sizes)
    GC.check(emu_run(emu, x, G, w, b, gy, act), GC.reference(x, G, w, b, gy, act), dt)


def test_the_seams_lie_on_both_sides(emu, seam_sizes):
    opm = emu.emu_gnorm_one_pass_max()
    for c in (1, 8):
        cg, V = seam_sizes[f"one_pass_max_cg{c}"]
        assert cg * V == opm
        assert seam_sizes[f"one_pass_max-1_cg{c}"][0] * seam_sizes[f"one_pass_max-1_cg{c}"][1] < opm
        assert seam_sizes[f"one_pass_max+1_cg{c}"][0] * seam_sizes[f"one_pass_max+1_cg{c}"][1] > opm


@pytest.mark.parametrize("dtype", sorted(GC.DTYPES))
def test_explicit_negative_slope(emu, dtype):
    dt = GC.DTYPES[dtype]
    x, G, w, b, gy = GC.make("cg3_odd_v", dt, True, None)
    GC.check(emu_run(emu, x, G, w, b, gy, "leaky_relu", 0.2), GC.reference(x, G, w, b, gy, "leaky_relu", 0.2), dt)


@pytest.mark.parametrize("act", GC.ACTS, ids=GC.ACT_IDS)
@pytest.mark.parametrize("dtype", sorted(GC.DTYPES))
def test_emulation_exact_properties(emu, dtype, act):
    dt = GC.DTYPES[dtype]
    # a constant group at 1e6: exactly zero variance, z == β exactly, y == act(β) exactly, a finite gx within the bound
    x = torch.full((2, 6, 1367), 1e6).to(dt)
    gy = GC._randn(x.shape, 31).to(dt)
    g = torch.Generator().manual_seed(7)
    w, b = 1 + 0.5 * torch.randn(6, generator=g), torch.randn(6, generator=g)
    got = emu_run(emu, x, 2, w, b, gy, act)
    want = GC.activation(b.double(), act).to(dt).view(1, 6, 1).expand_as(x)
    assert torch.equal(got["y"], want)
    assert torch.equal(got["stats"][:, 0], torch.full((4,), float(x[0, 0, 0]), dtype=torch.float64))
    ref = GC.reference(x, 2, w, b, gy, act, constant=True)
    assert GC.ratio_elementwise(got["gx"], ref["gx"], dt) <= 1.0
    got0 = emu_run(emu, x, 2, None, None, gy, act)
    assert torch.count_nonzero(got0["y"]) == 0 and torch.isfinite(got0["gx"].float()).all()
    # x[1:2] run alone equals that sample of the batched run bit for bit — on the one-launch and the two-launch path
    for name in ("cg3_odd_v", "odd_v_two_launch"):
        x, G, w, b, gy = GC.make(name, dt, True, None)
        whole = emu_run(emu, x, G, w, b, gy, act)
        part = emu_run(emu, x[1:2].clone(), G, w, b, gy[1:2].clone(), act)
        assert torch.equal(whole["y"][1:2], part["y"]) and torch.equal(whole["gx"][1:2], part["gx"])


# ---------------------------------------------------------------- plan and entry points -----------------------------------
@pytest.fixture(scope="module")
def native():
    from factorizer_amd import _native, build
    build.build(verbose=False)
    return _native.lib()


def test_plan_answers(emu, native, seam_sizes):
    opm = native.fz_gnorm_one_pass_max()
    assert opm == emu.emu_gnorm_one_pass_max() and opm >= 4096
    for cg, V in list(seam_sizes.values()) + [(3, 777), (64, 8), (4, 128 ** 3)]:
        assert native.fz_gnorm_chunks(cg, V) == emu.emu_gnorm_chunks(cg, V)
    # both sides of the one-pass seam, with and without parameter gradients
    for cg in (1, 8):
        V = opm // cg
        assert [native.fz_gnorm_launches(cg, V, bw, af) for bw in (0, 1) for af in (0, 1)] == [1, 1, 1, 2]
        assert [native.fz_gnorm_launches(cg, V + 1, bw, af) for bw in (0, 1) for af in (0, 1)] == [2, 2, 2, 3]
    assert GN.launches(8, opm // 8) == 1 and GN.launches(8, opm // 8 + 1, backward=True, affine=True) == 3
    assert native.fz_gnorm_chunks(0, 5) == -1 and native.fz_gnorm_chunks(2, 0) == -1 and native.fz_gnorm_launches(0, 5, 0, 0) == -1
    sizes = [native.fz_gnorm_workspace_bytes(B, 32, 8, 70001) for B in range(1, 9)]
    assert all(b > a > 0 for a, b in zip(sizes, sizes[1:]))                      # monotone in B
    assert native.fz_gnorm_workspace_bytes(2, 32, 8, 100) == (2 * 32 + 2 * 32) * 16
    assert native.fz_gnorm_workspace_bytes(0, 32, 8, 16) == -1 and native.fz_gnorm_workspace_bytes(2, 30, 8, 16) == -1
    assert native.fz_gnorm_workspace_bytes(2, 32, 8, 1 << 31) == -1


def test_host_side_argument_checks(native):
    p8 = ctypes.c_void_p(8)     # a non-null pointer value the host code never dereferences
    err = native.fz_last_error_string
    fwd = lambda *, x=p8, B=2, C=32, G=8, V=16, act=2, dt=0: native.fz_gnorm_fwd(  # noqa: E731
        x, None, None, p8, p8, B, C, G, V, 1e-5, act, 0.01, dt, p8, None)
    bwd = lambda *, gy=p8, B=2, C=32, G=8, V=16, act=2, dt=0, gw=None, w=None: native.fz_gnorm_bwd(  # noqa: E731
        p8, gy, w, None, p8, p8, gw, None, B, C, G, V, act, 0.01, dt, p8, None)
    for f in (fwd, bwd):
        assert f(V=0) == -4 and b"V" in err()
        assert f(B=0) == -4
        assert f(dt=7) == -2 and b"act_dtype" in err()
        assert f(act=3) == -2 and b"activation" in err()
        assert f(act=-1) == -2
        assert f(C=30) == -1 and b"multiple of G" in err()
        assert f(G=0) == -1
        assert f(C=8, G=1, V=1 << 28) == -1 and b"2^31" in err()             # a span of 2^31 elements
        assert f(B=1 << 24, C=1, G=1) == -1 and b"2^24" in err()
    assert fwd(x=None) == -4 and b"null" in err()
    assert bwd(gy=None) == -4 and b"null" in err()
    assert bwd(gw=p8) == -4 and b"parameter" in err()                            # dγ without γ


# ---------------------------------------------------------------- the module on the CPU -----------------------------------
def test_constructor_state_dict_and_isinstance_match_the_parent():
    a, b = ft.GroupNorm(8, 32), nn.GroupNorm(8, 32)
    assert isinstance(a, nn.GroupNorm)
    for k in ("num_groups", "num_channels", "eps", "affine"):
        assert getattr(a, k) == getattr(b, k)
    assert list(a.state_dict()) == list(b.state_dict()) == ["weight", "bias"]
    with torch.no_grad():
        b.weight.normal_()
        b.bias.normal_()
    a.load_state_dict(b.state_dict())                                            # a framework checkpoint loads
    assert torch.equal(a.weight, b.weight) and torch.equal(a.bias, b.bias)
    b.load_state_dict(a.state_dict())
    assert list(ft.GroupNorm(2, 4, eps=1e-3, affine=False).state_dict()) == []
    with pytest.raises(ValueError):
        ft.GroupNorm(3, 32)                                                      # the parent's divisibility check


@pytest.mark.parametrize("shape", [(2, 8, 9), (2, 8, 5, 6), (2, 8, 3, 4, 5), (3, 8)])
@pytest.mark.parametrize("affine", [False, True])
def test_cpu_tensors_are_bit_identical_to_the_framework(shape, affine):
    torch.manual_seed(3)
    a, b = ft.GroupNorm(4, 8, affine=affine), nn.GroupNorm(4, 8, affine=affine)
    if affine:
        with torch.no_grad():
            a.weight.normal_()
            a.bias.normal_()
        b.load_state_dict(a.state_dict())
    x = torch.randn(*shape)
    with warnings.catch_warnings():
        warnings.simplefilter("error", RuntimeWarning)                          # silent on the CPU
        xa, xb = x.clone().requires_grad_(True), x.clone().requires_grad_(True)
        ya, yb = a(xa), b(xb)
        assert torch.equal(ya, yb)
        ya.square().sum().backward()
        yb.square().sum().backward()
        assert torch.equal(xa.grad, xb.grad)
        if affine:
            assert torch.equal(a.weight.grad, b.weight.grad) and torch.equal(a.bias.grad, b.bias.grad)
        for act, fn in (("relu", F.relu), ("leaky_relu", lambda t: F.leaky_relu(t, 0.2)), (None, lambda t: t)):
            assert torch.equal(ft.group_norm(x, 4, a.weight, a.bias, 1e-3, act, 0.2), fn(F.group_norm(x, 4, a.weight, a.bias, 1e-3)))
            assert torch.equal(a.forward_act(x, act, 0.2), fn(b(x)))
    with pytest.raises(RuntimeError):
        ft.group_norm(x, 3)                                                      # what the framework raises
    with pytest.raises(ValueError):
        ft.group_norm(x, 4, act="gelu")


def test_device_fallback_reasons():
    f32, bf = torch.float32, torch.bfloat16
    for dt in (f32, bf):
        assert GN.fallback_reason(dt) is None and GN.fallback_reason(dt, [f32, f32]) is None
    reasons = {GN.fallback_reason(torch.float16), GN.fallback_reason(torch.float64), GN.fallback_reason(bf, [bf])}
    assert len(reasons) == 3 and None not in reasons                             # one warn_once key each
    assert "float16" in GN.fallback_reason(torch.float16) and "not float32" in GN.fallback_reason(f32, [bf])


def test_convert_keeps_parameters_and_keys_and_is_idempotent():
    torch.manual_seed(5)
    model = nn.Sequential(nn.Conv2d(2, 8, 3), nn.GroupNorm(4, 8), nn.LeakyReLU(),
                          nn.Sequential(nn.GroupNorm(2, 8, eps=1e-3, affine=False), nn.BatchNorm2d(8), nn.InstanceNorm2d(8)))
    model[3].eval()
    with torch.no_grad():
        model[1].weight.normal_()
    before = {k: v.clone() for k, v in model.state_dict().items()}
    kinds = [type(m) for m in model.modules()]
    old = model[1]
    conv = ft.convert_group_norm(model)
    assert conv is model
    assert list(conv.state_dict()) == list(before) and all(torch.equal(conv.state_dict()[k], v) for k, v in before.items())
    assert type(conv[1]) is ft.GroupNorm and conv[1].weight is old.weight and conv[1].bias is old.bias and conv[1].training
    new = conv[3][0]
    assert type(new) is ft.GroupNorm and (new.num_groups, new.num_channels, new.eps, new.affine, new.training) == (2, 8, 1e-3, False, False)
    for m, k in zip(conv.modules(), kinds):
        assert type(m) is k or (k is nn.GroupNorm and type(m) is ft.GroupNorm)
    mods = list(conv.modules())
    again = ft.convert_group_norm(conv)
    assert again is conv and all(a is b for a, b in zip(again.modules(), mods))
    assert type(ft.convert_group_norm(nn.GroupNorm(2, 4))) is ft.GroupNorm
    x = torch.randn(2, 2, 7, 7)
    ref = nn.Sequential(nn.Conv2d(2, 8, 3), nn.GroupNorm(4, 8), nn.LeakyReLU(),
                        nn.Sequential(nn.GroupNorm(2, 8, eps=1e-3, affine=False), nn.BatchNorm2d(8), nn.InstanceNorm2d(8)))
    ref.load_state_dict(conv.state_dict())
    ref[3].eval()
    assert torch.equal(conv(x), ref(x))
