"""CPU checks of the native instance norm (factorizer_amd/instance_norm.py, csrc/inorm.hip, csrc/inorm_core.h): the host
emulation tests/emul/emul_inorm.cpp — the kernels' own chunk plan, visiting order, reductions and formulas — against float64
at the bounds of tests/inorm_cases.py; the host-side argument checks of the entry points; the modules on CPU tensors."""
import ctypes
import importlib
import math
import os
import subprocess
import warnings

import numpy as np
import pytest
import torch
import torch.nn.functional as F
from torch import nn

import factorizer_amd as ft
import inorm_cases as IC

IN = importlib.import_module("factorizer_amd.instance_norm")   # (ft.instance_norm is the function of that name)

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "emul", "emul_inorm.cpp")
LIB = os.path.join(HERE, "emul", "_fz_emul_inorm.so")
CORE = os.path.join(os.path.dirname(HERE), "factorizer_amd", "csrc", "inorm_core.h")
_vp, _i, _i64, _d = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_double


@pytest.fixture(scope="module")
def emu():
    if not os.path.exists(LIB) or os.path.getmtime(LIB) < max(os.path.getmtime(SRC), os.path.getmtime(CORE)):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-o", LIB, SRC])
    lib = ctypes.CDLL(LIB)
    lib.emu_inorm_chunks.argtypes = [_i64]
    lib.emu_inorm_chunk.argtypes = [_i64, _i, ctypes.POINTER(_i64), ctypes.POINTER(_i64)]
    lib.emu_inorm_round_bf16.argtypes = [_d]
    lib.emu_inorm_round_bf16.restype = ctypes.c_uint
    lib.emu_inorm_visits.argtypes = [_i64, _i, _vp]
    lib.emu_inorm_fwd.argtypes = [_vp] * 5 + [_i64, _i, _i64, _d, _i]
    lib.emu_inorm_bwd.argtypes = [_vp] * 7 + [_i64, _i, _i64, _i]
    lib.emu_inorm_fwd.restype = lib.emu_inorm_bwd.restype = lib.emu_inorm_visits.restype = None
    return lib


@pytest.fixture(scope="module")
def seam_sizes(emu):
    return IC.seams(emu.emu_inorm_one_pass_max(), emu.emu_inorm_chunks)


def _bits(t):
    """a contiguous tensor the emulation can address: bf16 as its uint16 bits"""
    t = t.contiguous()
    return t.view(torch.int16) if t.dtype == torch.bfloat16 else t


def emu_run(emu, x, w, b, gy):
    x = x.contiguous()                     # the module makes a permuted input contiguous before the kernels see it
    P, C = x.shape[0] * x.shape[1], x.shape[1]
    V = x.numel() // P
    dt = int(x.dtype == torch.bfloat16)
    xb, gb_ = _bits(x), _bits(gy)
    y, gx = torch.empty_like(xb), torch.empty_like(xb)
    stats = torch.empty(P, 2, dtype=torch.float64)
    p = lambda t: None if t is None else t.data_ptr()
    emu.emu_inorm_fwd(p(xb), p(w), p(b), p(y), p(stats), P, C, V, IC.EPS, dt)
    gw = torch.empty(C) if w is not None else None
    gb = torch.empty(C) if b is not None else None
    emu.emu_inorm_bwd(p(xb), p(gb_), p(w), p(stats), p(gx), p(gw), p(gb), P, C, V, dt)
    out = {"y": y.view(x.dtype).view(x.shape), "gx": gx.view(x.dtype).view(x.shape), "stats": stats}
    if w is not None:
        out.update(gw=gw, gb=gb)
    return out


# ---------------------------------------------------------------- the emulation against float64 ---------------------------
@pytest.mark.parametrize("affine", [False, True], ids=["plain", "affine"])
@pytest.mark.parametrize("dtype", sorted(IC.DTYPES))
@pytest.mark.parametrize("name", IC.CASES)
def test_emulation_against_float64(emu, seam_sizes, name, dtype, affine):
    dt = IC.DTYPES[dtype]
    x, w, b, gy = IC.make(name, dt, affine, seam_sizes)
    IC.check(emu_run(emu, x, w, b, gy), IC.reference(x, w, b, gy), dt)


@pytest.mark.parametrize("dtype", sorted(IC.DTYPES))
def test_emulation_exact_properties(emu, dtype):
    dt = IC.DTYPES[dtype]
    # a constant plane at 1e6: exactly zero variance, y == 0 exactly, a finite gx within the bound
    x = torch.full((2, 3, 4099), 1e6).to(dt)
    gy = IC._randn(x.shape, 31).to(dt)
    got = emu_run(emu, x, None, None, gy)
    assert torch.count_nonzero(got["y"]) == 0
    assert torch.equal(got["stats"][:, 0], x[:, :, 0].reshape(-1).double())
    assert IC.ratio_elementwise(got["gx"], IC.reference(x, None, None, gy)["gx"], dt) <= 1.0
    # the planes of x[1:2] run alone equal those planes of the batched run bit for bit — on the one-launch and two-launch path
    for V in (4099, 70001):
        x, w, b, gy = IC.make("ragged_chunks" if V == 70001 else "tail_odd_planes", dt, True, None)
        whole = emu_run(emu, x, w, b, gy)
        part = emu_run(emu, x[1:2].clone(), w, b, gy[1:2].clone())
        assert torch.equal(whole["y"][1:2], part["y"]) and torch.equal(whole["gx"][1:2], part["gx"])
        again = emu_run(emu, x, w, b, gy)
        assert all(torch.equal(whole[k], again[k]) for k in ("y", "gx", "gw", "gb"))


def _bf16_nearest_even(v):
    """the bf16 nearest to the float64 v (normal range), ties to even, in exact arithmetic"""
    m, e = math.frexp(abs(v))              # |v| = m 2^e, 0.5 <= m < 1
    q = m * 256.0                          # exact: eight significand bits in front of the point
    lo = math.floor(q)
    r = q - lo
    n = lo + (1 if r > 0.5 or (r == 0.5 and lo % 2 == 1) else 0)
    return math.copysign(n * 2.0 ** (e - 8), v)


def test_float64_to_bf16_is_one_rounding(emu):
    """a float64 just above / below the midpoint of two bf16 values rounds to fp32 ON the midpoint: going through a rounded fp32
    would then break the tie the wrong way"""
    rng = np.random.default_rng(0)
    vals = list(rng.standard_normal(2000) * 10.0 ** rng.integers(-3, 4, 2000))
    for k in range(200):
        base = float(torch.tensor(float(rng.uniform(0.5, 300.0))).to(torch.bfloat16))
        half = 2.0 ** (math.frexp(base)[1] - 9)            # half a unit in the last place of base
        for s in (1.0, -1.0):
            for tiny in (0.0, 2.0 ** -45, -(2.0 ** -45)):
                vals.append(s * (base + half) * (1.0 + tiny))
    for v in vals:
        bits = emu.emu_inorm_round_bf16(float(v))
        got = float(torch.tensor([bits], dtype=torch.int32).to(torch.int16).view(torch.bfloat16)[0]) if bits < 0x8000 else \
            float(torch.tensor([bits - 0x10000], dtype=torch.int32).to(torch.int16).view(torch.bfloat16)[0])
        assert got == _bf16_nearest_even(float(v)), v


# ---------------------------------------------------------------- plan and entry points -----------------------------------
@pytest.fixture(scope="module")
def native():
    from factorizer_amd import _native, build
    build.build(verbose=False)
    return _native.lib()


def test_chunk_plan_covers_every_element_once(emu, native, seam_sizes):
    sizes = list(range(1, 5001)) + sorted(set(seam_sizes.values())) + [256 * 16384, 256 * 16384 + 1, 5_000_001]
    for V in sizes:
        n = emu.emu_inorm_chunks(V)
        assert n == native.fz_inorm_chunks(V)
        lo, hi, at = _i64(), _i64(), 0
        for c in range(n):                                   # the chunks tile [0, V) in order, none empty
            emu.emu_inorm_chunk(V, c, ctypes.byref(lo), ctypes.byref(hi))
            assert lo.value == at and hi.value > lo.value
            at = hi.value
        assert at == V
        if V <= 5000 or V in seam_sizes.values():
            for W in (4, 8):                                 # ... and the threads of a workgroup visit each element once
                count = np.zeros(V, np.int32)
                emu.emu_inorm_visits(V, W, count.ctypes.data)
                assert (count == 1).all(), (V, W)
    assert emu.emu_inorm_one_pass_max() == native.fz_inorm_one_pass_max()
    assert native.fz_inorm_chunks(256 * 16384 + 1) <= 256        # the chunk grows, the partials of a plane do not


def test_one_pass_limit_covers_the_deepest_bundle_stages(native):
    assert native.fz_inorm_one_pass_max() >= 4096               # V = 512, 4096 (3-D at roi 128^3), 1024, 4096 (2-D at 512^2)


def test_host_side_argument_checks(native):
    p8 = ctypes.c_void_p(8)     # a non-null pointer value the host code never dereferences
    err = native.fz_last_error_string
    assert native.fz_inorm_fwd(p8, None, None, p8, p8, 6, 3, 0, 1e-5, 0, p8, None) == -4 and b"V" in err()
    assert native.fz_inorm_fwd(p8, None, None, p8, p8, 0, 3, 16, 1e-5, 0, p8, None) == -4 and b"P" in err()
    assert native.fz_inorm_fwd(p8, None, None, p8, p8, 6, 3, 16, 1e-5, 7, p8, None) == -2 and b"act_dtype" in err()
    assert native.fz_inorm_bwd(p8, p8, None, p8, p8, None, None, 6, 3, 0, 0, p8, None) == -4 and b"V" in err()
    assert native.fz_inorm_bwd(p8, p8, None, p8, p8, None, None, -1, 3, 16, 0, p8, None) == -4 and b"P" in err()
    assert native.fz_inorm_bwd(p8, p8, None, p8, p8, None, None, 6, 3, 16, 2, p8, None) == -2 and b"act_dtype" in err()
    assert native.fz_inorm_fwd(p8, None, None, p8, p8, 7, 3, 16, 1e-5, 0, p8, None) == -1        # P is no multiple of C
    assert native.fz_inorm_fwd(None, None, None, p8, p8, 6, 3, 16, 1e-5, 0, p8, None) == -4 and b"null" in err()
    assert native.fz_inorm_workspace_bytes(0, 16) == -1 and native.fz_inorm_workspace_bytes(6, 0) == -1
    assert native.fz_inorm_chunks(0) == -1
    # a 1-D grid of 256-thread workgroups holds fewer than 2^24 of them
    assert native.fz_inorm_workspace_bytes((1 << 24) - 1, 16) > 0 and native.fz_inorm_workspace_bytes(1 << 24, 16) == -1
    assert native.fz_inorm_workspace_bytes(1 << 20, 16 * 16384) == -1
    assert native.fz_inorm_fwd(p8, None, None, p8, p8, 1 << 24, 1, 16, 1e-5, 0, p8, None) == -1 and b"2^24" in err()
    # partials of every chunk, then two totals per plane, float64
    V = 3 * 16384 + 5
    assert native.fz_inorm_workspace_bytes(6, V) == (6 * native.fz_inorm_chunks(V) + 6) * 16
    assert native.fz_inorm_workspace_bytes(6, 100) == 12 * 16


# ---------------------------------------------------------------- the modules on the CPU ----------------------------------
PAIRS = [(ft.InstanceNorm1d, nn.InstanceNorm1d, (2, 4, 9)), (ft.InstanceNorm2d, nn.InstanceNorm2d, (2, 4, 5, 6)),
         (ft.InstanceNorm3d, nn.InstanceNorm3d, (2, 4, 3, 4, 5))]


@pytest.mark.parametrize("mine,theirs,shape", PAIRS)
def test_constructor_state_dict_and_isinstance_match_the_parent(mine, theirs, shape):
    a, b = mine(4), theirs(4)
    assert isinstance(a, theirs)
    for k in ("num_features", "eps", "momentum", "affine", "track_running_stats"):
        assert getattr(a, k) == getattr(b, k)
    assert (a.eps, a.affine, a.track_running_stats) == (1e-5, False, False)
    assert list(a.state_dict()) == list(b.state_dict()) == []
    for kw in (dict(affine=True), dict(track_running_stats=True), dict(affine=True, track_running_stats=True, eps=1e-3, momentum=0.2)):
        a, b = mine(4, **kw), theirs(4, **kw)
        assert list(a.state_dict()) == list(b.state_dict())
        b.load_state_dict(a.state_dict())
        a.load_state_dict(b.state_dict())


@pytest.mark.parametrize("mine,theirs,shape", PAIRS)
@pytest.mark.parametrize("kw", [dict(), dict(affine=True), dict(affine=True, track_running_stats=True)], ids=["plain", "affine", "running"])
def test_cpu_tensors_are_bit_identical_to_the_framework(mine, theirs, shape, kw):
    torch.manual_seed(3)
    a, b = mine(4, **kw), theirs(4, **kw)
    if kw.get("affine"):
        with torch.no_grad():
            a.weight.normal_()
            a.bias.normal_()
        b.load_state_dict(a.state_dict())
    x = torch.randn(*shape)
    with warnings.catch_warnings():
        warnings.simplefilter("error", RuntimeWarning)         # silent on the CPU
        for mode in (True, False):
            a.train(mode)
            b.train(mode)
            xa, xb = x.clone().requires_grad_(True), x.clone().requires_grad_(True)
            ya, yb = a(xa), b(xb)
            assert torch.equal(ya, yb)
            ya.square().sum().backward()
            yb.square().sum().backward()
            assert torch.equal(xa.grad, xb.grad)
            assert torch.equal(a(x[0]), b(x[0]))               # unbatched input
        assert all(torch.equal(u, v) for u, v in zip(a.state_dict().values(), b.state_dict().values()))
        assert torch.equal(ft.instance_norm(x, eps=1e-3), F.instance_norm(x, eps=1e-3))
    with pytest.raises(ValueError):
        a(torch.randn(2, 4, 2, 2, 2, 2, 2))                     # the parent's rank check


def test_gradcheck_float64():
    torch.manual_seed(4)
    x = torch.randn(2, 3, 7, dtype=torch.float64, requires_grad=True)
    w = torch.randn(3, dtype=torch.float64, requires_grad=True)
    b = torch.randn(3, dtype=torch.float64, requires_grad=True)
    assert torch.autograd.gradcheck(lambda x, w, b: ft.instance_norm(x, w, b), (x, w, b))
    m = ft.InstanceNorm1d(3, affine=True).double()
    assert torch.autograd.gradcheck(m, (x,))


def test_one_spatial_element_raises_like_the_framework():
    for m, shape in ((ft.InstanceNorm1d(3), (2, 3, 1)), (ft.InstanceNorm3d(3), (2, 3, 1, 1, 1))):
        with pytest.raises(ValueError, match="more than 1 spatial element"):
            m(torch.randn(*shape))
    with pytest.raises(ValueError, match="more than 1 spatial element"):
        ft.instance_norm(torch.randn(2, 3, 1))


def test_device_fallback_reasons():
    """the pure gate: what a device tensor of this type in a module with these flags would do"""
    f32, bf = torch.float32, torch.bfloat16
    for dt in (f32, bf):
        assert IN.fallback_reason(dt) is None
        assert IN.fallback_reason(dt, training=False, track_running_stats=False) is None       # eval without running statistics
        assert IN.fallback_reason(dt, param_dtypes=[f32, f32]) is None
    assert "float16" in IN.fallback_reason(torch.float16)
    assert "float64" in IN.fallback_reason(torch.float64)
    assert "track_running_stats=True" in IN.fallback_reason(f32, training=True, track_running_stats=True)
    assert "eval mode with running statistics" in IN.fallback_reason(f32, training=False, track_running_stats=True)
    assert "not float32" in IN.fallback_reason(bf, param_dtypes=[bf, bf])
    reasons = {IN.fallback_reason(torch.float16), IN.fallback_reason(torch.float64), IN.fallback_reason(f32, True, True),
               IN.fallback_reason(f32, False, True), IN.fallback_reason(f32, True, False, [bf])}
    assert len(reasons) == 5                                     # one warn_once key each


# ---------------------------------------------------------------- convert_instance_norm -----------------------------------
def test_convert_is_a_round_trip():
    torch.manual_seed(5)
    model = nn.Sequential(nn.Conv2d(2, 4, 3), nn.InstanceNorm2d(4), nn.ReLU(),
                          nn.Sequential(nn.InstanceNorm2d(4, affine=True, track_running_stats=True, eps=1e-3, momentum=0.3),
                                        nn.BatchNorm2d(4), nn.GroupNorm(2, 4)),
                          nn.InstanceNorm1d(4, affine=True), nn.InstanceNorm3d(4))
    model[3].eval()
    with torch.no_grad():
        model[3][0].running_mean.normal_()
        model[4].weight.normal_()
    before = {k: v.clone() for k, v in model.state_dict().items()}
    kinds = [type(m) for m in model.modules()]
    old = model[3][0]
    conv = ft.convert_instance_norm(model)
    assert conv is model                                         # containers are kept, only the norms are new objects
    assert list(conv.state_dict()) == list(before) and all(torch.equal(conv.state_dict()[k], v) for k, v in before.items())
    new = conv[3][0]
    assert type(new) is ft.InstanceNorm2d and new.weight is old.weight and new.running_mean is old.running_mean
    assert (new.eps, new.momentum, new.affine, new.track_running_stats, new.training) == (1e-3, 0.3, True, True, False)
    assert type(conv[1]) is ft.InstanceNorm2d and conv[1].training
    assert type(conv[4]) is ft.InstanceNorm1d and type(conv[5]) is ft.InstanceNorm3d
    for m, k in zip(conv.modules(), kinds):                     # nothing but the InstanceNorm modules was replaced
        assert type(m) is k or (issubclass(type(m), k) and k in (nn.InstanceNorm1d, nn.InstanceNorm2d, nn.InstanceNorm3d))
    mods = list(conv.modules())
    again = ft.convert_instance_norm(conv)                       # idempotent: the same objects
    assert again is conv and all(a is b for a, b in zip(again.modules(), mods))
    assert type(ft.convert_instance_norm(nn.InstanceNorm3d(2))) is ft.InstanceNorm3d     # a bare norm


def _deconver2d(norm):
    torch.manual_seed(0)
    return ft.Deconver(in_channels=2, out_channels=3, spatial_dims=2, encoder_width=(8, 16), encoder_depth=(1, 1), strides=(1, 2),
                       decoder_depth=(1,), act=nn.ReLU, groups=-1, ratio=1, kernel_size=(3, 3), num_iters=2, mlp_ratio=2,
                       dropout=0.0, norm=norm)


def test_deconver_checkpoint_loads_into_the_converted_model_and_back():
    plain = _deconver2d(nn.InstanceNorm2d)
    native_ = ft.convert_instance_norm(_deconver2d(nn.InstanceNorm2d))
    built = _deconver2d(ft.InstanceNorm2d)
    n = sum(isinstance(m, nn.InstanceNorm2d) for m in plain.modules())
    assert n > 0 and sum(type(m) is ft.InstanceNorm2d for m in native_.modules()) == n
    assert sum(type(m) is ft.InstanceNorm2d for m in built.modules()) == n
    assert list(plain.state_dict()) == list(native_.state_dict()) == list(built.state_dict())
    with torch.no_grad():
        for p in plain.parameters():
            p.add_(0.01)
    native_.load_state_dict(plain.state_dict())
    back = _deconver2d(nn.InstanceNorm2d)
    back.load_state_dict(native_.state_dict())
    x = torch.rand(1, 2, 16, 24)
    with torch.no_grad():
        y = plain(x)
        assert torch.equal(native_(x), y) and torch.equal(back(x), y)      # on the CPU all three run the framework's norm
