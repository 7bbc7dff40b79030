"""CPU checks of the native cd / smu solvers (factorizer_amd/csrc/nmf_core.h, SOLVER_CD = 2, SOLVER_SMU = 3): the wave program
through its host lock-step emulation (tests/emul/emul_solvers.cpp) against the reference's goldens g11 and against the package's
composed path in float64 autograd; the host routing; the C header's ids; the spill audit of the cfg-1-shape backward kernels."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest
import torch
from torch import nn

import factorizer_amd as ft
from factorizer_amd import _native
from factorizer_amd import nmf as nmf_mod

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SRC = os.path.join(HERE, "emul", "emul_solvers.cpp")
LIB = os.path.join(HERE, "emul", "_fz_emul_solvers.so")
CSRC = os.path.join(ROOT, "factorizer_amd", "csrc")
SID = {"cd": 2, "smu": 3}


@pytest.fixture(scope="module")
def emu():
    deps = [SRC, os.path.join(HERE, "emul", "emul.cpp"), os.path.join(CSRC, "nmf_core.h"), os.path.join(CSRC, "nmf_gram.h")]
    if not os.path.exists(LIB) or os.path.getmtime(LIB) < max(os.path.getmtime(d) for d in deps):
        subprocess.check_call(["g++", "-O1", "-std=c++17", "-shared", "-fPIC", "-o", LIB, SRC])
    lib = ctypes.CDLL(LIB)
    fp = ctypes.POINTER(ctypes.c_float)
    lib.emu_solver_fwd.argtypes = [fp] * 6 + [ctypes.c_int64] + [ctypes.c_int] * 5 + [ctypes.c_float]
    lib.emu_solver_bwd.argtypes = [fp] * 7 + [ctypes.c_int64] + [ctypes.c_int] * 6 + [ctypes.c_float]
    return lib


def _p(a):
    return None if a is None else a.ctypes.data_as(ctypes.POINTER(ctypes.c_float))


def _np(t):
    return np.ascontiguousarray(t.detach().float().numpy())


def emu_fwd(lib, x, u0, v0, T, solver):
    M, N = x.shape[-2:]
    R = u0.shape[1]
    xn = _np(x.reshape(-1, M, N))
    nmat = xn.shape[0]
    y, u, v = np.empty_like(xn), np.empty((nmat, M, R), np.float32), np.empty((nmat, N, R), np.float32)
    rc = lib.emu_solver_fwd(_p(xn), _p(_np(u0)), _p(_np(v0)), _p(y), _p(u), _p(v), nmat, M, N, R, T, SID[solver], 1e-16)
    assert rc == 0
    lead = x.shape[:-2]
    return (torch.from_numpy(y).reshape(x.shape), torch.from_numpy(u).reshape(*lead, M, R),
            torch.from_numpy(v).reshape(*lead, N, R))


def emu_bwd(lib, x, u0, v0, gy, T, G, solver, gu=None, gv=None):
    M, N = x.shape[-2:]
    R = u0.shape[1]
    xn = _np(x.reshape(-1, M, N))
    gyn = None if gy is None else _np(gy.reshape(-1, M, N))
    gun = None if gu is None else _np(gu)
    gvn = None if gv is None else _np(gv)
    gx = np.empty_like(xn)
    rc = lib.emu_solver_bwd(_p(xn), _p(_np(u0)), _p(_np(v0)), _p(gyn), _p(gun), _p(gvn), _p(gx), xn.shape[0], M, N, R, T, G,
                            SID[solver], 1e-16)
    assert rc == 0
    return torch.from_numpy(gx).reshape(x.shape)


def composed(x, u0, v0, T, G, solver, gy=None, gu=None, gv=None, dtype=torch.float64):
    """the package's composed path on CPU in `dtype` (autograd through the reference's update rules): y, u, v, dL/dx"""
    M, N = x.shape[-2:]
    mf = ft.MatrixFactorization((M, N), rank=u0.shape[1], init="uniform", solver=solver, num_iters=T, num_grad_steps=G)
    mf.init.u0.copy_(u0)
    mf.init.v0.copy_(v0)
    xx = x.to(dtype).requires_grad_(True)
    u, v = mf.decompose(xx)
    y = mf.reconstruct(u, v)
    outs, grads = [], []
    for o, g in ((y, gy), (u, gu), (v, gv)):
        if g is not None:
            outs.append(o)
            grads.append(g.to(dtype))
    gx = torch.autograd.grad(outs, xx, grads, allow_unused=True)[0] if outs and G > 0 else None
    if gx is None:
        gx = torch.zeros_like(xx)
    return y.detach(), u.detach(), v.detach(), gx


def _bound(got, ref64, ref32, rel=2e-4, mult=30.0):
    """|got - ref64| <= rel * max|ref64| + 1e-5 + mult * |fp32 composed - ref64|: the last term is the conditioning guard of
    test_emul_vs_oracle_shapes — where even the composed path in fp32 misses float64 (cd at R >= 3 on short factors, smu near
    n ~ eps), the bound is a stated multiple of that disagreement"""
    kink = (ref32.double() - ref64).abs().max().item()
    err = (got.double() - ref64).abs().max().item()
    return err, rel * ref64.abs().max().item() + 1e-5 + mult * kink


# ---- the reference's own outputs (goldens g11, tools/make_goldens.py) ---------------------------------------------------------
def _g11_names():
    z = np.load(os.path.join(HERE, "golden", "g11_solvers.npz"))
    return sorted({k.split(":")[0] for k in z.keys()})


@pytest.mark.parametrize("name", _g11_names())
def test_emul_vs_g11_goldens(emu, golden, name):
    g = golden("g11_solvers").case(name)
    solver = "cd" if name.startswith("cd") else "smu"
    T, G = (int(v) for v in re.search(r"_t(\d+)_g(\d+)$", name).groups())
    x, u0, v0 = g["x"], g["u0"], g["v0"]
    y, u, v = emu_fwd(emu, x, u0, v0, T, solver)
    y64, u64, v64, gx64 = composed(x, u0, v0, T, G, solver, gy=g["gy"])
    for what, got, ref in (("y", y, g["y"]), ("u", u, g["u"]), ("v", v, g["v"])):
        ref64 = {"y": y64, "u": u64, "v": v64}[what]
        err, bound = _bound(got, ref64, ref)
        assert err <= bound, (what, err, bound)
        # and the reference's fp32 numbers themselves, at the same conditioning-scaled bound
        assert (got - ref).abs().max().item() <= bound + (ref.double() - ref64).abs().max().item(), what
    gx = emu_bwd(emu, x, u0, v0, g["gy"], T, G, solver)
    err, bound = _bound(gx, gx64, g["gx"])
    assert err <= bound, ("gx", err, bound)


# ---- against float64 autograd across the shape families of test_emul_vs_oracle_shapes -----------------------------------
@pytest.mark.parametrize("M,N", [(8, 512), (8, 200), (8, 150), (8, 100), (4, 64), (16, 256), (16, 64), (32, 128), (32, 64), (5, 100)])
@pytest.mark.parametrize("solver,signed", [("cd", False), ("smu", False), ("smu", True)])
def test_emul_vs_float64_shapes(emu, M, N, solver, signed):
    torch.manual_seed(M * 1000 + N + 7 * signed)
    for R in (1, 2, 3, 4):
        x = torch.randn(3, M, N) if signed else torch.rand(3, M, N)
        x[1, :, : N // 2] = 0
        if solver == "cd":
            u0, v0 = torch.randn(M, R), torch.randn(N, R)
        else:
            u0, v0 = torch.rand(M, R), torch.rand(N, R)
        gy = torch.rand_like(x) - 0.5
        y, u, v = emu_fwd(emu, x, u0, v0, 4, solver)
        y64, _, _, _ = composed(x, u0, v0, 4, 0, solver)
        y32, _, _, _ = composed(x, u0, v0, 4, 0, solver, dtype=torch.float32)
        err, bound = _bound(y, y64, y32)
        assert err <= bound, (R, err, bound)
        for G in (4, 2):
            gx = emu_bwd(emu, x, u0, v0, gy, 4, G, solver)
            _, _, _, gx64 = composed(x, u0, v0, 4, G, solver, gy=gy)
            _, _, _, gx32 = composed(x, u0, v0, 4, G, solver, gy=gy, dtype=torch.float32)
            err, bound = _bound(gx, gx64, gx32)
            assert err <= bound, (R, G, err, bound)


@pytest.mark.parametrize("solver", ["cd", "smu"])
def test_emul_decompose_gradients(emu, solver):
    """dL/dx from gradients of the decompose() outputs u and v (no dL/dy), masked rows (M = 5) and columns (N = 100)"""
    torch.manual_seed(3)
    M, N, R, T, G = 5, 100, 2, 5, 3
    x = torch.rand(2, M, N)
    u0, v0 = torch.rand(M, R), torch.rand(N, R)
    gu, gv = torch.rand(2, M, R) - 0.5, torch.rand(2, N, R) - 0.5
    gx = emu_bwd(emu, x, u0, v0, None, T, G, solver, gu=gu, gv=gv)
    _, _, _, gx64 = composed(x, u0, v0, T, G, solver, gu=gu, gv=gv)
    _, _, _, gx32 = composed(x, u0, v0, T, G, solver, gu=gu, gv=gv, dtype=torch.float32)
    err, bound = _bound(gx, gx64, gx32)
    assert err <= bound, (err, bound)


def test_emulation_of_cd_smu_under_asan(tmp_path):
    """the CD / SMU instantiations of the wave program under AddressSanitizer + UBSan (the recipe of
    test_wave_program_emul.py::test_emulation_under_asan): ragged shapes, ranks 1-4, signed input, an all-zero matrix"""
    exe = str(tmp_path / "emul_solvers_asan")
    r = subprocess.run(["g++", "-O0", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        "-DFZ_EMUL_SOLVERS_MAIN", "-o", exe, SRC], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    assert "0 problem(s)" in r.stdout


# ---- routing ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key,want", [("cd", "cd"), ("nncd", "hals"), ("hals", "hals"), ("smu", "smu"), ("mu", "mu")])
def test_native_id_of_solver_keys(key, want):
    mf = ft.MatrixFactorization((8, 64), rank=2, solver=key)
    assert mf.solver.native_id == want


def test_native_id_of_a_custom_projection_is_none():
    s = nmf_mod.CoordinateDescent(project=nn.Sigmoid)
    assert s.native_id is None
    assert nmf_mod.CoordinateDescent().native_id == "cd"
    assert nmf_mod.SemiMultiplicativeUpdate().native_id == "smu"


def test_solver_ids_match_the_c_header():
    hdr = open(os.path.join(ROOT, "include", "factorizer_hip.h")).read()
    ids = {m.group(1).lower(): int(m.group(2)) for m in re.finditer(r"#define FZ_SOLVER_(\w+)\s+(\d+)", hdr)}
    assert ids == {"mu": 0, "hals": 1, "cd": 2, "smu": 3}
    assert _native.SOLVER_ID == ids


# ---- registers ------------------------------------------------------------------------------------------------------------------
def test_cfg1_shape_standalone_cd_smu_backward_does_not_spill():
    """the 8 x 512 fast-path backward of cd and smu (ranks 1 and 2, fp32) owns no scratch, like the MU / HALS instantiations
    test_no_spills.py::test_cfg1_shape_standalone_nmf_backward_does_not_spill pins"""
    import importlib.util
    from factorizer_amd import build as B
    B.build(verbose=False)
    spec = importlib.util.spec_from_file_location("scratch_audit", os.path.join(ROOT, "tools", "scratch_audit.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    for R in (1, 2):
        ks = {name: (scratch, spills, vgprs) for name, scratch, spills, vgprs in
              mod.kernels_of(os.path.join(CSRC, "build", f"nmf_r{R}_cdsmu.o"))}
        hits = {k: v for k, v in ks.items() if f"nmf_bwd_kernelILi8ELi8ELi{R}E" in k and "Lb1Ef" in k}
        assert sorted(re.search(rf"ILi8ELi8ELi{R}ELi(\d)E", k).group(1) for k in hits) == ["2", "3"], list(ks)[:5]
        for name, (scratch, spills, vgprs) in hits.items():
            assert spills == 0 and scratch == 0, (name, scratch, spills, vgprs)
