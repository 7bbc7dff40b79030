"""CPU checks of the out-projection on the core's rank-1 factors (csrc/cf_patch.h, csrc/outproj_fac.h): the voxel -> patch map
the kernels use, compiled for the host (tests/emul/emul_cf_patch.cpp), against brute force over the oracle's gather formula for
every voxel; the predicate; and the host-side refusals of every launch that brings factors where no kernel takes them (nothing
is launched: the entry points check before they touch the device)."""
import ctypes
import os
import subprocess

import numpy as np
import pytest
import torch

from oracle import cpu_ref as O

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "emul", "emul_cf_patch.cpp")
HDR = os.path.join(os.path.dirname(HERE), "factorizer_amd", "csrc", "cf_patch.h")

GRIDS = [(8, 8, 64), (16, 8, 128)]
# both orders of a plain and a shifted window, the shifted-first-window pair of tests/test_gpu_cf_factors.py, and shifts that wrap
# on all three axes (negative ones as the library normalises them)
SHIFT_PAIRS = [[(0, 0, 0), (4, 4, 4)], [(4, 4, 4), (0, 0, 0)], [(4, 4, 0), (0, 4, 4)], [(-4, -4, -4), (12, 4, 60)]]


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    lib = str(tmp_path_factory.mktemp("cf_patch") / "_fz_emul_cf_patch.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-o", lib, SRC])
    h = ctypes.CDLL(lib)
    h.emu_cf_voxel_patch.argtypes = [ctypes.c_int] * 6 + [ctypes.c_void_p]
    h.emu_cf_voxel_patch.restype = None
    return h


def _brute(S, shift):
    """patch of every voxel from the gather formula y[g, p] = x[(8 g + p - s) mod S] (oracle/cpu_ref.py swm_gather_index)"""
    grid = tuple(v // 8 for v in S)
    idx = O.swm_gather_index(1, 8, S, 1, 8, grid, (8, 8, 8), shift)      # (1, G, 8, 512) flat indices into (1, 8, *S)
    vox = idx[0, :, 0, :]                                                # channel 0: the flat index is the voxel
    V = S[0] * S[1] * S[2]
    out = torch.full((V,), -1, dtype=torch.long)
    out[vox.reshape(-1)] = torch.arange(vox.shape[0]).view(-1, 1).expand_as(vox).reshape(-1)
    assert (out >= 0).all()                                              # the window's patches tile the volume
    return out.numpy()


@pytest.mark.parametrize("S", GRIDS)
@pytest.mark.parametrize("pair", SHIFT_PAIRS, ids=["000_444", "444_000", "440_044", "neg_wrap"])
def test_voxel_patch_map_equals_the_gather_formula(emu, S, pair):
    assert os.path.exists(HDR)
    for shift in pair:
        s = [v % n for v, n in zip(shift, S)]                            # normalised to [0, size) as the host code does
        got = np.empty(S[0] * S[1] * S[2], np.int32)
        emu.emu_cf_voxel_patch(*S, *s, got.ctypes.data)
        ref = _brute(S, shift)
        assert np.array_equal(got, ref), (S, shift, int((got != ref).sum()))
    # the wave's view: 64 consecutive voxels along W touch 8 patches of a window (9 when its W-axis shift is 4 mod 8), in
    # ascending cyclic order from the first voxel's patch — what outproj_fac.h stages per wave
    for shift in pair:
        s = [v % n for v, n in zip(shift, S)]
        got = np.empty(S[0] * S[1] * S[2], np.int32)
        emu.emu_cf_voxel_patch(*S, *s, got.ctypes.data)
        rows = got.reshape(-1, 64)
        G2 = S[2] // 8
        for r in rows[:: max(1, len(rows) // 64)]:
            first, base = r[0] % G2, r[0] - r[0] % G2
            rel = ((s[2] & 7) + np.arange(64)) >> 3
            assert np.array_equal(r, base + (first + rel) % G2)
            assert rel.max() == (8 if s[2] & 7 else 7)


# ---------------------------------------------------------------- predicate and refusals (host side) ----------------------
@pytest.fixture(scope="module")
def native():
    from factorizer_amd import _native, build
    build.build(verbose=False)
    return _native


def _pred(N, C=32, Hd=64, S=(8, 8, 64), shifts=((0, 0, 0), (4, 4, 4)), R=1, ad=None, products=None, dropout=0):
    flat = [v for s in shifts for v in s]
    return N.lib().fz_outproj_factors_supported(C, Hd, *S, 8, 8, 8, 8, R, 5, 5, len(shifts), (N._i * len(flat))(*flat),
                                                N.STORE_F32 if ad is None else ad,
                                                N.PRODUCTS_SPLIT_BF16 if products is None else products, dropout)


def test_predicate(native):
    N = native
    assert _pred(N) == 1 and _pred(N, S=(16, 8, 128), shifts=((4, 4, 0), (0, 4, 4))) == 1
    assert _pred(N, C=64) == 0 and _pred(N, Hd=128) == 0                 # stage 1, mlp_ratio 4
    assert _pred(N, ad=N.STORE_BF16) == 0
    assert _pred(N, products=N.PRODUCTS_FP32_MFMA) == 0
    assert _pred(N, dropout=1) == 0
    assert _pred(N, R=2) == 0
    assert _pred(N, shifts=((0, 0, 0), (2, 2, 2), (4, 4, 4), (6, 6, 6))) == 0
    assert _pred(N, shifts=((0, 0, 0), (4, 4, 2))) == 0 and _pred(N, S=(8, 8, 32)) == 0


P8 = 8     # a non-null pointer value the host code never dereferences


def _fac(N, S=(8, 8, 64), heads=4, shifts=(0, 0, 0, 4, 4, 4), ptrs=(P8,) * 4):
    f = N.OutprojFac()
    f.v[0], f.u[0], f.v[1], f.u[1] = ptrs
    f.dims[:] = list(S)
    f.heads = heads
    f.shift[:] = list(shifts)
    return f


def _mlp(N, C=32, Hd=64, V=4096, mode=0, ad=None, products=None, pre_in=None):
    d = N.MlpDesc()
    d.mode, d.w1, d.w2, d.ln_g, d.ln_b, d.stats, d.z1, d.out = mode, P8, P8, P8, P8, P8, P8, P8
    d.inp = d.x1 = d.gz1 = d.part = d.gln = d.wpart = d.gw1 = d.gb1 = d.gw2 = d.gb2 = d.glp = P8
    d.B, d.C, d.H, d.V = 1, C, Hd, V
    d.act_dtype = N.STORE_F32 if ad is None else ad
    d.products = N.PRODUCTS_SPLIT_BF16 if products is None else products
    d.pre_in, d.pre_w, d.pre_res, d.pre_out = pre_in, P8, P8, P8
    return d


def _dw(N, ad=None, ln=0, q=None, drop=None):
    d = N.GemmDwDesc()
    d.g, d.q, d.w, d.y, d.wpart, d.gw = P8, q, P8, P8, P8, P8
    d.stats = d.ln_g = d.ln_b = d.gln = P8
    d.ln, d.B, d.C, d.V = ln, 1, 32, 4096
    d.act_dtype = N.STORE_F32 if ad is None else ad
    if drop:
        d.drop_m, d.drop_s = P8, 2.0
    return d


def test_factor_launches_outside_the_supported_form_are_refused(native):
    N = native
    L, U, A = N.lib(), N.FZ_E_UNSUPPORTED, -4
    n0 = N.launch_count()
    chain = lambda d, f=None: L.fz_mlp_chain_fac(ctypes.byref(d), ctypes.byref(f if f is not None else _fac(N)), None)   # noqa: E731
    dw = lambda d, f=None: L.fz_gemm_dw_fac(ctypes.byref(d), ctypes.byref(f if f is not None else _fac(N)), None)        # noqa: E731
    err = lambda: L.fz_last_error_string()                        # noqa: E731
    # the chain: the C = 64 form, hidden 128, modes 1 and 2, bf16 storage, fp32-MFMA products, a tensor AND factors
    assert chain(_mlp(N, C=64, Hd=128)) == U and b"fz_mlp_chain_fac" in err()
    assert chain(_mlp(N, Hd=128)) == U and b"fz_mlp_chain_fac" in err()
    assert chain(_mlp(N, mode=1)) == U and b"fz_mlp_chain_fac" in err()
    assert chain(_mlp(N, mode=2)) == U and b"fz_mlp_chain_fac" in err()
    assert chain(_mlp(N, ad=N.STORE_BF16)) == U and b"fz_mlp_chain_fac" in err()
    assert chain(_mlp(N, products=N.PRODUCTS_FP32_MFMA)) == U and b"fz_mlp_chain_fac" in err()
    assert chain(_mlp(N, pre_in=P8)) == U and b"fz_mlp_chain_fac" in err()
    assert L.fz_mlp_chain_fac(ctypes.byref(_mlp(N)), None, None) == A
    # a supported launch with broken factors
    assert chain(_mlp(N), _fac(N, ptrs=(P8, P8, None, P8))) == A
    assert chain(_mlp(N), _fac(N, heads=2)) == U
    assert chain(_mlp(N), _fac(N, S=(8, 8, 32))) == U
    assert chain(_mlp(N), _fac(N, S=(8, 16, 64))) == U                     # D H W != V
    assert chain(_mlp(N), _fac(N, shifts=(0, 0, 0, 4, 4, 2))) == U
    d = _mlp(N)
    d.pre_w = None
    assert chain(d) == A                                                    # the out-projection's own operands are still checked
    # fz_gemm_dw_fac: the LayerNorm form, bf16 storage, dropout, a tensor AND factors
    assert dw(_dw(N, ln=1)) == U and b"fz_gemm_dw_fac" in err()
    assert dw(_dw(N, ad=N.STORE_BF16)) == U and b"fz_gemm_dw_fac" in err()
    assert dw(_dw(N, drop=True)) == U and b"fz_gemm_dw_fac" in err()
    assert dw(_dw(N, q=P8)) == U and b"fz_gemm_dw_fac" in err()
    assert dw(_dw(N), _fac(N, ptrs=(None, P8, P8, P8))) == A
    assert dw(_dw(N), _fac(N, heads=8)) == U and dw(_dw(N), _fac(N, S=(8, 8, 96))) == U
    assert dw(_dw(N), _fac(N, shifts=(0, 0, 2, 4, 4, 4))) == U
    assert L.fz_gemm_dw_fac(ctypes.byref(_dw(N)), None, None) == A
    assert L.fz_gemm_dw(ctypes.byref(_dw(N)), None) == A                    # the tensor form still needs its q
    # fz_nmf_cf_factors_to_tensor
    z, s = (N._i * 3)(0, 0, 0), (N._i * 3)(4, 4, 4)
    f2t = lambda *a: L.fz_nmf_cf_factors_to_tensor(*a, None)      # noqa: E731
    assert f2t(P8, P8, P8, P8, P8, 1, 32, 8, 8, 64, z, s, N.STORE_BF16) == U
    assert f2t(P8, P8, None, P8, P8, 1, 32, 8, 8, 64, z, s, N.STORE_F32) == A
    assert f2t(P8, P8, P8, P8, P8, 1, 32, 8, 8, 32, z, s, N.STORE_F32) == U
    assert f2t(P8, P8, P8, P8, P8, 1, 32, 8, 8, 64, z, (N._i * 3)(4, 4, 2), N.STORE_F32) == U
    assert N.launch_count() == n0                                           # nothing was launched


def test_switch_and_binding():
    from factorizer_amd import _native as N, functional as Fn
    assert Fn._OUTPROJ_FACTORS == (os.environ.get("FZ_OUTPROJ_FACTORS", "1") != "0")
    # fz_outproj_fac: two pointer pairs, then 3 + 1 + 6 ints (include/factorizer_hip.h)
    assert [f[0] for f in N.OutprojFac._fields_] == ["v", "u", "dims", "heads", "shift"] and ctypes.sizeof(N.OutprojFac) == 32 + 40
