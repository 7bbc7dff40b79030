"""Block dropout without a GPU: the Philox4x32-10 of csrc/fz_philox.h (the device header compiled for the host) and the numpy
reference against the Random123 known-answer vectors, the packed bit layout, and the host-side argument checks of the
fz_dropout_* entry points (all before any device work)."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import philox_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "factorizer_amd", "csrc", "fz_philox.h")


@pytest.mark.parametrize("ctr,key,want", R.KAT)
def test_python_philox_known_answers(ctr, key, want):
    got = R.philox4x32_10(*ctr, *key)
    assert tuple(int(w) for w in got) == want


@pytest.fixture(scope="module")
def host_philox(tmp_path_factory):
    """fz_philox.h compiled by the host C++ compiler (as tests/emul builds its sources): philox(ctr[4], key[2], out[4])"""
    d = tmp_path_factory.mktemp("philox")
    src, lib = d / "philox_host.cpp", d / "philox_host.so"
    src.write_text('#include "%s"\n'
                   'extern "C" void philox(const uint32_t* c, const uint32_t* k, uint32_t* o, int n) {\n'
                   '  for (int i = 0; i < n; ++i) {\n'
                   '    const fz::philox4x32 r = fz::philox4x32_10(c[4*i], c[4*i+1], c[4*i+2], c[4*i+3], k[2*i], k[2*i+1]);\n'
                   '    for (int e = 0; e < 4; ++e) o[4*i+e] = r.v[e];\n'
                   '  }\n'
                   '}\n' % HEADER)
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-shared", "-fPIC", "-o", str(lib), str(src)])
    h = ctypes.CDLL(str(lib))
    P = ctypes.POINTER(ctypes.c_uint32)
    h.philox.argtypes = [P, P, P, ctypes.c_int]

    def run(ctr, key):
        ctr = np.ascontiguousarray(ctr, dtype=np.uint32).reshape(-1, 4)
        key = np.ascontiguousarray(key, dtype=np.uint32).reshape(-1, 2)
        out = np.zeros_like(ctr)
        h.philox(ctr.ctypes.data_as(P), key.ctypes.data_as(P), out.ctypes.data_as(P), ctr.shape[0])
        return out
    return run


def test_device_header_known_answers_and_reference(host_philox):
    for ctr, key, want in R.KAT:
        assert tuple(int(w) for w in host_philox([ctr], [key])[0]) == want
    rng = np.random.default_rng(0)
    ctr = rng.integers(0, 2 ** 32, (4096, 4), dtype=np.uint64)
    key = rng.integers(0, 2 ** 32, (4096, 2), dtype=np.uint64)
    ref = np.stack(R.philox4x32_10(ctr[:, 0], ctr[:, 1], ctr[:, 2], ctr[:, 3], key[:, 0], key[:, 1]), axis=1)
    assert np.array_equal(host_philox(ctr, key), ref.astype(np.uint32))


def test_bit_layout_and_threshold():
    keep = np.zeros((1, 2, 70), dtype=bool)
    keep[0, 0, [0, 31, 32, 69]] = True
    keep[0, 1, 5] = True
    w = R.pack_bits(keep).view(np.uint32)
    assert w.shape == (1, 2, 3)
    assert w[0, 0].tolist() == [1 | (1 << 31), 1, 1 << 5] and w[0, 1].tolist() == [1 << 5, 0, 0]
    assert R.keep_threshold(0.0) == 2 ** 32 and R.keep_mask(7, 1, 2, 3, 50, 0.0).all()
    assert R.keep_threshold(0.5) == 2 ** 31
    # word v & 3 of the counter (v >> 2, c, b, site)
    seed = (0x12345678 << 32) | 0x9ABCDEF0
    m = R.keep_mask(seed, 2, 2, 3, 10, 0.3)
    r = R.philox4x32_10(9 >> 2, 1, 1, 2, 0x9ABCDEF0, 0x12345678)
    assert m[1, 1, 9] == (int(r[9 & 3]) < R.keep_threshold(0.3))


@pytest.fixture(scope="module")
def lib():
    from factorizer_amd import build
    build.build(verbose=False)
    from factorizer_amd import _native
    return _native.lib()


def test_dropout_entry_points_exported(lib):
    from factorizer_amd import _native
    for n in ("fz_dropout_bits_words", "fz_dropout_keep_bits", "fz_dropout_apply"):
        assert hasattr(lib, n) and n in _native.declared_symbols()
    assert lib.fz_abi_version() == _native.ABI_VERSION == 7


def test_dropout_host_side_checks(lib):
    """every argument is checked on the host before a launch: no device is touched (there is none here)"""
    from factorizer_amd import _native
    E_SHAPE, E_ARG = -1, -4
    dummy, seed = ctypes.c_void_p(256), ctypes.c_void_p(512)
    assert lib.fz_dropout_bits_words(2, 3, 64) == 12 and lib.fz_dropout_bits_words(2, 3, 65) == 18
    assert lib.fz_dropout_bits_words(-1, 3, 64) == -1
    for p in (1.0, -0.1, 1.5, float("nan")):
        assert lib.fz_dropout_keep_bits(seed, 0, 2, 32, 64, p, dummy, None) == E_ARG
        assert b"[0, 1)" in lib.fz_last_error_string()
    assert lib.fz_dropout_keep_bits(None, 0, 2, 32, 64, 0.1, dummy, None) == E_ARG
    assert lib.fz_dropout_keep_bits(seed, 0, 2, 32, 64, 0.1, None, None) == E_ARG
    assert b"null" in lib.fz_last_error_string()
    assert lib.fz_dropout_keep_bits(seed, 3, 2, 32, 64, 0.1, dummy, None) == E_ARG
    assert lib.fz_dropout_keep_bits(seed, 0, -2, 32, 64, 0.1, dummy, None) == E_SHAPE
    assert lib.fz_dropout_keep_bits(seed, 0, 2, 32, -64, 0.1, dummy, None) == E_SHAPE
    # an empty plane is a valid no-op
    assert lib.fz_dropout_keep_bits(seed, 0, 0, 32, 64, 0.1, dummy, None) == 0
    f32 = _native.STORE_F32
    assert lib.fz_dropout_apply(7, dummy, 0.1, dummy, None, dummy, 2, 32, 64, f32, None) == E_ARG
    assert lib.fz_dropout_apply(_native.DROP_RES, dummy, 1.0, dummy, None, dummy, 2, 32, 64, f32, None) == E_ARG
    assert lib.fz_dropout_apply(_native.DROP_RES, None, 0.1, dummy, None, dummy, 2, 32, 64, f32, None) == E_ARG
    assert lib.fz_dropout_apply(_native.DROP_GELU_BWD, dummy, 0.1, dummy, None, dummy, 2, 32, 64, f32, None) == E_ARG
    assert lib.fz_dropout_apply(_native.DROP_RES, dummy, 0.1, dummy, None, dummy, -2, 32, 64, f32, None) == E_SHAPE
    assert lib.fz_dropout_apply(_native.DROP_RES, dummy, 0.1, dummy, None, dummy, 2, 32, 66, f32, None) == E_SHAPE
    assert lib.fz_dropout_apply(_native.DROP_RES, dummy, 0.1, dummy, None, dummy, 2, 32, 64, 5, None) == E_ARG
    assert lib.fz_dropout_apply(_native.DROP_RES, dummy, 0.1, ctypes.c_void_p(260), None, dummy, 2, 32, 64, f32, None) == E_ARG
