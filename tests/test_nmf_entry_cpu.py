"""No GPU: the host side of the wave-resident NMF entry points (csrc/nmf.hip) — every refusal of fz_nmf_fwd / fz_nmf_bwd
with its code and message, the shape table that fz_nmf_supported sizes the LDS history from against the rows the
launchers take (csrc/nmf_shapes.h), and the Tgrad clamp of the split-N launch counts.  Every call here returns before
the first device call."""
import ctypes

import pytest

from factorizer_amd import _native

P8 = ctypes.c_void_p(8)   # a non-null pointer value the host code never dereferences
MU, HALS, CD, SMU = (_native.SOLVER_ID[s] for s in ("mu", "hals", "cd", "smu"))


@pytest.fixture(scope="module")
def lib():
    from factorizer_amd import build
    build.build(verbose=False)
    return _native.lib()


def _fwd(lib, nmat=2, M=8, N=64, R=2, T=5, solver=HALS, act=0, x=P8, u0=P8, v0=P8, y=P8):
    return lib.fz_nmf_fwd(x, u0, v0, y, None, None, nmat, M, N, R, T, solver, 1e-16, act, None)


def _bwd(lib, nmat=2, M=8, N=64, R=2, T=5, solver=HALS, act=0, x=P8, u0=P8, v0=P8, gy=P8, gu=None, gv=None, gx=P8, G=5):
    return lib.fz_nmf_bwd(x, u0, v0, gy, gu, gv, gx, nmat, M, N, R, T, G, solver, 1e-16, act, None)


REFUSALS = (
    [(kw, -1, b"sizes") for kw in ({"nmat": -1}, {"M": 0}, {"N": 0}, {"T": -1})]
    + [({"solver": s}, -4, b"solver") for s in (4, -1)]
    + [({"R": r}, -2, b"rank") for r in (0, 5)]
    + [({"M": m, "N": n}, -2, b"outside") for m, n in ((33, 64), (8, 513), (16, 257), (32, 129))]
    + [({p: None}, -4, b"null") for p in ("x", "u0", "v0")]
)


@pytest.mark.parametrize("kw,code,frag", REFUSALS, ids=lambda v: "-".join(f"{k}{x}" for k, x in v.items()) if isinstance(v, dict) else None)
def test_refusals_of_both_directions(lib, kw, code, frag):
    assert _fwd(lib, **kw) == code and frag in lib.fz_last_error_string()
    assert lib.fz_last_error_string().startswith(b"fz_nmf")
    assert _bwd(lib, **kw) == code and frag in lib.fz_last_error_string()
    assert lib.fz_last_error_string().startswith(b"fz_nmf")


def test_refusals_of_one_direction(lib):
    err = lib.fz_last_error_string
    assert _fwd(lib, y=None) == -4 and b"null" in err() and err().startswith(b"fz_nmf_fwd:")
    assert _bwd(lib, gx=None) == -4 and b"null" in err() and err().startswith(b"fz_nmf_bwd:")
    assert _bwd(lib, gy=None, gu=None, gv=None) == -4 and b"null" in err() and err().startswith(b"fz_nmf_bwd:")


@pytest.mark.parametrize("solver", [MU, HALS, CD, SMU])
def test_order_of_the_last_checks(lib, solver):
    """shape and solver refusals come before the pointers, the pointers before nmat == 0, and nmat == 0 (nothing to do)
    before the storage type"""
    err = lib.fz_last_error_string
    assert _fwd(lib, solver=solver, nmat=0) == 0 and _bwd(lib, solver=solver, nmat=0) == 0
    assert _fwd(lib, solver=solver, nmat=0, act=2) == 0 and _bwd(lib, solver=solver, nmat=0, act=2) == 0
    assert _fwd(lib, solver=solver, nmat=0, x=None) == -4 and _bwd(lib, solver=solver, nmat=0, x=None) == -4
    assert _fwd(lib, solver=solver, M=33, x=None) == -2 and _bwd(lib, solver=solver, M=33, x=None) == -2
    assert _fwd(lib, solver=4, R=5, M=33) == -4 and _fwd(lib, M=0, solver=4) == -1 and _fwd(lib, R=5, M=33) == -2
    for act in (2, -1):
        assert _fwd(lib, solver=solver, act=act) == -4 and b"act_dtype" in err() and err().startswith(b"fz_nmf")
        assert _bwd(lib, solver=solver, act=act) == -4 and b"act_dtype" in err() and err().startswith(b"fz_nmf")


# (MP, NPL, largest M, largest N): the register footprints of the kernel families, smallest first
SHAPES = [(8, 1, 8, 64), (8, 2, 8, 128), (8, 3, 8, 192), (8, 4, 8, 256), (8, 8, 8, 512), (16, 1, 16, 64), (16, 4, 16, 256),
          (32, 1, 32, 64), (32, 2, 32, 128)]


def _hist_bytes(MP, NPL, R, G):
    return 4 * ((G + 1) * R * NPL * 64 + (G + 1) * MP * R + G * (MP * R + R * R))


@pytest.mark.parametrize("R", [1, 2, 3, 4])
@pytest.mark.parametrize("MP,NPL,M,N", SHAPES, ids=[f"{s[2]}x{s[3]}" for s in SHAPES])
def test_history_is_sized_for_the_row_the_launcher_takes(lib, MP, NPL, M, N, R):
    """the largest number of graded iterations whose history (Hist<MP, NPL, R>::floats, csrc/nmf_kernels.inc) fits 160 KiB
    of LDS, at the largest matrix of each row: fz_nmf_supported turns exactly there"""
    G = 0
    while _hist_bytes(MP, NPL, R, G + 1) <= 160 * 1024:
        G += 1
    assert _hist_bytes(MP, NPL, R, G) <= 160 * 1024 < _hist_bytes(MP, NPL, R, G + 1)
    assert lib.fz_nmf_supported(M, N, R, G, G) == 1
    assert lib.fz_nmf_supported(M, N, R, G + 1, G + 1) == 0


@pytest.mark.parametrize("T", [0, 1, 5])
def test_launch_counts_clamp_tgrad(lib, T):
    for backward in (0, 1):
        assert lib.fz_gnmf_launches(T, T, backward) == lib.fz_gnmf_launches(T, T + 3, backward)
        assert lib.fz_gnmf_launches(T, 0, backward) == lib.fz_gnmf_launches(T, -2, backward)
        assert lib.fz_gnmfx_launches(64, 1024, 7, T, T, backward) == lib.fz_gnmfx_launches(64, 1024, 7, T, T + 3, backward)
        assert lib.fz_gnmfx_launches(64, 1024, 7, T, 0, backward) == lib.fz_gnmfx_launches(64, 1024, 7, T, -2, backward)
    assert lib.fz_gnmf_launches(5, 5, 1) > lib.fz_gnmf_launches(5, 0, 1)
    assert lib.fz_gnmfx_launches(64, 1024, 7, 5, 5, 1) > lib.fz_gnmfx_launches(64, 1024, 7, 5, 0, 1)
