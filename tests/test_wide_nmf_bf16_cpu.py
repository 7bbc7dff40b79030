"""No GPU: the split-N NMF families on bf16 activation storage (fz_gnmf_fwd_act / _bwd_act, fz_gnmfx_fwd_act /
_bwd_act) — the entry points and their argument lists, their host-side refusals (those of the fp32 entry points plus
act_dtype), the workspace sizes, and the conditioning guard of every parity case on the bf16-rounded inputs
(tests/wide_bf16_cases.py)."""
import ctypes

import pytest

import wide_bf16_cases as WB
import wide_rank_cases as W
from factorizer_amd import _native

F32, BF16 = 0, 1   # FZ_STORE_F32, FZ_STORE_BF16
MU, HALS = _native.SOLVER_ID["mu"], _native.SOLVER_ID["hals"]


@pytest.fixture(scope="module")
def lib():
    from factorizer_amd import build
    build.build(verbose=False)
    return _native.lib()


def test_symbols_and_argument_lists(lib):
    vp, i, i64, f = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_float
    assert (_native.STORE_F32, _native.STORE_BF16) == (F32, BF16)
    # x u0 v0 y u_out v_out | nmat M N R T solver eps act_dtype | workspace stream
    fwd = [vp] * 6 + [i64, i, i64, i, i, i, f, i, vp, vp]
    # x u0 v0 gy gu gv gx | nmat M N R T Tgrad solver eps act_dtype | workspace stream
    bwd = [vp] * 7 + [i64, i, i64, i, i, i, i, f, i, vp, vp]
    for fam in ("gnmf", "gnmfx"):
        for name, args in ((f"fz_{fam}_fwd_act", fwd), (f"fz_{fam}_bwd_act", bwd)):
            assert _native._SIGS[name] == (args, i), name
            fn = getattr(lib, name)          # the library exports it
            assert list(fn.argtypes) == args and fn.restype is i
        # the fp32 entry points: the same lists without act_dtype
        assert _native._SIGS[f"fz_{fam}_fwd"][0] == fwd[:13] + fwd[14:]
        assert _native._SIGS[f"fz_{fam}_bwd"][0] == bwd[:15] + bwd[16:]
    assert lib.fz_abi_version() == 7


P8 = ctypes.c_void_p(8)   # a non-null pointer value the host code never dereferences


def _calls(lib, fam, act):
    """(fwd, bwd, names) of one family: the _act entry points with `act`, or (act None) the fp32 entry points"""
    sfx = "" if act is None else "_act"
    f, b = getattr(lib, f"fz_{fam}_fwd{sfx}"), getattr(lib, f"fz_{fam}_bwd{sfx}")
    ad = () if act is None else (act,)

    def fwd(M, N, R, solver, x=P8, ws=P8, nmat=2):
        return f(x, P8, P8, P8, None, None, nmat, M, N, R, 5, solver, 1e-16, *ad, ws, None)

    def bwd(M, N, R, solver, gy=P8, gu=None, gv=None, gx=P8, G=5, nmat=2):
        return b(P8, P8, P8, gy, gu, gv, gx, nmat, M, N, R, 5, G, solver, 1e-16, *ad, P8, None)

    return fwd, bwd, (f"fz_{fam}_fwd{sfx}".encode(), f"fz_{fam}_bwd{sfx}".encode())


OTHER = {   # shapes of the other families, and beyond every family
    "gnmfx": ((8, 1200, 5), (16, 4096, 1), (8, 512, 2), (513, 512, 26), (64, 4096, 33), (16, 4096, 17)),
    "gnmf": ((64, 1024, 7), (128, 2052, 13), (65, 1030, 1), (16, 4096, 5), (0, 512, 2), (16, 0, 1)),
}
OWN = {"gnmfx": (64, 1024, 7), "gnmf": (16, 4096, 1)}


@pytest.mark.parametrize("act", [None, F32, BF16], ids=["fp32-entry", "act-f32", "act-bf16"])
@pytest.mark.parametrize("fam", ["gnmf", "gnmfx"])
def test_entry_points_refuse(lib, fam, act):
    """codes and messages of the fp32 entry points (act None: they themselves still refuse the same things)"""
    fwd, bwd, (nf, nb) = _calls(lib, fam, act)
    err = lib.fz_last_error_string
    for M, N, R in OTHER[fam]:
        assert fwd(M, N, R, HALS) == -2 and err().startswith(nf + b":")
        assert bwd(M, N, R, HALS) == -2 and err().startswith(nb + b":")
        assert getattr(lib, f"fz_{fam}_workspace_bytes")(2, M, N, R, 5, 1) == -1
        assert getattr(lib, f"fz_{fam}_workspace_bytes_act")(2, M, N, R, 5, 1, BF16) == -1
    M, N, R = OWN[fam]
    bad_solvers = (4, -1) + ((_native.SOLVER_ID["cd"], _native.SOLVER_ID["smu"]) if fam == "gnmfx" else ())
    for solver in bad_solvers:
        assert fwd(M, N, R, solver) == -4 and b"solver" in err() and err().startswith(nf + b":")
        assert bwd(M, N, R, solver) == -4 and b"solver" in err() and err().startswith(nb + b":")
    assert fwd(M, N, R, HALS, x=None) == -4 and b"null" in err() and err().startswith(nf + b":")
    assert fwd(M, N, R, MU, ws=None) == -4 and b"null" in err()
    assert bwd(M, N, R, HALS, gy=None) == -4 and b"null" in err() and err().startswith(nb + b":")
    assert bwd(M, N, R, HALS, gx=None) == -4 and b"null" in err()
    assert fwd(M, N, R, HALS, nmat=65536) == -1 and err().startswith(nf + b":")
    assert bwd(M, N, R, MU, nmat=65536) == -1 and err().startswith(nb + b":")
    assert bwd(M, N, R, HALS, G=0) == -4 and b"no iteration" in err()      # the caller returns zeros
    assert fwd(M, N, R, HALS, nmat=0) == 0 and bwd(M, N, R, HALS, nmat=0) == 0   # nothing to do


@pytest.mark.parametrize("fam", ["gnmf", "gnmfx"])
@pytest.mark.parametrize("bad", [2, -1])
def test_act_dtype_outside_the_enum_is_refused(lib, fam, bad):
    fwd, bwd, (nf, nb) = _calls(lib, fam, bad)
    M, N, R = OWN[fam]
    assert fwd(M, N, R, HALS) == -4 and b"act_dtype" in lib.fz_last_error_string()
    assert lib.fz_last_error_string().startswith(nf + b":")
    assert bwd(M, N, R, HALS) == -4 and b"act_dtype" in lib.fz_last_error_string()
    assert lib.fz_last_error_string().startswith(nb + b":")
    assert getattr(lib, f"fz_{fam}_workspace_bytes_act")(2, M, N, R, 5, 1, bad) == -1


@pytest.mark.parametrize("fam,M,N,R", [("gnmf", 16, 4096, 1), ("gnmf", 5, 777, 2), ("gnmf", 64, 1024, 4),
                                       ("gnmfx", 64, 1024, 7), ("gnmfx", 128, 2052, 13), ("gnmfx", 512, 512, 26)])
def test_workspace_and_launches_do_not_depend_on_storage(lib, fam, M, N, R):
    """launch counts and `supported` have no storage argument at all; the workspace of either storage type is that of
    the fp32 entry points, but for the fp32 running sum of gX (nmat·M·N floats, padded to 16 bytes) that a bf16 BACKWARD
    keeps so that each gX element is rounded once"""
    ws, wsa = getattr(lib, f"fz_{fam}_workspace_bytes"), getattr(lib, f"fz_{fam}_workspace_bytes_act")
    for nmat in (1, 3):
        for T in (0, 1, 5):
            for backward in (0, 1):
                base = ws(nmat, M, N, R, T, backward)
                assert base > 0 and wsa(nmat, M, N, R, T, backward, F32) == base
                acc = 4 * ((nmat * M * N + 3) // 4 * 4) if backward else 0
                assert wsa(nmat, M, N, R, T, backward, BF16) == base + acc
    assert wsa(-1, M, N, R, 5, 0, BF16) == -1


@pytest.mark.parametrize("M,N,R,T,G,solver", W.PAIRS, ids=W.IDS)
def test_conditioning_guard_on_rounded_inputs(M, N, R, T, G, solver):
    """x and gy rounded to bf16: the fp32 oracle within 3e-5 of the float64 oracle, y and gx (worst of the 23 pairs:
    9.8e-6, 256 x 520 R 25 HALS, gx)"""
    assert W.GUARD == 3e-5
    WB.guard(M, N, R, T, G, solver)
