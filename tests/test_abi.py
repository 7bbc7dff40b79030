"""The C-ABI shared library builds for gfx950, loads, and exports every symbol that
include/factorizer_hip.h declares (no compute calls — there is no GPU in this container)."""
import ctypes
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def built_lib():
    from factorizer_amd import build
    return build.build(verbose=False)


def header_functions():
    src = open(os.path.join(ROOT, "include", "factorizer_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(fz_[a-z0-9_]+)\s*\(", src)))


def test_header_symbols_exported(built_lib):
    names = header_functions()
    assert {"fz_swm_fwd", "fz_swm_inv", "fz_nmf_fwd", "fz_nmf_bwd", "fz_version"} <= set(names)
    lib = ctypes.CDLL(built_lib)
    for n in names:
        assert hasattr(lib, n), f"{n} declared in include/factorizer_hip.h but not exported"


def test_integration_md_names_every_entry_point():
    """INTEGRATION.md maps each entry point to the reference call site it replaces: none may be missing from it."""
    text = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    missing = [n for n in header_functions() if n not in text]
    assert not missing, missing


def test_python_binding_matches_header(built_lib):
    from factorizer_amd import _native
    assert set(_native.declared_symbols()) <= set(header_functions())
    lib = _native.lib()
    assert lib.fz_version() >= 100
    assert lib.fz_abi_version() == _native.ABI_VERSION   # the loader refuses a library of another revision
    assert lib.fz_last_error_string() is not None


def test_binding_covers_every_entry_point():
    """the binding is derived from the header: no entry point is missing from it and none is bound that the header lacks"""
    from factorizer_amd import _native
    assert set(_native.declared_symbols()) == set(header_functions())
    assert len(_native.declared_symbols()) > 100


def test_descriptor_layouts_match_the_c_compiler(tmp_path):
    """sizeof and every offsetof of the header's structs, as the host C compiler lays them out, against the ctypes classes"""
    from factorizer_amd import _header, _native
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang")
    if cc is None:
        pytest.skip("no host C compiler")
    structs = _header.read().structs
    assert len(structs) >= 9
    lines = ["#include <stddef.h>", "#include <stdio.h>", '#include "factorizer_hip.h"', "int main(void) {"]
    for name, fields in structs.items():
        lines.append(f'  printf("{name} %zu\\n", sizeof({name}));')
        lines += [f'  printf("{name}.{f} %zu\\n", offsetof({name}, {f}));' for _, f, _ in fields]
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines + ["  return 0;", "}"]) + "\n")
    subprocess.run([cc, "-I", _header.INCLUDE_DIR, "-o", str(tmp_path / "layout"), str(src)], check=True)
    out = subprocess.run([str(tmp_path / "layout")], check=True, capture_output=True, text=True).stdout
    compiled = {k: int(v) for k, v in (line.split() for line in out.splitlines())}
    bound = {}
    for name, fields in structs.items():
        cls = _native._DESC[name]
        assert len(cls._fields_) == len(fields), name
        bound[name] = ctypes.sizeof(cls)
        for (_, f, _), (pyname, _) in zip(fields, cls._fields_):   # positional: fz_mlp_desc.in is `inp` in Python
            bound[f"{name}.{f}"] = getattr(cls, pyname).offset
    assert bound == compiled


def _parse_error(text):
    from factorizer_amd import _header
    with pytest.raises(_header.NativeError) as e:
        _header.parse(text)
    return str(e.value)


def test_header_reader_on_snippets():
    from factorizer_amd import _header
    T = _header.CType
    h = _header.parse("""
        /* a comment with ; and ( in it: fz_not_a_function(int x); */
        #ifndef GUARD_H
        #define GUARD_H
        #define FZ_ZERO 0
        #define FZ_E_BAD (-3) /* ; ( */
        typedef void* fz_stream_t; // hipStream_t; fz_neither(
        struct fz_geom;
        typedef struct fz_geom {
          int Di, Hi, Wi;       /* multi-declarator; */
          const void* x[4];
          double scale[3];
          int64_t V;
          const uint32_t* bits;
        } fz_geom;
        int fz_version(void);
        const char* fz_text(void);
        int64_t fz_three_lines(const void* x /* activation */, const int* shifts,
                               const struct fz_geom* geom, float eps,
                               fz_stream_t stream);
        int fz_group(const fz_geom* const* descs, void* const* workspaces, int n);
        #endif
    """)
    assert h.defines == {"FZ_ZERO": 0, "FZ_E_BAD": -3}
    assert h.structs == {"fz_geom": [(T("int", 0), "Di", 0), (T("int", 0), "Hi", 0), (T("int", 0), "Wi", 0), (T("void", 1), "x", 4),
                                     (T("double", 0), "scale", 3), (T("int64_t", 0), "V", 0), (T("uint32_t", 1), "bits", 0)]}
    assert list(h.functions) == ["fz_version", "fz_text", "fz_three_lines", "fz_group"]
    assert h.functions["fz_version"] == (T("int", 0), [])
    assert h.functions["fz_text"] == (T("char", 1), [])
    assert h.functions["fz_three_lines"] == (T("int64_t", 0), [(T("void", 1), "x"), (T("int", 1), "shifts"), (T("fz_geom", 1), "geom"),
                                                               (T("float", 0), "eps"), (T("fz_stream_t", 0), "stream")])
    assert h.functions["fz_group"] == (T("int", 0), [(T("fz_geom", 2), "descs"), (T("void", 2), "workspaces"), (T("int", 0), "n")])


@pytest.mark.parametrize("text, names", [
    ("int fz_f(size_t n);", ["fz_f", "size_t"]),                              # a type without a rule
    ("int fz_f(unsigned n);", ["fz_f", "unsigned"]),
    ("int fz_f(const float*** p);", ["fz_f", "float***"]),
    ("void* fz_f(int n);", ["fz_f"]),                                         # a return type without a rule
    ("typedef struct fz_s { short a; } fz_s;", ["fz_s", "short"]),
    ("typedef struct fz_s { int (*cb)(int); } fz_s;", ["fz_s", "cb"]),        # a field that does not fit
    ("typedef struct fz_s { int a : 3; } fz_s;", ["fz_s", "a : 3"]),
    ("static inline int fz_x(int a) { return a; }", ["fz_x"]),                # fz_x( left over: not a prototype
    ("int fz_a(int x), fz_b(int y);", ["fz_a"]),
    ("int fz_f(int n); int fz_f(int n);", ["fz_f"]),                          # declared twice
    ("#define FZ_N 1u", ["FZ_N"]),                                            # a constant that is not an integer
    ("#define FZ_CALL(x) fz_x(x)", ["FZ_CALL"]),
    ("struct fz_unknown;", ["fz_unknown"]),
])
def test_header_reader_refuses(text, names):
    msg = _parse_error(text)
    assert all(n in msg for n in names), msg


def test_host_side_argument_checks(built_lib):
    """Entry points validate shapes before touching the device (no GPU needed)."""
    from factorizer_amd import _native
    lib = _native.lib()
    sh = _native.shifts_array([(0, 0, 0)])
    rc = lib.fz_swm_fwd(None, None, 1, 30, 8, 8, 8, 8, 4, 4, 4, 1, sh, 4, 0, 1, None)
    assert rc == -1 and b"head_dim" in lib.fz_last_error_string()
    rc = lib.fz_swm_fwd(None, None, 1, 32, 10, 12, 10, 8, 8, 8, 8, 1, sh, 4, 0, 1, None)
    assert rc == -1 and b"patch" in lib.fz_last_error_string()
    assert lib.fz_nmf_supported(8, 512, 1, 5, 5) == 1
    assert lib.fz_nmf_supported(8, 512, 2, 10, 10) == 1
    assert lib.fz_nmf_supported(16, 262144, 1, 5, 5) == 0
    assert lib.fz_nmf_supported(8, 512, 5, 5, 5) == 0
    rc = lib.fz_nmf_fwd(None, None, None, None, None, None, 4, 8, 512, 9, 5, 1, 1e-16, 0, None)
    assert rc == -2
    # storage type of the activations (FZ_STORE_F32 / FZ_STORE_BF16): anything else is refused by the host code
    d = _native.GemmDesc()
    d.act_dtype = 7
    assert lib.fz_gemm(ctypes.byref(d), None) == -4 and b"act_dtype" in lib.fz_last_error_string()
    w = _native.WgradDesc()
    w.act_dtype = 7
    assert lib.fz_wgrad(ctypes.byref(w), ctypes.c_void_p(8), None) == -4
    rc = lib.fz_swm_inv(ctypes.c_void_p(8), ctypes.c_void_p(8), 1, 8, 8, 8, 8, 8, 8, 8, 8, 1, sh, 1, None, 5, None)
    assert rc == -4 and b"act_dtype" in lib.fz_last_error_string()


def test_fused_core_history_limit(built_lib):
    """fz_nmf_cf_supported sizes the backward's per-wave history (Hist<8, 8, R>::floats(G), csrc/nmf_core.h) against 160 KB of
    LDS: rank 1 fits up to T = G = 76 (162 896 bytes; 77: 165 012), rank 2 up to 37 (161 040; 38: 165 280)."""
    from factorizer_amd import _native
    lib = _native.lib()

    def ok(R, T):
        return lib.fz_nmf_cf_supported(8, 8, 8, 8, 8, 8, 8, 8, R, T, T)

    assert ok(1, 76) == 1 and ok(1, 77) == 0
    assert ok(2, 37) == 1 and ok(2, 38) == 0


def test_fused_chain_and_finish_queue_argument_checks(built_lib):
    """Round-5 entry points: which shapes take the out-projection in front of the MLP chain, what the descriptor must carry, and
    the finish queue's host-side state — all decided before anything touches the device."""
    from factorizer_amd import _native
    lib = _native.lib()
    S = _native.PRODUCTS_SPLIT_BF16
    assert lib.fz_mlp_pre_supported(32, 64, 128 ** 3, S) == 1 and lib.fz_mlp_pre_supported(32, 64, 120, S) == 1
    assert lib.fz_mlp_pre_supported(64, 128, 64 ** 3, S) == 1          # 1024 tiles of 256 voxels per sample: even
    assert lib.fz_mlp_pre_supported(64, 128, 120, S) == 0              # one tile: the 512-thread form walks tiles in pairs
    assert lib.fz_mlp_pre_supported(64, 128, 64 ** 3, _native.PRODUCTS_FP32_MFMA) == 0
    assert lib.fz_mlp_pre_supported(32, 128, 128 ** 3, S) == 0 and lib.fz_mlp_pre_supported(128, 256, 32 ** 3, S) == 0
    p8 = 8   # (a non-null pointer value the host code never dereferences)
    d = _native.MlpDesc()
    d.mode, d.B, d.C, d.H, d.V, d.act_dtype, d.products = 0, 1, 64, 128, 64 ** 3, _native.STORE_F32, S
    d.w1 = d.w2 = d.out = d.z1 = d.stats = d.ln_g = d.ln_b = p8
    d.pre_in = p8                                                          # ... without pre_w / pre_res / pre_out
    assert lib.fz_mlp_chain(ctypes.byref(d), None) == -4 and b"pre_in" in lib.fz_last_error_string()
    d.pre_w = d.pre_res = d.pre_out = p8
    d.post_out, d.post_w, d.post_m = p8, p8, 3                             # the head rides only in the C = 32 chain
    assert lib.fz_mlp_chain(ctypes.byref(d), None) == -4 and b"post_out" in lib.fz_last_error_string()
    d.post_out = None
    d.V = 120
    assert lib.fz_mlp_chain(ctypes.byref(d), None) == -2                   # FZ_E_UNSUPPORTED (fz_mlp_pre_supported says no)
    # finish queue: state only
    assert lib.fz_finish_defer(-1) == 0 and lib.fz_finish_pending() == 0 and lib.fz_finish_flush(None) == 0
    assert lib.fz_finish_defer(1) == 0 and lib.fz_finish_defer(-1) == 1 and lib.fz_finish_defer(0) == 1
    assert lib.fz_chunk_reduce_ld(ctypes.c_void_p(8), 4, 96, 64, ctypes.c_void_p(8), 0, None) == -4   # ld < n


def test_missing_library_fails_loudly(monkeypatch):
    from factorizer_amd import _native
    monkeypatch.setattr(_native, "_lib", None)
    monkeypatch.setattr(_native, "LIB_PATH", "/nonexistent/libfactorizer_hip.so")
    with pytest.raises(_native.NativeError):
        _native.lib()
