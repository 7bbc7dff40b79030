"""Device ops of the hot path as autograd Functions over the C ABI (include/factorizer_hip.h).

Every Function here runs ONLY the native gfx950 kernels; CPU tensors never get here (modules
route them to `composed.py`).  Backward passes are hand-written kernels as well
(SURVEY.md Appendix A for NMF).
"""
from __future__ import annotations

import ctypes
import math
import os

import torch

from . import _native as N


def _dev_guard(t: torch.Tensor):
    return torch.cuda.device(t.device)


class KernelTimer:
    """Optional per-launch timing of the native kernels with HIP events recorded on the
    stream the kernels are launched on (torch's current stream).  bench.py installs one over
    its timed region to get the dominant kernel's average launch duration and algorithmic
    bytes for the roofline line.  Every record also carries the launch's voxel-column count
    (`cols`: batch x voxels of the finest tensor it touches — which stage of the U-shape it belongs to) and its
    matrix-core flops (`flops`: 2·M·K per output column of the GEMM-shaped layers; 0 for the byte-moving kernels)."""

    def __init__(self, only=None):
        self.records = []  # (name, algorithmic_bytes, start_event, end_event, cols, flops)
        self.only = None if only is None else set(only)  # time these keys only (events cost ~1 us of stream each)

    def launch(self, name, nbytes, fn, cols=0, flops=0):
        if self.only is not None and name not in self.only:
            return fn()
        s = torch.cuda.Event(enable_timing=True)
        e = torch.cuda.Event(enable_timing=True)
        s.record()
        out = fn()
        e.record()
        self.records.append((name, nbytes, s, e, cols, flops))
        return out

    def summary(self):
        torch.cuda.synchronize()
        agg = {}
        for name, nbytes, s, e, cols, flops in self.records:
            a = agg.setdefault(name, {"calls": 0, "ms": 0.0, "bytes": 0, "flops": 0, "cols": cols})
            a["calls"] += 1
            a["ms"] += s.elapsed_time(e)
            a["bytes"] += nbytes
            a["flops"] += flops
            a["cols"] = max(a["cols"], cols)
        return agg


_timer = None


def set_timer(t):
    global _timer
    _timer = t


def _timed(name, nbytes, fn, cols=0, flops=0):
    if _timer is None:
        return fn()
    return _timer.launch(name, nbytes, fn, cols, flops)


class Geometry:
    """Static shape contract of a shifted-window matricize (operations.py:299-355, 381-415):
    channels C = h·d, spatial S_i = G_i·p_i, windows with cyclic shifts s_w."""

    def __init__(self, channels, spatial, head_dim, patch, shifts):
        self.C = int(channels)
        self.spatial = tuple(int(s) for s in spatial)
        self.d = int(head_dim)
        self.patch = tuple(int(p) for p in patch)
        self.shifts = [tuple(int(v) for v in s) for s in shifts]
        if self.C % self.d:
            raise ValueError(f"channels {self.C} not divisible by head_dim {self.d}")
        for s, p in zip(self.spatial, self.patch):
            if s % p:
                raise ValueError(f"spatial size {self.spatial} not divisible by patch size {self.patch}")
        self.h = self.C // self.d
        self.grid = tuple(s // p for s, p in zip(self.spatial, self.patch))
        self.G = math.prod(self.grid)
        self.P = math.prod(self.patch)
        self.nshift = len(self.shifts)
        # the native kernels are 3-D; lower-D problems are padded with leading unit axes
        nd = len(self.spatial)
        if nd > 3:
            raise ValueError("at most 3 spatial dims")
        pad = 3 - nd
        self.s3 = (1,) * pad + self.spatial
        self.p3 = (1,) * pad + self.patch
        self.shifts3 = [(0,) * pad + s for s in self.shifts]
        self._carr = N.shifts_array(self.shifts3)
        self._factors_ok = {}    # nmf_cf_factors_supported, by (R, T, G)

    def y_shape(self, B):
        return (self.nshift * B * self.h, self.G, self.d, self.P)


def _swm_fwd_raw(x, geo: Geometry, relu=False, div=1):
    B = x.shape[0]
    y = torch.empty(geo.y_shape(B), dtype=x.dtype, device=x.device)
    if x.dtype == torch.float32:
        es = 4
    elif x.dtype in (torch.bfloat16, torch.float16):
        es = 2
        if x.dtype == torch.float16 and (relu or div > 1):
            raise TypeError("SWMatricize with fused arithmetic: float32 or bfloat16 (float16 only moves bits)")
    else:
        raise TypeError(f"SWMatricize: unsupported dtype {x.dtype}")
    with _dev_guard(x):
        rc = _timed("swm_fwd", (1 + geo.nshift) * x.numel() * es, lambda: N.lib().fz_swm_fwd(
            x.data_ptr(), y.data_ptr(), B, geo.C, *geo.s3, geo.d, *geo.p3, geo.nshift, geo._carr, es,
            int(relu), int(div), N.stream_ptr(x)))
    N.check(rc, "fz_swm_fwd")
    return y


def _swm_inv_raw(y, geo: Geometry, average=True, gate=None):
    ad = N.act_dtype(y)   # float32, or bfloat16 storage (window sum / average in fp32, rounded once)
    if gate is not None and gate.dtype != y.dtype:
        raise TypeError("SWMatricize.inverse_forward: gate and y must have the same dtype")
    B = y.shape[0] // (geo.nshift * geo.h)
    x = torch.empty((B, geo.C, *geo.spatial), dtype=y.dtype, device=y.device)
    with _dev_guard(y):
        rc = _timed("swm_inv", (1 + geo.nshift) * x.numel() * y.element_size(), lambda: N.lib().fz_swm_inv(
            y.data_ptr(), x.data_ptr(), B, geo.C, *geo.s3, geo.d, *geo.p3, geo.nshift, geo._carr,
            int(average), N.ptr(gate), ad, N.stream_ptr(y)))
    N.check(rc, "fz_swm_inv")
    return x


class SWMForwardFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, geo):
        ctx.geo = geo
        return _swm_fwd_raw(x.contiguous(), geo)

    @staticmethod
    def backward(ctx, gy):
        if gy.dtype not in (torch.float32, torch.bfloat16):   # fp16: sum the windows in fp32
            return _swm_inv_raw(gy.float().contiguous(), ctx.geo, average=False).to(gy.dtype), None
        return _swm_inv_raw(gy.contiguous(), ctx.geo, average=False), None


class SWMInverseFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, y, geo):
        ctx.geo = geo
        return _swm_inv_raw(y.contiguous(), geo, average=True)

    @staticmethod
    def backward(ctx, gx):
        if gx.dtype == torch.float16:
            return _swm_fwd_raw(gx.float().contiguous(), ctx.geo, div=ctx.geo.nshift).to(gx.dtype), None
        return _swm_fwd_raw(gx.contiguous(), ctx.geo, div=ctx.geo.nshift), None


def swm_forward(x, geo):
    return SWMForwardFn.apply(x, geo)


def swm_inverse(y, geo):
    return SWMInverseFn.apply(y, geo)


# ---- batched NMF: three kernel families behind one binding ----------------------------------------
# family: (forward entry point, backward entry point, takes a workspace, joins the side streams first)
#   "nmf"    wave-resident (csrc/nmf.hip): M <= 32, N <= 512, rank <= 4
#   "gnmf"   split-N, matrices too wide for one wavefront (csrc/nmf_global.hip): M <= 64, rank <= 4
#   "gnmfx"  split-N (csrc/nmf_global_rank.hip): 16 <= M <= 512, rank <= 32, MU / HALS
# all three on fp32 or bf16 activation storage, with one argument list but for the workspace
_NMF_FAMILIES = {
    "nmf": ("fz_nmf_fwd", "fz_nmf_bwd", False, True),
    "gnmf": ("fz_gnmf_fwd_act", "fz_gnmf_bwd_act", True, False),
    "gnmfx": ("fz_gnmfx_fwd_act", "fz_gnmfx_bwd_act", True, False),
}


def nmf_supported(M, N_, R, T, G) -> bool:
    return bool(N.lib().fz_nmf_supported(int(M), int(N_), int(R), int(T), int(G)))


def gnmf_supported(M, N_, R, T, G) -> bool:
    return bool(N.lib().fz_gnmf_supported(int(M), int(N_), int(R), int(T), int(G)))


def gnmfx_supported(M, N_, R, T, G) -> bool:
    return bool(N.lib().fz_gnmfx_supported(int(M), int(N_), int(R), int(T), int(G)))


def _join_side_streams(t):
    """The standalone NMF kernels (csrc/nmf_r*.hip) are the only ones of the library that use scratch; a kernel with a
    private segment must not run beside the weight-gradient kernels of the second stream (results varied from run to run,
    tests/test_no_spills.py): the current stream waits for the side streams first."""
    from . import pointwise as _PW
    if _PW._SIDE:
        _PW.wait_wgrad_streams_all(t.device)


def _gnmf_ws(x, nmat, M, Nn, R, T, backward, fam="gnmf"):
    nb = getattr(N.lib(), f"fz_{fam}_workspace_bytes_act")(nmat, M, Nn, R, T, int(backward), N.act_dtype(x))
    if nb < 0:
        raise N.NativeError(f"fz_{fam}_workspace_bytes_act failed")
    return torch.empty(max(nb // 4, 1), dtype=torch.float32, device=x.device)


def _nmf_launch(fam, backward, x, R, T, head, tail):
    """one entry point of `fam`: (*head, nmat, M, N, R, T, *tail, act_dtype, [workspace,] stream)"""
    fwd_name, bwd_name, has_ws, join = _NMF_FAMILIES[fam]
    name = bwd_name if backward else fwd_name
    M, Nn = x.shape[-2:]
    nmat = x.numel() // (M * Nn)
    ws = _gnmf_ws(x, nmat, M, Nn, R, T, backward, fam) if has_ws else None
    entry = getattr(N.lib(), name)
    args = (*head, nmat, M, Nn, R, T, *tail, N.act_dtype(x), *(() if ws is None else (ws.data_ptr(),)), N.stream_ptr(x))
    with _dev_guard(x):
        if join:
            _join_side_streams(x)
        rc = _timed(f"{fam}_{'bwd' if backward else 'fwd'}_{M}x{Nn}", (3 if backward else 2) * x.numel() * x.element_size(),
                    lambda: entry(*args))
    N.check(rc, name)


def _nmf_fwd(fam, x, u0, v0, T, solver, eps, want_uv=False):
    """x fp32 or bf16 storage; y has the dtype of x, the factors are fp32 whatever the storage type of x (SURVEY.md §5:
    fp32 U/V/Gram/eps)"""
    M, Nn = x.shape[-2:]
    R = u0.shape[1]
    y = torch.empty_like(x)
    u = v = None
    if want_uv:
        u = torch.empty((*x.shape[:-2], M, R), dtype=torch.float32, device=x.device)
        v = torch.empty((*x.shape[:-2], Nn, R), dtype=torch.float32, device=x.device)
    _nmf_launch(fam, False, x, R, T, (x.data_ptr(), u0.data_ptr(), v0.data_ptr(), y.data_ptr(), N.ptr(u), N.ptr(v)),
                (N.SOLVER_ID[solver], eps))
    return y, u, v


def _nmf_bwd(fam, x, u0, v0, gy, gu, gv, T, G, solver, eps):
    gx = torch.empty_like(x)
    if gy is not None and gy.dtype != x.dtype:
        gy = gy.to(x.dtype)
    if gu is not None:
        gu, gv = gu.float().contiguous(), gv.float().contiguous()
    _nmf_launch(fam, True, x, u0.shape[1], T,
                (x.data_ptr(), u0.data_ptr(), v0.data_ptr(), N.ptr(gy), N.ptr(gu), N.ptr(gv), gx.data_ptr()),
                (G, N.SOLVER_ID[solver], eps))
    return gx


# the wave-resident family by name: the block's hand-chained node calls these (pointwise.py)
def _nmf_fwd_raw(x, u0, v0, T, solver, eps, want_uv=False):
    return _nmf_fwd("nmf", x, u0, v0, T, solver, eps, want_uv)


def _nmf_bwd_raw(x, u0, v0, gy, gu, gv, T, G, solver, eps):
    return _nmf_bwd("nmf", x, u0, v0, gy, gu, gv, T, G, solver, eps)


class NMFFn(torch.autograd.Function):
    """y = u_T v_Tᵀ after T unrolled iterations (matrix_factorization.py:514-546); `fam`: the kernel family."""

    @staticmethod
    def forward(ctx, x, u0, v0, T, G, solver, eps, fam):
        x, u0, v0 = x.contiguous(), u0.contiguous(), v0.contiguous()
        y, _, _ = _nmf_fwd(fam, x, u0, v0, T, solver, eps)
        ctx.save_for_backward(x, u0, v0)
        ctx.cfg = (T, G, solver, eps, fam)
        return y

    @staticmethod
    def backward(ctx, gy):
        x, u0, v0 = ctx.saved_tensors
        T, G, solver, eps, fam = ctx.cfg
        if G <= 0:
            return (torch.zeros_like(x), *[None] * 7)
        return (_nmf_bwd(fam, x, u0, v0, gy.contiguous(), None, None, T, G, solver, eps), *[None] * 7)


class NMFDecomposeFn(torch.autograd.Function):
    """(u_T, v_T) of the same iterations — NMF.decompose (matrix_factorization.py:514-530)."""

    @staticmethod
    def forward(ctx, x, u0, v0, T, G, solver, eps, fam):
        x, u0, v0 = x.contiguous(), u0.contiguous(), v0.contiguous()
        _, u, v = _nmf_fwd(fam, x, u0, v0, T, solver, eps, want_uv=True)
        ctx.save_for_backward(x, u0, v0)
        ctx.cfg = (T, G, solver, eps, fam)
        return u, v

    @staticmethod
    def backward(ctx, gu, gv):
        x, u0, v0 = ctx.saved_tensors
        T, G, solver, eps, fam = ctx.cfg
        if G <= 0:
            return (torch.zeros_like(x), *[None] * 7)
        gx = _nmf_bwd(fam, x, u0, v0, None, gu.contiguous(), gv.contiguous(), T, G, solver, eps)
        return (gx, *[None] * 7)


def nmf(x, u0, v0, T, G, solver, eps=1e-16):
    return NMFFn.apply(x, u0, v0, T, G, solver, eps, "nmf")


def nmf_decompose(x, u0, v0, T, G, solver, eps=1e-16):
    return NMFDecomposeFn.apply(x, u0, v0, T, G, solver, eps, "nmf")


def gnmf(x, u0, v0, T, G, solver, eps=1e-16):
    return NMFFn.apply(x, u0, v0, T, G, solver, eps, "gnmf")


def gnmf_decompose(x, u0, v0, T, G, solver, eps=1e-16):
    return NMFDecomposeFn.apply(x, u0, v0, T, G, solver, eps, "gnmf")


def gnmfx(x, u0, v0, T, G, solver, eps=1e-16):
    return NMFFn.apply(x, u0, v0, T, G, solver, eps, "gnmfx")


def gnmfx_decompose(x, u0, v0, T, G, solver, eps=1e-16):
    return NMFDecomposeFn.apply(x, u0, v0, T, G, solver, eps, "gnmfx")


# ---- fused FactMixer core on channels-first tensors ------------------------------------------
def nmf_cf_supported(geo: Geometry, R, T, G) -> bool:
    """the 8x8x8 hot-shape kernels (csrc/nmf_cf_fwd.hip, csrc/nmf_cf_bwd.hip, csrc/nmf_cf_gram.hip; asked of csrc/nmf_cf.hip)"""
    if len(geo.spatial) != 3 or any(s[2] % 2 for s in geo.shifts):  # odd W-axis shifts, 1-D / 2-D: the generic-patch kernels
        return False
    return bool(N.lib().fz_nmf_cf_supported(geo.C, *geo.spatial, geo.d, *geo.patch, int(R), int(T), int(G)))


def nmf_cf_factors_supported(geo: Geometry, R, T, G) -> bool:
    """rank 1, two windows, W % 64 == 0, W-axis shifts multiples of 4: the forward hands window 0 to window 1 as its factors
    (fz_nmf_cf_fwd_store_factors / fz_nmf_cf_fwd_from_factors, include/factorizer_hip.h) instead of as a stored tensor"""
    if len(geo.spatial) != 3:
        return False
    k = (int(R), int(T), int(G))
    ok = geo._factors_ok.get(k)         # the answer depends on (geometry, R, T, G) only: asked once, not per forward
    if ok is None:
        ok = geo._factors_ok[k] = bool(N.lib().fz_nmf_cf_factors_supported(geo.C, *geo.spatial, geo.d, *geo.patch, *k,
                                                                          geo.nshift, geo._carr))
    return ok


def nmf_cf_bwd_factors_supported(geo: Geometry, R, T, G, solver, relu_gate) -> bool:
    """where nmf_cf_factors_supported holds, for HALS behind the ReLU with every iteration graded (G = T): the backward hands
    window 0's gradient to window 1 as its factors (fz_nmf_cf_bwd_store_factors / fz_nmf_cf_bwd_from_factors,
    include/factorizer_hip.h) instead of as a stored tensor"""
    if len(geo.spatial) != 3:
        return False
    k = ("bwd", int(R), int(T), int(G), solver, bool(relu_gate))
    ok = geo._factors_ok.get(k)         # asked once per (geometry, R, T, G, solver, gate), not per backward
    if ok is None:
        ok = geo._factors_ok[k] = bool(N.lib().fz_nmf_cf_bwd_factors_supported(
            geo.C, *geo.spatial, geo.d, *geo.patch, *k[1:4], N.SOLVER_ID[solver], int(k[5]), geo.nshift, geo._carr))
    return ok


_OUTPROJ_FACTORS = os.environ.get("FZ_OUTPROJ_FACTORS", "1") != "0"   # diagnostics: 0 = the core stores its output a


def outproj_factors_supported(geo: Geometry, Hd, R, T, G, act_dtype, dropout) -> bool:
    """where nmf_cf_factors_supported holds at C = 32, hidden 64, fp32 storage, split-bf16 products, without dropout: both
    windows of the core leave their factors and the out-projection's two launches rebuild a from them (fz_mlp_chain_fac,
    fz_gemm_dw_fac, include/factorizer_hip.h) — a is never stored.  FZ_OUTPROJ_FACTORS=0: the stored tensor."""
    if not _OUTPROJ_FACTORS or len(geo.spatial) != 3:
        return False
    k = ("outproj", int(Hd), int(R), int(T), int(G), int(act_dtype), N.products(), bool(dropout))
    ok = geo._factors_ok.get(k)         # asked once per configuration, not per forward
    if ok is None:
        ok = geo._factors_ok[k] = bool(N.lib().fz_outproj_factors_supported(
            geo.C, k[1], *geo.spatial, geo.d, *geo.patch, *k[2:5], geo.nshift, geo._carr, k[5], k[6], int(k[7])))
    return ok


def core_factors(t, u0, v0, geo: Geometry, T, solver, eps):
    """The forward core of a two-window rank-1 geometry (nmf_cf_factors_supported) as the factors of BOTH windows:
    (vfac0, ufac0, vfac1, ufac1) — v one plane per head, u 8 floats per patch, per window; 1.13 passes over t per window and no
    output tensor.  factors_to_tensor forms FactCoreFn's output from them, bit for bit."""
    t, u0, v0 = t.contiguous(), u0.contiguous(), v0.contiguous()
    B = t.shape[0]
    nt = t.element_size() * t.numel()
    launch, sp, shifts = _core_launches(t, geo, N.act_dtype(t))
    nf = 4 * (t.numel() // 8)
    fac = []
    with _dev_guard(t):
        for w in range(2):
            vfac = torch.empty((B, geo.h, *geo.spatial), device=t.device, dtype=torch.float32)
            ufac = torch.empty((B * geo.h * geo.G, 8), device=t.device, dtype=torch.float32)
            N.set_tile_order(w)           # window 1 walks the tiles backwards (_native.py: set_tile_order)
            launch("fz_nmf_cf_fwd_store_factors", "nmf_cf_fwd_" + sp, nt + nf, t.data_ptr(), u0.data_ptr(), v0.data_ptr(),
                   vfac.data_ptr(), ufac.data_ptr(), B, geo.C, *geo.spatial, shifts[w], u0.shape[1], T, N.SOLVER_ID[solver], eps)
            fac += [vfac, ufac]
        N.set_tile_order(0)
    return tuple(fac)


def factors_to_tensor(fac, geo: Geometry, like):
    """a = ((0 + u0 v0ᵀ) + u1 v1ᵀ) / 2 of core_factors' result as a tensor like `like` (fz_nmf_cf_factors_to_tensor)"""
    out = torch.empty_like(like)
    B = like.shape[0]
    s0, s1 = [(N._i * 3)(*s) for s in geo.shifts3]
    with _dev_guard(like):
        rc = _timed("nmf_cf_factors_to_tensor", like.element_size() * like.numel() * 5 // 4,
                    lambda: N.lib().fz_nmf_cf_factors_to_tensor(*(f.data_ptr() for f in fac), out.data_ptr(), B, geo.C, *geo.spatial,
                                                                s0, s1, N.act_dtype(like), N.stream_ptr(like)))
    N.check(rc, "fz_nmf_cf_factors_to_tensor")
    return out


def nmf_pcf_supported(geo: Geometry, R, T, G) -> bool:
    """the generic-patch fused core (csrc/nmf_pcf.hip): head_dim 8, <= 256 voxels per patch, any shift.  1-D and 2-D tensors
    (operations.py:318-325 is N-D generic; the reference's own test models are 2-D) run as depth-1 (and height-1) volumes:
    the matricized order '(b h) (g..) d (p..)' of a (1, H, W) volume with (1, ph, pw) patches is that of the 2-D tensor."""
    if os.environ.get("FZ_NMF_PCF", "1") == "0":
        return False
    return bool(N.lib().fz_nmf_pcf_supported(geo.C, *geo.s3, geo.d, *geo.p3, int(R), int(T), int(G)))


def nmf_core_supported(geo: Geometry, R, T, G) -> bool:
    return nmf_cf_supported(geo, R, T, G) or nmf_pcf_supported(geo, R, T, G)


def _core_launches(t, geo: Geometry, ad):
    """What the launches of one FactCoreFn call share, computed once.  launch(name, key, nbytes, *args) runs the library's
    `name` under the KernelTimer and checks its status; the storage dtype and t's stream close every argument list of the
    family.  With it: the geometry suffix of the timer keys and the windows' shifts as ctypes arrays."""
    lib, cols, tail = N.lib(), t.numel() // geo.C, (ad, N.stream_ptr(t))

    def launch(name, key, nbytes, *args):
        fn = getattr(lib, name)
        N.check(_timed(key, nbytes, cols=cols, fn=lambda: fn(*args, *tail)), name)

    return launch, f"{geo.C}x" + "x".join(str(v) for v in geo.spatial), [(N._i * 3)(*s) for s in geo.shifts3]


class FactCoreFn(torch.autograd.Function):
    """a = SWMatricize⁻¹(NMF(SWMatricize(t))) for t >= 0 already activated (factorizer.py:41-50)
    without materialising the matricized tensors (csrc/nmf_cf_fwd.hip, csrc/nmf_cf_bwd.hip).  `relu_gate`: the caller's
    t is relu(z) (so t >= 0 — the library relies on it: HALS rank 1 then runs its backward in the row space,
    csrc/nmf_gram.h); the backward returns the gradient w.r.t. z (gated by [t > 0])."""

    @staticmethod
    def forward(ctx, t, u0, v0, geo, T, G, solver, eps, relu_gate):
        t = t.contiguous()
        u0, v0 = u0.contiguous(), v0.contiguous()
        B = t.shape[0]
        out = torch.empty_like(t)
        R = u0.shape[1]
        nt = t.element_size() * t.numel()         # bytes of one pass over t
        hot = nmf_cf_supported(geo, R, T, G)      # 8x8x8 patches: csrc/nmf_cf.hip; any other patch: csrc/nmf_pcf.hip
        launch, sp, shifts = _core_launches(t, geo, N.act_dtype(t))
        key = ("nmf_cf_fwd_" if hot else "nmf_pcf_fwd_") + sp
        lead = (t.data_ptr(), u0.data_ptr(), v0.data_ptr())
        dims = (B, geo.C, *geo.spatial) if hot else (B, geo.C, *geo.s3, *geo.p3)
        cfg = (R, T, N.SOLVER_ID[solver], eps)
        with _dev_guard(t):
            if hot and nmf_cf_factors_supported(geo, R, T, G):
                # window 0 leaves its rank-1 factors (v: one plane per head, u: 8 floats per patch), window 1 rebuilds u vᵀ from
                # them: 1.13 + 2.13 passes over t instead of 2 + 3, the same bits
                vfac = torch.empty((B, geo.h, *geo.spatial), device=t.device, dtype=torch.float32)
                ufac = torch.empty((B * geo.h * geo.G, 8), device=t.device, dtype=torch.float32)
                fac = (vfac.data_ptr(), ufac.data_ptr())
                nf = 4 * (t.numel() // 8)
                N.set_tile_order(0)
                launch("fz_nmf_cf_fwd_store_factors", key, nt + nf, *lead, *fac, *dims, shifts[0], *cfg)
                N.set_tile_order(1)
                launch("fz_nmf_cf_fwd_from_factors", key, 2 * nt + nf, *lead, *fac, out.data_ptr(), *dims, shifts[1], shifts[0], 2,
                       *cfg)
            else:
                name = "fz_nmf_cf_fwd" if hot else "fz_nmf_pcf_fwd"
                for w, arr in enumerate(shifts):
                    N.set_tile_order(w & 1)       # odd windows walk the tiles backwards (_native.py: set_tile_order)
                    launch(name, key, (3 if w else 2) * nt, *lead, out.data_ptr(), *dims, arr, int(w > 0),
                           geo.nshift if w == geo.nshift - 1 else 1, *cfg)
            N.set_tile_order(0)
        ctx.save_for_backward(t, u0, v0)
        ctx.cfg = (geo, T, G, solver, eps, relu_gate)
        return out

    @staticmethod
    def backward(ctx, ga):
        t, u0, v0 = ctx.saved_tensors
        geo, T, G, solver, eps, relu_gate = ctx.cfg
        if G <= 0:
            return (torch.zeros_like(t),) + (None,) * 8
        ga = ga.contiguous()
        if ga.dtype != t.dtype:
            ga = ga.to(t.dtype)
        gt = torch.empty_like(t)
        B = t.shape[0]
        R = u0.shape[1]
        nt = t.element_size() * t.numel()
        ad = N.act_dtype(t)
        hot = nmf_cf_supported(geo, R, T, G)
        launch, sp, shifts = _core_launches(t, geo, ad)
        key = ("nmf_cf_bwd_" if hot else "nmf_pcf_bwd_") + sp
        dims = (B, geo.C, *geo.spatial) if hot else (B, geo.C, *geo.s3, *geo.p3)
        with _dev_guard(t):
            if hot and nmf_cf_bwd_factors_supported(geo, R, T, G, solver, relu_gate):
                # window 0 leaves the factors of its gradient (gc: one plane per head, 88 coefficients per patch), window 1
                # rebuilds the gated value from them and its own t: 2.15 + 3.15 passes over t instead of 3 + 4
                gcfac = torch.empty((B, geo.h, *geo.spatial), device=t.device, dtype=torch.float32)
                cofac = torch.empty((B * geo.h * geo.G, 88), device=t.device, dtype=torch.float32)
                lead = (t.data_ptr(), v0.data_ptr(), ga.data_ptr(), gcfac.data_ptr(), cofac.data_ptr())
                cfg = (geo.nshift, T, G, eps)
                nf = 4 * (t.numel() // 8) + 4 * cofac.numel()
                N.set_tile_order(0)
                launch("fz_nmf_cf_bwd_store_factors", key, 2 * nt + nf, *lead, *dims, shifts[0], *cfg)
                N.set_tile_order(1)
                launch("fz_nmf_cf_bwd_from_factors", key, 3 * nt + nf, *lead, gt.data_ptr(), *dims, shifts[1], shifts[0], *cfg)
            else:
                name = "fz_nmf_cf_bwd" if hot else "fz_nmf_pcf_bwd"
                lead = (t.data_ptr(), u0.data_ptr(), v0.data_ptr(), ga.data_ptr())
                cfg = (geo.nshift, int(relu_gate), R, T, G, N.SOLVER_ID[solver], eps)
                for w, arr in enumerate(shifts):
                    N.set_tile_order(w & 1)
                    if not hot and w > 0 and N.lib().fz_nmf_pcf_bwd_prefers_separate(*geo.p3, ad):
                        # the window's gradient into its own buffer, then one coalesced add (include/factorizer_hip.h)
                        tmp = torch.empty_like(gt)
                        launch(name, key, 3 * nt, *lead, tmp.data_ptr(), *dims, arr, 0, *cfg)
                        launch("fz_act_add", "window_add_" + sp, 3 * nt, gt.data_ptr(), tmp.data_ptr(), gt.numel())
                        del tmp
                    else:
                        launch(name, key, (4 if w else 3) * nt, *lead, gt.data_ptr(), *dims, arr, int(w > 0), *cfg)
            N.set_tile_order(0)
        return (gt,) + (None,) * 8


# ---- grouped "same" cross-correlation of the Deconver family (csrc/deconv.hip) --------------
def _k3(w):
    """kernel dims of a (Bw, G, Co, Ci, *k) filter bank as (kd, kh, kw) with 2-D layers as depth 1"""
    k = tuple(w.shape[4:])
    return (1,) * (3 - len(k)) + k


def _act_ok(*ts) -> bool:
    """activation operands of the grouped-correlation kernels: all fp32 or all bf16 (csrc/deconv_kernels.h, storage type AT)"""
    return ts[0].dtype in (torch.float32, torch.bfloat16) and all(t.dtype == ts[0].dtype for t in ts)


def gcorr_supported(inp, w) -> bool:
    if not (inp.is_cuda and inp.numel() and _act_ok(inp) and w.dtype == torch.float32):
        return False
    if inp.dim() not in (4, 5) or w.dim() != inp.dim() + 2 or w.shape[0] not in (1, inp.shape[0]):
        return False
    if not N.lib().fz_gcorr_supported(int(w.shape[3]), int(w.shape[2]), *_k3(w)):
        return False
    if torch.is_grad_enabled() and inp.requires_grad:      # the input gradient is the adjoint correlation: Co ↔ Ci
        return bool(N.lib().fz_gcorr_supported(int(w.shape[2]), int(w.shape[3]), *_k3(w)))
    return True


def _gcorr_raw(inp, w, add_eps=0.0, mul_a=None, mul_b=None):
    """out = corr(inp, w) + add_eps, or mul_a ∘ mul_b / (corr + add_eps): activations fp32 or bf16 (one type), w fp32"""
    B = inp.shape[0]
    Bw, G, Co, Ci = w.shape[:4]
    sp = tuple(inp.shape[2:])
    D, H, W = (1,) * (3 - len(sp)) + sp
    if w.dtype != torch.float32 or not _act_ok(inp, *(t for t in (mul_a, mul_b) if t is not None)):
        raise TypeError("grouped correlation: activations of one type (float32 or bfloat16), float32 filters")
    out = torch.empty((B, G * Co, *sp), dtype=inp.dtype, device=inp.device)
    kd, kh, kw = _k3(w)
    with _dev_guard(inp):
        rc = _timed(f"gcorr_{Ci}->{Co}_k{kd}{kh}{kw}",
                    inp.element_size() * (inp.numel() + out.numel() * (3 if mul_a is not None else 1)),
                    lambda: N.lib().fz_gcorr_act(inp.data_ptr(), w.data_ptr(), out.data_ptr(), N.ptr(mul_a), N.ptr(mul_b), B, G,
                                                 Ci, Co, D, H, W, kd, kh, kw, int(Bw != 1), float(add_eps),
                                                 N.act_dtype(inp), N.stream_ptr(inp)))
    N.check(rc, "fz_gcorr_act")
    return out


def adjoint_filters(w):
    """(Bw, G, Co, Ci, *k) → (Bw, G, Ci, Co, *k), spatially flipped: correlation with it is the adjoint operator"""
    return torch.flip(w.transpose(2, 3), dims=tuple(range(4, w.ndim))).contiguous()


def _gcorr_wgrad_raw(inp, gout, w_shape):
    """gw (Bw, G, Co, Ci, *k), fp32, of out = corr(inp, w): fz_gcorr_wgrad_act (deterministic two-stage reduction)"""
    B = inp.shape[0]
    Bw, G, Co, Ci = w_shape[:4]
    sp = tuple(inp.shape[2:])
    D, H, W = (1,) * (3 - len(sp)) + sp
    ks = tuple(w_shape[4:])
    kd, kh, kw = (1,) * (3 - len(ks)) + ks
    if not _act_ok(inp, gout):
        raise TypeError("grouped correlation filter gradient: input and output gradient of one type (float32 or bfloat16)")
    gw = torch.empty(tuple(w_shape), dtype=torch.float32, device=inp.device)
    nb = N.lib().fz_gcorr_wgrad_workspace_bytes(B, G, Ci, Co, D, H, W, kd, kh, kw)
    ws = torch.empty(max(nb // 4, 1), dtype=torch.float32, device=inp.device)
    with _dev_guard(inp):
        rc = _timed(f"gcorr_wgrad_{Ci}->{Co}_k{kd}{kh}{kw}", inp.element_size() * (inp.numel() + gout.numel()),
                    lambda: N.lib().fz_gcorr_wgrad_act(inp.data_ptr(), gout.data_ptr(), gw.data_ptr(), ws.data_ptr(), B, G, Ci,
                                                       Co, D, H, W, kd, kh, kw, int(Bw != 1), N.act_dtype(inp),
                                                       N.stream_ptr(inp)))
    N.check(rc, "fz_gcorr_wgrad_act")
    return gw


def _gcorr_mu_bwd_raw(r, wT, g, s, num, eps, want):
    """(ds, dnum, dden) of s' = s ∘ num / (corr(r, wT) + eps) from g = dL/ds' in one launch (fz_gcorr_mu_bwd: the denominator
    is recomputed, not read); `want` = (ds?, dnum?, dden?) — an output that is not wanted is None and not written"""
    flags = [bool(f) for f in want]
    B = r.shape[0]
    Bw, G, Co, Ci = wT.shape[:4]
    sp = tuple(r.shape[2:])
    D, H, W = (1,) * (3 - len(sp)) + sp
    if wT.dtype != torch.float32 or not _act_ok(r, g, s, num):
        raise TypeError("multiplicative-update backward: activations of one type (float32 or bfloat16), float32 filters")
    outs = [torch.empty_like(s) if f else None for f in flags]
    kd, kh, kw = _k3(wT)
    with _dev_guard(r):
        rc = _timed(f"gcorr_mu_bwd_{Ci}->{Co}_k{kd}{kh}{kw}", r.element_size() * (r.numel() + s.numel() * (3 + sum(flags))),
                    lambda: N.lib().fz_gcorr_mu_bwd(r.data_ptr(), wT.data_ptr(), g.data_ptr(), s.data_ptr(), num.data_ptr(),
                                                    N.ptr(outs[0]), N.ptr(outs[1]), N.ptr(outs[2]), B, G, Ci, Co, D, H, W,
                                                    kd, kh, kw, int(Bw != 1), float(eps), N.act_dtype(r), N.stream_ptr(r)))
    N.check(rc, "fz_gcorr_mu_bwd")
    return outs


class GCorrFn(torch.autograd.Function):
    """out = corr(inp, w) + add_eps: native forward, input gradient (the adjoint correlation) and filter gradient
    (the lag-correlation of inp with the output gradient, fz_gcorr_wgrad).  Activations and their gradients in the
    storage type of `inp` (fp32 or bf16), the filter gradient in fp32."""

    @staticmethod
    def forward(ctx, inp, w, add_eps):
        inp, w = inp.contiguous(), w.contiguous()
        ctx.save_for_backward(inp, w)
        return _gcorr_raw(inp, w, add_eps)

    @staticmethod
    def backward(ctx, gout):
        inp, w = ctx.saved_tensors
        gout = gout.contiguous()
        ginp = gw = None
        if ctx.needs_input_grad[0]:
            ginp = _gcorr_raw(gout, adjoint_filters(w))
        if ctx.needs_input_grad[1]:
            gw = _gcorr_wgrad_raw(inp, gout, w.shape)
        return ginp, gw, None


class GCorrMuFn(torch.autograd.Function):
    """s' = s ∘ num / (corr(r, wT) + eps) as ONE node: the forward is the fused-epilogue launch, the backward recomputes the
    denominator in the kernel (fz_gcorr_mu_bwd) — saved are s, num, r and wT, which exist anyway; den, s ∘ num and the
    quotient are never stored.  From dden the gradients of r (the adjoint correlation) and of wT (the filter gradient) follow.
    On bf16 storage every tensor that reaches memory is rounded once."""

    @staticmethod
    def forward(ctx, s, num, r, wT, eps):
        s, num, r, wT = s.contiguous(), num.contiguous(), r.contiguous(), wT.contiguous()
        ctx.save_for_backward(s, num, r, wT)
        ctx.eps = float(eps)
        return _gcorr_raw(r, wT, eps, s, num)

    @staticmethod
    def backward(ctx, g):
        s, num, r, wT = ctx.saved_tensors
        need = ctx.needs_input_grad
        ds, dnum, dden = _gcorr_mu_bwd_raw(r, wT, g.contiguous(), s, num, ctx.eps,
                                           (need[0], need[1], need[2] or need[3]))
        dr = _gcorr_raw(dden, adjoint_filters(wT)) if need[2] else None
        dwT = _gcorr_wgrad_raw(r, dden, wT.shape) if need[3] else None
        return ds, dnum, dr, dwT, None


class LagCorrFn(torch.autograd.Function):
    """L[b, g, c, k, τ] = Σ_v x[b, g·C + c, v] · s[b, g·K + k, v + τ − p] — the lag correlations of the filter update
    (deconvolution.py:43-50 `sconv`, :150-156 `update_h`).  The same reduction as the filter gradient of the grouped
    correlation (fz_gcorr_wgrad); its own gradients are two grouped correlations with gL as per-sample filters.
    s and x in one storage type (fp32 or bf16); L and gL are fp32."""

    @staticmethod
    def forward(ctx, s, x, G, ksize):
        s, x = s.contiguous(), x.contiguous()
        ctx.save_for_backward(s, x)
        B = s.shape[0]
        return _gcorr_wgrad_raw(s, x, (B, G, x.shape[1] // G, s.shape[1] // G, *ksize))

    @staticmethod
    def backward(ctx, gL):
        s, x = ctx.saved_tensors
        gL = gL.float().contiguous()
        gs = gx = None
        if ctx.needs_input_grad[0]:
            gs = _gcorr_raw(x, adjoint_filters(gL))
        if ctx.needs_input_grad[1]:
            gx = _gcorr_raw(s, gL)
        return gs, gx, None, None


def lag_corr_supported(s, x, G, ksize) -> bool:
    if not (s.is_cuda and s.numel() and _act_ok(s, x) and s.dim() in (4, 5)):
        return False
    K, C = s.shape[1] // G, x.shape[1] // G
    k3 = (1,) * (3 - len(ksize)) + tuple(int(k) for k in ksize)
    return bool(N.lib().fz_gcorr_supported(K, C, *k3)) and bool(N.lib().fz_gcorr_supported(C, K, *k3))


def lag_corr(s, x, G, ksize):
    return LagCorrFn.apply(s, x, G, tuple(int(k) for k in ksize))


def gcorr(inp, w, add_eps=0.0):
    return GCorrFn.apply(inp, w, add_eps)


def gcorr_mu_update(s, num, r, wT, eps):
    """s ∘ num / (corr(r, wT) + eps) in one launch — for iterations that carry no gradient (inference, or the
    leading `num_iters − num_grad_iters` iterations of deconvolution.py:158-166)."""
    return _gcorr_raw(r.contiguous(), wT.contiguous(), eps, s.contiguous(), num.contiguous())


def gcorr_mu_update_graded(s, num, r, wT, eps):
    """the same update as an autograd node (GCorrMuFn): gradients with respect to s, num, r and wT, two stored tensors
    (the result and, in the backward, dden) where the composed expression stores five"""
    return GCorrMuFn.apply(s, num, r, wT, eps)


# ---- block dropout masks (csrc/dropout.hip) ---------------------------------------------------------------------------
def dropout_seed(device):
    """THE seed draw of one FactorizerBlock forward with live dropout: an int64 tensor (1,) on `device`, drawn by a torch op from
    that device's default generator — no host sync, `torch.manual_seed` / `torch.cuda.manual_seed` make runs repeat, and
    consecutive forwards get new masks.  FactorizerBlockFn.forward calls it before anything else in the block touches the
    generator, so `torch.cuda.manual_seed(s); dropout_seed(dev)` rebuilds the seed (and, through `dropout_keep_bits`, the
    masks) of a forward run right after the same `torch.cuda.manual_seed(s)`."""
    return torch.randint(0, 2 ** 62, (1,), device=device, dtype=torch.int64)


def dropout_keep_bits(seed, site, B, ch, V, p):
    """keep bits of dropout site `site` (0: fact.dropout, 1: mlp.block[2], 2: mlp.block[4]) for a (B, ch, V) tensor: int32
    tensor (B, ch, ceil(V / 32)) holding the uint32 words of fz_dropout_keep_bits (bit v & 31 of word v >> 5)."""
    lib = N.lib()
    nw = (int(V) + 31) // 32
    out = torch.empty((B, ch, nw), dtype=torch.int32, device=seed.device)
    with _dev_guard(seed):
        rc = _timed(f"dropout_bits_{ch}", 4 * out.numel(), lambda: lib.fz_dropout_keep_bits(
            seed.data_ptr(), int(site), int(B), int(ch), int(V), float(p), out.data_ptr(), N.stream_ptr(seed)), cols=B * V)
    N.check(rc, "fz_dropout_keep_bits")
    return out


def dropout_apply(kind, bits, p, t, aux=None):
    """y = aux + keep·s·t (N.DROP_RES; aux None: keep·s·t), keep·s·gelu(t) (N.DROP_GELU) or keep·s·t·gelu'(aux)
    (N.DROP_GELU_BWD) with s = 1 / (1 − p): one pass of fz_dropout_apply over a (B, ch, ...) activation."""
    B, ch = t.shape[:2]
    V = t[0, 0].numel() if t.numel() else math.prod(t.shape[2:])
    y = torch.empty_like(t)
    n = 2 + (aux is not None)
    with _dev_guard(t):
        rc = _timed(f"dropout_apply{kind}_{ch}", n * t.element_size() * t.numel(), lambda: N.lib().fz_dropout_apply(
            int(kind), bits.data_ptr(), float(p), t.data_ptr(), N.ptr(aux), y.data_ptr(), B, ch, V, N.act_dtype(t),
            N.stream_ptr(t)), cols=B * V)
    N.check(rc, "fz_dropout_apply")
    return y


# ---- segmentation metrics (csrc/segmetric.hip) ------------------------------------------------------------------------
_SEG_KIND = {torch.float32: N.SEG_F32, torch.bfloat16: N.SEG_BF16, torch.uint8: N.SEG_U8, torch.bool: N.SEG_U8}


def seg_kind_ok(t) -> bool:
    """the element kinds fz_seg_counts reads: fp32 / bf16 values, uint8 / bool masks"""
    return t.dtype in _SEG_KIND


def seg_counts(pred, label, bound, want_mask=False, want_counts=True):
    """One pass of fz_seg_counts over `pred` (B, C, *S) — logits of a native float kind (foreground iff x >= bound) or a
    one-byte mask (foreground iff non-zero) — and the optional `label` (non-zero counts).  Returns (counts, mask): int64
    (B, C, 3) = {|P ∧ Y|, |P|, |Y|} or None, uint8 mask shaped like `pred` or None."""
    B, C = pred.shape[:2]
    planes = B * C
    V = pred.numel() // planes
    lib = N.lib()
    ws = torch.empty(int(lib.fz_seg_counts_workspace_bytes(planes, V)) // 4, dtype=torch.int32, device=pred.device)
    counts = torch.empty((B, C, 3), dtype=torch.int64, device=pred.device) if want_counts else None
    mask = torch.empty(pred.shape, dtype=torch.uint8, device=pred.device) if want_mask else None
    nbytes = pred.numel() * pred.element_size() + (label.numel() * label.element_size() if label is not None else 0) + \
        (pred.numel() if want_mask else 0)
    with _dev_guard(pred):
        rc = _timed("seg_counts", nbytes, lambda: lib.fz_seg_counts(
            pred.data_ptr(), _SEG_KIND[pred.dtype], N.ptr(label), _SEG_KIND[label.dtype] if label is not None else 0,
            float(bound), N.ptr(mask), ws.data_ptr(), N.ptr(counts), planes, V, N.stream_ptr(pred)), cols=B * V)
    N.check(rc, "fz_seg_counts")
    return counts, mask


LABEL_KIND = {torch.uint8: N.LABEL_U8, torch.int64: N.LABEL_I64, torch.float32: N.LABEL_F32}


def label_kind_ok(t) -> bool:
    """a class-index label map the kernels read in its own type: uint8 / int64 / fp32, contiguous, 16-byte aligned"""
    return t.dtype in LABEL_KIND and t.is_contiguous() and t.data_ptr() % 16 == 0


def seg_argmax(pred, label, num_classes, want_map=False, want_onehot=False, want_counts=False):
    """One pass of fz_seg_argmax over `pred` — logits (B, C, *S) of a native float kind, or a uint8 label map (B, 1, *S) of
    `num_classes` classes — and the optional class-index `label` (B, 1, *S).  Returns (map, onehot, counts): uint8
    (B, 1, *S), uint8 (B, C, *S), int64 (B, C, 3) = {|P = c ∧ Y = c|, |P = c|, |Y = c|}, each None unless asked for."""
    B, C = pred.shape[0], int(num_classes)
    sp = tuple(pred.shape[2:])
    V = math.prod(sp)
    lib = N.lib()
    dev = pred.device
    cmap = torch.empty((B, 1, *sp), dtype=torch.uint8, device=dev) if want_map else None
    onehot = torch.empty((B, C, *sp), dtype=torch.uint8, device=dev) if want_onehot else None
    counts = torch.empty((B, C, 3), dtype=torch.int64, device=dev) if want_counts else None
    ws = torch.empty(int(lib.fz_seg_argmax_workspace_bytes(B, C, V)) // 4, dtype=torch.int32, device=dev) if want_counts else None
    nbytes = pred.numel() * pred.element_size() + (label.numel() * label.element_size() if label is not None else 0) + \
        (B * V if want_map else 0) + (B * C * V if want_onehot else 0)
    with _dev_guard(pred):
        rc = _timed("seg_argmax", nbytes, lambda: lib.fz_seg_argmax(
            pred.data_ptr(), _SEG_KIND[pred.dtype], N.ptr(label), LABEL_KIND[label.dtype] if label is not None else 0,
            N.ptr(cmap), N.ptr(onehot), N.ptr(ws), N.ptr(counts), B, C, V, N.stream_ptr(pred)), cols=B * V)
    N.check(rc, "fz_seg_argmax")
    return cmap, onehot, counts


def mask_edges(mask):
    """fz_mask_edges over a one-byte mask (B, C, *S) with 1 to 3 spatial axes: (edges uint8 like mask, counts int64 (B, C))"""
    B, C = mask.shape[:2]
    sp = tuple(mask.shape[2:])
    nd = len(sp)
    d3 = (1,) * (3 - nd) + sp
    edges = torch.empty(mask.shape, dtype=torch.uint8, device=mask.device)
    counts = torch.empty((B, C), dtype=torch.int64, device=mask.device)
    with _dev_guard(mask):
        rc = _timed("mask_edges", 2 * mask.numel(), lambda: N.lib().fz_mask_edges(
            mask.data_ptr(), edges.data_ptr(), counts.data_ptr(), B * C, nd, *d3, N.stream_ptr(mask)),
            cols=B * math.prod(sp))
    N.check(rc, "fz_mask_edges")
    return edges, counts


def edge_min_dist2(q, t, w):
    """fz_edge_min_dist2: q (nq, 4), t (nt, 4) fp32 coordinate lists (nq, nt >= 1), w = the three squared spacings; returns
    the fp32 (nq,) minimum over t of Σ_k w_k (q_k − t_k)²"""
    nq, nt = q.shape[0], t.shape[0]
    lib = N.lib()
    out = torch.empty(nq, dtype=torch.float32, device=q.device)
    nws = int(lib.fz_edge_min_dist2_workspace_bytes(nq, nt))
    ws = torch.empty(nws // 4, dtype=torch.float32, device=q.device) if nws else None
    with _dev_guard(q):
        rc = _timed("edge_min_dist2", 16 * (nq + nt) + 4 * nq, lambda: lib.fz_edge_min_dist2(
            q.data_ptr(), nq, t.data_ptr(), nt, float(w[0]), float(w[1]), float(w[2]), out.data_ptr(), N.ptr(ws),
            N.stream_ptr(q)), cols=nq)
    N.check(rc, "fz_edge_min_dist2")
    return out


# ---- batch augmentations (csrc/augment.hip) ---------------------------------------------------------------------------
def aug_noise_field(seed, B, C, V):
    """fz_aug_noise_field: fp32 (B, C, V) normals of the int64 device tensor `seed` (factorizer_amd/augment.py)"""
    out = torch.empty((B, C, V), dtype=torch.float32, device=seed.device)
    with _dev_guard(seed):
        rc = _timed("aug_noise_field", 4 * out.numel(), lambda: N.lib().fz_aug_noise_field(
            out.data_ptr(), seed.data_ptr(), int(B), int(C), int(V), N.stream_ptr(seed)), cols=B * V)
    N.check(rc, "fz_aug_noise_field")
    return out


def aug_apply(image, label, records, table_words, ns, seed):
    """fz_aug_resample over the whole batch, then fz_aug_smooth over its `ns` smoothing samples (ns = 0: no second launch).
    `records`: the device copy of augment._records — `table_words` fp32 words of per-sample records, the int32 sample list of
    the smoothing slots behind them.  image (B, C, *S) fp32 / bf16 and label (B, L, *S) uint8 / bool, contiguous, either may
    be None; seed: int64 device tensor or None (no noise).  Returns new (image, label)."""
    lib = N.lib()
    ref = image if image is not None else label
    B = ref.shape[0]
    sp = tuple(ref.shape[2:])
    nd = len(sp)
    d3 = (1,) * (3 - nd) + sp
    V = math.prod(sp)
    C = image.shape[1] if image is not None else 0
    L = label.shape[1] if label is not None else 0
    if int(lib.fz_aug_record_floats()) * B != table_words:
        raise N.NativeError("the record layout of augment.py and of the library differ")
    out_i = torch.empty_like(image) if image is not None else None
    out_l = torch.empty_like(label) if label is not None else None
    ns = ns if image is not None else 0
    ws = torch.empty((ns, C, V), dtype=torch.float32, device=ref.device) if ns else None
    dt = N.act_dtype(image) if image is not None else N.STORE_F32
    es = image.element_size() if image is not None else 0
    with _dev_guard(ref):
        rc = _timed("aug_resample", B * V * (2 * C * es + 2 * L), lambda: lib.fz_aug_resample(
            N.ptr(image), N.ptr(out_i), dt, C, N.ptr(label), N.ptr(out_l), L, records.data_ptr(), N.ptr(seed), N.ptr(ws), ns,
            B, nd, *d3, N.stream_ptr(ref)), cols=B * V)
        N.check(rc, "fz_aug_resample")
        if ns:
            rc = _timed("aug_smooth", ns * C * V * (4 + es), lambda: lib.fz_aug_smooth(
                ws.data_ptr(), out_i.data_ptr(), dt, C, records.data_ptr(), records.data_ptr() + 4 * table_words, ns, B, nd,
                *d3, N.stream_ptr(ref)), cols=ns * V)
            N.check(rc, "fz_aug_smooth")
    return out_i, out_l


def aug_crop_apply(buf, source_words, table_words, ns, seed, roi, C, L, image_dtype, label_dtype):
    """fz_aug_crop_resample over a batch whose samples are cut from their own source volumes (csrc/aug_crop.hip), then
    fz_aug_smooth over its `ns` smoothing samples.  `buf`: the device copy of augment._crop_table — `source_words` fp32 words
    that hold the int64 source table, then `table_words` words of records, then the int32 sample list.  roi: the output's
    spatial shape; C / L planes of image_dtype / label_dtype per sample (0: none); seed as in aug_apply.  The caller keeps the
    source tensors alive until this returns.  Returns new (image (B, C, *roi), label (B, L, *roi))."""
    lib = N.lib()
    roi = tuple(int(r) for r in roi)
    nd = len(roi)
    d3 = (1,) * (3 - nd) + roi
    V = math.prod(roi)
    B = table_words // int(lib.fz_aug_record_floats())
    if int(lib.fz_aug_record_floats()) * B != table_words or 2 * int(lib.fz_aug_source_words()) * B != source_words:
        raise N.NativeError("the record or source-table layout of augment.py and of the library differ")
    out_i = torch.empty((B, C) + roi, dtype=image_dtype, device=buf.device) if C else None
    out_l = torch.empty((B, L) + roi, dtype=label_dtype, device=buf.device) if L else None
    ns = ns if C else 0
    ws = torch.empty((ns, C, V), dtype=torch.float32, device=buf.device) if ns else None
    dt = N.act_dtype(out_i) if C else N.STORE_F32
    es = out_i.element_size() if C else 0
    records = buf.data_ptr() + 4 * source_words
    with _dev_guard(buf):
        rc = _timed("aug_crop_resample", B * V * (2 * C * es + 2 * L), lambda: lib.fz_aug_crop_resample(
            buf.data_ptr(), N.ptr(out_i), dt, C, N.ptr(out_l), L, records, N.ptr(seed), N.ptr(ws), ns, B, nd, *d3,
            N.stream_ptr(buf)), cols=B * V)
        N.check(rc, "fz_aug_crop_resample")
        if ns:
            rc = _timed("aug_smooth", ns * C * V * (4 + es), lambda: lib.fz_aug_smooth(
                ws.data_ptr(), out_i.data_ptr(), dt, C, records, records + 4 * table_words, ns, B, nd, *d3,
                N.stream_ptr(buf)), cols=ns * V)
            N.check(rc, "fz_aug_smooth")
    return out_i, out_l


# ---- volume preparation and prediction restore (csrc/volprep.hip) -----------------------------------------------------
_VOL_KIND = {torch.float32: N.VOL_F32, torch.bfloat16: N.VOL_BF16, torch.uint8: N.VOL_U8, torch.int16: N.VOL_I16}


def vol_kind_ok(role, dtype) -> bool:
    """fz_vol_kind_ok: does the role (N.VOL_IMAGE_IN, ...) take tensors of this dtype natively"""
    return dtype in _VOL_KIND and bool(N.lib().fz_vol_kind_ok(role, _VOL_KIND[dtype]))


def vol_geom(size, start, end, pad, out):
    """fz_vol_geom of 1 to 3 spatial axes, lifted to three with leading unit axes"""
    nd = len(size)
    g = N.VolGeom()
    g.nd = nd
    lift = 3 - nd
    for name, vals, fill in (("size", size, 1), ("start", start, 0), ("end", end, 1), ("pad", pad, 0), ("out", out, 1)):
        arr = getattr(g, name)
        for a in range(3):
            arr[a] = fill if a < lift else int(vals[a - lift])
    return g


def vol_bbox(image):
    """fz_vol_bbox over image (C, *S), fp32 or int16, contiguous: int32 device tensor {min z, y, x, max z, y, x} of the lifted
    axes over the voxels where any channel is > 0 (min > max: none)"""
    C = image.shape[0]
    sp = tuple(image.shape[1:])
    nd = len(sp)
    d3 = (1,) * (3 - nd) + sp
    box = torch.empty(6, dtype=torch.int32, device=image.device)
    with _dev_guard(image):
        rc = _timed("vol_bbox", image.numel() * image.element_size(), lambda: N.lib().fz_vol_bbox(
            image.data_ptr(), _VOL_KIND[image.dtype], C, nd, *d3, box.data_ptr(), N.stream_ptr(image)), cols=math.prod(sp))
    N.check(rc, "fz_vol_bbox")
    return box


def vol_prepare(image, label, geom, nonzero, channel_wise, classes, out_dtype):
    """fz_vol_stats + fz_vol_write: image (C, *S) fp32 / int16 and the optional label — a class map (*S) uint8 / int16 with
    `classes` (a sequence of id sequences), or (L, *S) uint8 with classes None — through `geom` (vol_geom).  Returns
    (image (C, *out) of out_dtype, label (K, *out) uint8 or None, mean (C,), std (C,))."""
    lib = N.lib()
    C = image.shape[0]
    nd = geom.nd
    out_sp = tuple(geom.out[3 - nd:3])
    box_sp = tuple(geom.end[a] - geom.start[a] for a in range(3 - nd, 3))
    dev = image.device
    nws = int(lib.fz_vol_workspace_bytes(C, ctypes.byref(geom)))
    if nws < 0:
        # let the entry point say what is wrong with the geometry
        N.check(lib.fz_vol_stats(image.data_ptr(), _VOL_KIND[image.dtype], C, ctypes.byref(geom), int(nonzero),
                                 int(channel_wise), None, N.stream_ptr(image)), "fz_vol_stats")
        raise N.NativeError("fz_vol_workspace_bytes refused the geometry")
    ws = torch.empty(nws // 8, dtype=torch.float64, device=dev)
    out = torch.empty((C,) + out_sp, dtype=out_dtype, device=dev)
    mean = torch.empty(C, dtype=torch.float32, device=dev)
    std = torch.empty(C, dtype=torch.float32, device=dev)
    ids = counts = None
    lab_out, lch, ncls, lkind = None, 0, 0, 0
    if label is not None:
        lkind = _VOL_KIND[label.dtype]
        if classes is not None:
            flat = [int(v) for cs in classes for v in cs]
            ids = (ctypes.c_int * max(1, len(flat)))(*flat)
            counts = (ctypes.c_int * len(classes))(*[len(cs) for cs in classes])
            ncls = len(classes)
        else:
            lch = label.shape[0]
        lab_out = torch.empty((ncls or lch,) + out_sp, dtype=torch.uint8, device=dev)
    es = image.element_size()
    nbox = C * math.prod(box_sp)
    with _dev_guard(image):
        rc = _timed("vol_stats", 2 * nbox * es, lambda: lib.fz_vol_stats(
            image.data_ptr(), _VOL_KIND[image.dtype], C, ctypes.byref(geom), int(nonzero), int(channel_wise), ws.data_ptr(),
            N.stream_ptr(image)), cols=math.prod(box_sp))
        N.check(rc, "fz_vol_stats")
        nbytes = nbox * es + out.numel() * out.element_size() + \
            (0 if label is None else (lch or 1) * math.prod(box_sp) * label.element_size() + lab_out.numel())
        rc = _timed("vol_write", nbytes, lambda: lib.fz_vol_write(
            image.data_ptr(), _VOL_KIND[image.dtype], out.data_ptr(), _VOL_KIND[out_dtype], C, N.ptr(label), lkind, lch, ids,
            counts, ncls, N.ptr(lab_out), ctypes.byref(geom), int(nonzero), int(channel_wise), ws.data_ptr(), mean.data_ptr(),
            std.data_ptr(), N.stream_ptr(image)), cols=math.prod(out_sp))
        N.check(rc, "fz_vol_write")
    return out, lab_out, mean, std


def vol_restore(logits, geom, bound, label_values):
    """fz_vol_restore: logits = 1 to 8 contiguous (C, *out) tensors of one native kind; uint8 mask (C, *size), or with
    label_values (C byte values) the label map (*size)"""
    x = logits[0]
    C, K = x.shape[0], len(logits)
    nd = geom.nd
    size = tuple(geom.size[3 - nd:3])
    table = (ctypes.c_void_p * K)(*[t.data_ptr() for t in logits])
    vals = None if label_values is None else (ctypes.c_ubyte * C)(*[int(v) for v in label_values])
    res = torch.empty(size if label_values is not None else (C,) + size, dtype=torch.uint8, device=x.device)
    box = math.prod(geom.end[a] - geom.start[a] for a in range(3))
    with _dev_guard(x):
        rc = _timed("vol_restore", K * C * box * x.element_size() + res.numel(), lambda: N.lib().fz_vol_restore(
            table, K, _VOL_KIND[x.dtype], C, ctypes.byref(geom), float(bound), vals, res.data_ptr(), N.stream_ptr(x)),
            cols=math.prod(size))
    N.check(rc, "fz_vol_restore")
    return res


# ---- resampling to the recipe's voxel spacing and back (csrc/respace.hip) ---------------------------------------------
def respace_geom(src_size, src_axis, flip, scale, inv_scale, res_size, pad, out, orig_size, box_start):
    """fz_respace_geom of 1 to 3 spatial axes, lifted to three with leading unit axes (a lifted axis reads itself)"""
    nd = len(src_size)
    g = N.RespaceGeom()
    g.nd = nd
    lift = 3 - nd
    for name, vals, fill in (("src_size", src_size, 1), ("flip", flip, 0), ("res_size", res_size, 1), ("pad", pad, 0),
                             ("out", out, 1), ("orig_size", orig_size, 1), ("box_start", box_start, 0)):
        arr = getattr(g, name)
        for a in range(3):
            arr[a] = fill if a < lift else int(vals[a - lift])
    for a in range(3):
        g.src_axis[a] = a if a < lift else int(src_axis[a - lift]) + lift
        g.scale[a] = 1.0 if a < lift else float(scale[a - lift])
        g.inv_scale[a] = 1.0 if a < lift else float(inv_scale[a - lift])
    return g


def vol_respace(image, label, geom, mode, out_dtype):
    """fz_vol_respace: image (C, *src) fp32 and the optional label (L, *src) uint8, both contiguous, through `geom`
    (respace_geom) -> (image (C, *out) of out_dtype, label (L, *out) uint8 or None)"""
    C = image.shape[0]
    nd = geom.nd
    out_sp = tuple(geom.out[3 - nd:3])
    out = torch.empty((C,) + out_sp, dtype=out_dtype, device=image.device)
    L = 0 if label is None else label.shape[0]
    lab_out = None if label is None else torch.empty((L,) + out_sp, dtype=torch.uint8, device=image.device)
    src = math.prod(geom.src_size[a] for a in range(3))
    nbytes = C * src * 4 + out.numel() * out.element_size() + L * (src + math.prod(out_sp))   # every element once
    with _dev_guard(image):
        rc = _timed("vol_respace", nbytes, lambda: N.lib().fz_vol_respace(
            image.data_ptr(), C, out.data_ptr(), _VOL_KIND[out_dtype], N.ptr(label), L, N.ptr(lab_out), ctypes.byref(geom),
            int(mode), N.stream_ptr(image)), cols=math.prod(out_sp))
    N.check(rc, "fz_vol_respace")
    return out, lab_out


def vol_unspace(logits, geom, sigmoid, threshold):
    """fz_vol_unspace: logits = 1 to 8 contiguous (C, *out) tensors of one native kind -> uint8 mask (C, *orig_size) of
    `value >= threshold`, or with threshold None the fp32 values"""
    x = logits[0]
    C, K = x.shape[0], len(logits)
    nd = geom.nd
    size = tuple(geom.orig_size[3 - nd:3])
    table = (ctypes.c_void_p * K)(*[t.data_ptr() for t in logits])
    res = torch.empty((C,) + size, dtype=torch.float32 if threshold is None else torch.uint8, device=x.device)
    spaced = math.prod(geom.res_size[a] for a in range(3))
    with _dev_guard(x):
        rc = _timed("vol_unspace", K * C * spaced * x.element_size() + res.numel() * res.element_size(),
                    lambda: N.lib().fz_vol_unspace(table, K, _VOL_KIND[x.dtype], C, ctypes.byref(geom), int(bool(sigmoid)),
                                                   int(threshold is not None), float(threshold or 0.0), res.data_ptr(),
                                                   N.stream_ptr(x)), cols=math.prod(size))
    N.check(rc, "fz_vol_unspace")
    return res
