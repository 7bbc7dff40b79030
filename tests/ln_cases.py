"""Oracle, inputs, bounds and mutants of the channels-first LayerNorm tests (tests/test_layernorm_cpu.py: the oracle, the
bounds and the mutants on the CPU; tests/test_gpu_layernorm.py: csrc/ln.hip on the device).

Oracle (float64, closed forms, evaluated chunk-wise over the voxels; tensors are (B, C, V)):
  forward   mu = mean_c x, rs = (var_c x + eps)^-1/2 (biased variance), y = (x - mu) rs γ + β
  backward  of (gl, x, stats, γ, gadd) with stats = the (B, 2, V) tensor (mu, rs) the kernel reads:
            n = (x - mu) rs, a = gl γ, gx = rs (a - mean_c a - n mean_c(a n)) [+ gadd], gγ = Σ_{b,v} gl n, gβ = Σ_{b,v} gl

Exact inputs (`exact_bwd`, `exact_fwd`): dyadic data for which every intermediate and every partial sum of these formulas is
a float32 number, so the float64 answer is the only correct one, bit for bit, whatever the summation order or FMA contraction:
x integers in [-3, 3], mu in {-1, 0, 1}, rs in {1/2, 1, 2}, gl integers in [-2, 2], γ in ±{1/2, 1, 2}, gadd = k + 128 s with
k an integer in [-4, 4] and s in {-1, 0, 1} (all of them bf16 numbers; the halves that rs·(...) leaves next to ±128 are exact
ties of the bf16 store: nearest-even, half-away and truncation all differ on them).  C a power of two: 1/C is one, the full
formula is exact.  Any other C: the channels come in pairs that share x and carry opposite gl γ (an odd last channel has
gl = 0), so both per-voxel means are exactly 0.  Σ|terms| of gγ, gβ is returned; below 2^22 every partial sum of the halves
is exact in any order.

Bounds (a priori, element-wise, first order in u = 2^-24, times SLACK for the higher orders; nothing is tuned on a device).
Any summation tree over C terms errs by at most (C - 1) u Σ|terms| (the sequential sum is the worst case, and the one the
forward and the C < 64 backward use); one more u per element-wise operation; a bf16 store (8 significand bits, nearest-even)
adds half a unit in the last place of the stored value, `half_ulp_bf16`: at most 2^-8 |ref| (a truncating store errs by up to a
whole unit, 2^-7 |ref|; 2^-9 |ref| would be half a unit of a 9-bit format, and the fp32 emulation breaks it).
  forward   s = Σ x: (C - 1) u S1, S1 = Σ_c|x|.  mu = s·fl(1/C): dmu = (C - 1) u S1 / C + 2 u |mu|.
            q = Σ (x - mu')^2 around the computed mean mu' = mu + δ: Σ (x - mu')^2 = Q + C δ^2 exactly (Σ (x - mu) = 0), each
            term carries 3 u (difference, square), the sum (C - 1) u: dq = (C + 2) u Q + C dmu^2.  (C dmu^2 is second order
            in u but first in C |mean| / std: it is what a sequential channel sum costs on data far from zero, and it stays in.)
            v = q fl(1/C) + eps: dv = dq / C + 3 u v.  rs = 1 / sqrt(v), both correctly rounded to within 2 u: drs / rs =
            dv / (2 v) + 4 u.
            y = (x - mu') rs' γ + β: dy = |γ| rs (u |x - mu| + dmu) + |γ n| (drs / rs + 2 u) + u |y| [+ half_ulp_bf16]
  backward  (mu, rs are inputs: exact)  n' = (x - mu) rs: 2 u |n|.  a' = gl γ: u |a|.
            m1 = Σ a / C: dm1 = (C + 2) u A1 / C, A1 = Σ_c|a|.  m2 = Σ a n / C: each term 4 u, dm2 = (C + 5) u A2 / C.
            gx = rs (a' - m1 - n' m2) + gadd: dgx = rs (dm1 + |n| dm2 + 6 u (|a| + |m1| + |n m2|)) + u |gx| [+ half_ulp_bf16]
            gγ, gβ: the reduction tree of the path (`param_depth`): 4 voxels in a lane (2 levels), the lanes (wave_sum: 6; the
            16 lanes of a SUB = 4 sub-slice: 4), for C < 64 the grid-stride iterations in a lane and 2 levels across the 4 waves,
            then the row reduction (csrc/finish.h fin_rows_body: 8 strided sequential sums and 3 levels; two stages of it
            above 512 rows).  With depth D: dgβ = D u Σ|gl|, dgγ = (D + 3) u Σ|gl n| (a term gl n' carries 3 u).

The two grid caps are not exported: csrc/ln.hip ln_grid() caps every grid-stride launch at 256·16 = 4096 workgroups of 256
quads (GRID_CAP_FWD), and ln_bwd_launch() the affine-gradient backward of C < 64 at 1024 (`if (grid > 1024) grid = 1024`,
GRID_CAP_BWD).  The seams that are exported are taken from the library's answers: `sub_seam`, `rowsum_seams`."""
import torch
import torch.nn.functional as F

EPS = 1e-5
U = 2.0 ** -24
SLACK = 1.01
BF = torch.bfloat16
DTYPES = {"fp32": torch.float32, "bf16": BF}
GRID_CAP_FWD = 256 * 16      # ln_grid
GRID_CAP_BWD = 1024          # ln_bwd_launch: if (grid > 1024) grid = 1024
SLICE_C = (64, 128, 256, 512)


def is_pow2(n):
    return n & (n - 1) == 0


# ------------------------------------------------------------------ seams, from the library's own answers ------------------
def ws_rows(lib, B, C, V):
    """rows of 2C floats in the backward's workspace (fz_ln_bwd_workspace_bytes2), the 64 scratch rows included"""
    by = lib.fz_ln_bwd_workspace_bytes2(B, C, V)
    assert by % (8 * C) == 0
    return by // (8 * C)


def sub_seam(lib):
    """the quad count at which the slice kernel leaves SUB = 4 for SUB = 1: one partial row per 16 quads below it, per 64 from
    it on, so the number of workspace rows falls there (and only there: it grows with the quads everywhere else)"""
    rows = lambda q: ws_rows(lib, 1, 64, 4 * q)
    lo, hi = 16 * 1024 + 16, 1 << 22       # above the floor of 1024 rows on the SUB = 4 side
    assert rows(lo) == (lo + 15) // 16 + 64 and rows(hi) == hi // 64 + 64
    while hi - lo > 1:                      # the largest quad count that still has a row per 16 quads
        mid = (lo + hi) // 2
        lo, hi = (mid, hi) if rows(mid) == (mid + 15) // 16 + 64 else (lo, mid)
    assert rows(hi) < rows(lo)
    return hi


def rowsum_seams(chunks):
    """V at which fz_rowsum takes another chunk count (in the style of inorm_cases.seams), V % 4 == 0"""
    lo, hi = 4, 1 << 24
    assert chunks(lo) == 1 and chunks(hi) > 1
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (mid, hi) if chunks(mid) == 1 else (lo, mid)
    L = lo                                  # a chunk is S = (L + 1) / 2 voxels: V // S chunks, at least 1
    S = (L + 1) // 2
    assert chunks(L) == 1 and chunks(L + 1) == 2 and chunks(3 * L + 5) == (3 * L + 5) // S and S % 4 == 0
    top = chunks(1 << 40)                   # the cap
    assert chunks(top * S - 1) == top - 1 and chunks(top * S) == top and chunks(2 * top * S) == top
    return {"last_of_1": L // 4 * 4, "first_of_2": L + 1, "three_plus_4": 3 * S + 4, "cap": top * S + 4, "L": L, "S": S, "top": top}


def bwd_path(C, quads, seam, params=True):
    if C in SLICE_C:
        return "slice_sub4" if quads < seam else "slice_sub1"
    if C > 64:
        return "split16" if C >= 256 else "split8"
    return ("generic32" if C <= 32 else "generic64") if params else "generic0"


def partial_rows(C, quads, seam):
    """rows that ln_bwd_launch writes before the row reduction"""
    p = bwd_path(C, quads, seam)
    if p == "slice_sub4":
        return (quads + 15) // 16
    if p.startswith("generic"):
        return min((quads + 255) // 256, GRID_CAP_BWD)
    return (quads + 63) // 64


def rows_depth(rows, two_stage):
    if not two_stage:
        return (rows + 7) // 8 + 3
    return ((rows + 63) // 64 + 7) // 8 + 3 + 8 + 3


def param_depth(C, quads, seam):
    """depth of the summation tree behind one gγ / gβ element (module docstring)"""
    p, rows = bwd_path(C, quads, seam), partial_rows(C, quads, seam)
    if p.startswith("generic"):
        iters = (quads + rows * 256 - 1) // (rows * 256)
        return iters + 2 + 6 + 2 + rows_depth(rows, False)
    return 2 + (4 if p == "slice_sub4" else 6) + rows_depth(rows, rows > 512)


# ------------------------------------------------------------------ storage ------------------------------------------------
def store(t, dtype, trunc=False):
    """float64 -> the storage type, round-to-nearest-even (exact through fp32 for the exact cases); trunc: the mutant"""
    t = t.float()
    if dtype == torch.float32:
        return t
    if trunc:
        return (t.view(torch.int32) & -65536).view(torch.float32).to(BF)
    return t.to(BF)


def half_ulp_bf16(ref, d):
    """half a unit in the last place of bf16 at |ref| + d (the value that is stored lies within d of ref); 0 where that is 0"""
    t = ref.abs() + d
    e = torch.frexp(t)[1]                    # t = m 2^e, 1/2 <= m < 1: the bf16 unit there is 2^(e - 8)
    return torch.where(t > 0, torch.ldexp(torch.ones_like(t), e - 9), torch.zeros_like(t))


def bf16_ties(t64):
    """how many elements sit exactly half-way between two bf16 numbers"""
    f = t64.float()
    assert torch.equal(f.double(), t64)
    return int(((f.view(torch.int32) & 0xFFFF) == 0x8000).sum())


# ------------------------------------------------------------------ oracle -------------------------------------------------
def _chunks(C, V):
    step = max(4, (1 << 22) // C)
    return [(v, min(V, v + step)) for v in range(0, V, step)]


def fwd64(x, g, b, eps=EPS, mutant=None, out_dtype=torch.float64):
    """(mu, rs, y): mu, rs float64 (B, V); y of out_dtype (float64, or the storage type, rounded as the kernel's store must)"""
    B, C, V = x.shape
    g64, b64 = g.double().view(1, C, 1), b.double().view(1, C, 1)
    if mutant == "gamma_next":
        g64 = g64.roll(-1, 1)
    mu, rs = (torch.empty((B, V), dtype=torch.float64, device=x.device) for _ in range(2))
    y = torch.empty((B, C, V), dtype=out_dtype, device=x.device)
    for v0, v1 in _chunks(C, V):
        xc = x[:, :, v0:v1].double()
        m = xc.mean(1)
        if mutant == "mean_drop_last":
            m = xc[:, :-1].sum(1) / C
        if mutant == "one_pass_fp32":
            xf = xc.float()
            m32 = xf.sum(1) / C
            var = ((xf * xf).sum(1) / C - m32 * m32).double()
            m = m32.double()
        else:
            var = ((xc - m[:, None]) ** 2).sum(1) / (C - 1 if mutant == "div_c_minus_1" else C)
        r = 1 / (var.clamp_min(0).sqrt() + eps) if mutant == "eps_outside" else (var + eps).rsqrt()
        yc = (xc - m[:, None]) * r[:, None] * g64 + b64
        mu[:, v0:v1], rs[:, v0:v1] = m, r
        y[:, :, v0:v1] = yc if out_dtype == torch.float64 else store(yc, out_dtype, mutant == "bf16_trunc")
    return mu, rs, y


def bwd64(gl, x, stats, g, gadd=None, mutant=None, out_dtype=torch.float64):
    """dict gx (out_dtype), gg, gb (float64), gg_terms, gb_terms (Σ|terms| per channel), representable (gx, when stored in a
    narrower out_dtype: every float64 value was a float32 number)"""
    B, C, V = x.shape
    g64 = g.double().view(1, C, 1)
    if mutant == "gamma_next":
        g64 = g64.roll(-1, 1)
    div = C - 1 if mutant == "div_c_minus_1" else C
    gx = torch.empty((B, C, V), dtype=out_dtype, device=x.device)
    acc = torch.zeros((4, C), dtype=torch.float64, device=x.device)
    rep = True
    for v0, v1 in _chunks(C, V):
        xc, gc = x[:, :, v0:v1].double(), gl[:, :, v0:v1].double()
        mu, rs = stats[:, 0:1, v0:v1].double(), stats[:, 1:2, v0:v1].double()
        n = (xc - mu) * rs
        a = gc * g64
        m1 = (a[:, :-1] if mutant == "m1_drop_last" else a).sum(1, keepdim=True) / div
        an = a * n
        m2 = (an[:, :-1] if mutant == "m2_drop_last" else an).sum(1, keepdim=True) / div
        o = rs * (a - m1 - n * m2)
        if gadd is not None:
            r = gadd[:, :, v0:v1].double()
            if mutant == "gadd_skip_last":
                r = r.clone()
                r[:, -1] = 0
            o = o + r
        t = gc * n
        if mutant == "params_drop_last_quad" and v1 == V:
            t, gc = t.clone(), gc.clone()
            t[-1, :, -4:] = 0
            gc[-1, :, -4:] = 0
        acc[0] += t.sum((0, 2))
        acc[1] += gc.sum((0, 2))
        acc[2] += t.abs().sum((0, 2))
        acc[3] += gc.abs().sum((0, 2))
        if out_dtype == torch.float64:
            gx[:, :, v0:v1] = o
        else:
            rep = rep and bool((o.float().double() == o).all())
            gx[:, :, v0:v1] = store(o, out_dtype, mutant == "bf16_trunc")
    return {"gx": gx, "gg": acc[0], "gb": acc[1], "gg_terms": acc[2], "gb_terms": acc[3], "representable": rep}


FWD_MUTANTS = ["mean_drop_last", "div_c_minus_1", "eps_outside", "gamma_next", "one_pass_fp32", "bf16_trunc"]
BWD_MUTANTS = ["m1_drop_last", "m2_drop_last", "div_c_minus_1", "gamma_next", "gadd_skip_last", "params_drop_last_quad",
               "bf16_trunc"]


# ------------------------------------------------------------------ bounds (module docstring) -----------------------------
def fwd_bounds(x, g, b, dtype, eps=EPS):
    """element-wise bounds (dmu, drs, dy) around fwd64(x, g, b)"""
    B, C, V = x.shape
    x64 = x.double()
    mu, rs, y = fwd64(x, g, b, eps)
    d = x64 - mu[:, None]
    dmu = (C - 1) * U * x64.abs().sum(1) / C + 2 * U * mu.abs()
    Q = (d * d).sum(1)
    dq = (C + 2) * U * Q + C * dmu ** 2
    v = Q / C + eps
    drs_rel = (dq / C + 3 * U * v) / (2 * v) + 4 * U
    ga = g.double().abs().view(1, C, 1)
    n = d * rs[:, None]
    dy = ga * rs[:, None] * (U * d.abs() + dmu[:, None]) + ga * n.abs() * (drs_rel[:, None] + 2 * U) + U * y.abs()
    if dtype == BF:
        dy = dy + half_ulp_bf16(y, dy)
    return SLACK * dmu, SLACK * drs_rel * rs, SLACK * dy


def bwd_bounds(gl, x, stats, g, gadd, dtype, depth):
    """bounds (dgx element-wise, dgg, dgb per channel) around bwd64(gl, x, stats, g, gadd)"""
    B, C, V = x.shape
    ref = bwd64(gl, x, stats, g, gadd)
    mu, rs = stats[:, 0:1].double(), stats[:, 1:2].double()
    n = (x.double() - mu) * rs
    a = gl.double() * g.double().view(1, C, 1)
    A1, A2 = a.abs().sum(1, keepdim=True), (a * n).abs().sum(1, keepdim=True)
    m1, m2 = a.mean(1, keepdim=True), (a * n).mean(1, keepdim=True)
    dm1, dm2 = (C + 2) * U * A1 / C, (C + 5) * U * A2 / C
    dgx = rs * (dm1 + n.abs() * dm2 + 6 * U * (a.abs() + m1.abs() + (n * m2).abs())) + U * ref["gx"].abs()
    if dtype == BF:
        dgx = dgx + half_ulp_bf16(ref["gx"], dgx)
    return SLACK * dgx, SLACK * (depth + 3) * U * ref["gg_terms"], SLACK * depth * U * ref["gb_terms"], ref


def stats_bounds(x, eps=EPS):
    """bounds (dmu, drs) for any producer of the statistics: the larger of the two-pass derivation (fwd_bounds) and that of
    the pivoted single pass of the streaming GEMM prologues (csrc/gemm_bx.hip, gemm_bxk.hip, gemm_stream.hip), which sums
    d = x - p and d^2 around the pivot p = x[channel 0] and takes mu = p + m, v = Σ d^2 / C - m^2 + eps with m = Σ d / C:
    dm = (C - 1) u Σ|d| / C + 2 u |m|, dmu = dm + u |mu|; Σ d^2 carries (C + 2) u and the division one more: dv =
    (C + 3) u Σ d^2 / C + 2 |m| dm + 3 u (Σ d^2 / C + m^2 + v); drs / rs = dv / (2 v) + 4 u"""
    B, C, V = x.shape
    one, zero = torch.ones(C, device=x.device), torch.zeros(C, device=x.device)
    dmu, drs, _ = fwd_bounds(x, one, zero, torch.float32, eps)
    mu, rs, _ = fwd64(x, one, zero, eps)
    d = x.double() - x[:, :1].double()
    m, q = d.mean(1), (d * d).sum(1) / C
    dm = (C - 1) * U * d.abs().sum(1) / C + 2 * U * m.abs()
    v = rs ** -2
    dv = (C + 3) * U * q + 2 * m.abs() * dm + 3 * U * (q + m * m + v)
    return torch.maximum(dmu, SLACK * (dm + U * mu.abs())), torch.maximum(drs, SLACK * (dv / (2 * v) + 4 * U) * rs)


def fraction(got, ref, bound):
    """max over the elements of |got - ref| / bound (1 is the bound); an element with a zero bound must be exact"""
    ref = ref.double()
    got = got.detach().to(ref.device).double()
    assert got.shape == ref.shape and torch.isfinite(got).all()
    err, bound = (got - ref).abs(), bound.to(ref.device).double().expand_as(ref)
    if float(err.max()) == 0:
        return 0.0
    return float(torch.where(err > 0, err / bound.clamp_min(1e-300), err).max())


# ------------------------------------------------------------------ exact inputs -------------------------------------------
def _gen(seed, device):
    return torch.Generator(device=device).manual_seed(seed)


def _ri(lo, hi, shape, gen):
    return torch.randint(lo, hi + 1, shape, generator=gen, device=gen.device, dtype=torch.float32)


def _gamma(C, gen):
    return (2.0 ** _ri(-1, 1, (C,), gen)) * (2 * _ri(0, 1, (C,), gen) - 1)


def exact_bwd(B, C, V, dtype, with_gadd=True, seed=0, device="cpu"):
    """(gl, x, stats, γ, gadd) of the module docstring; gl, x, gadd of `dtype`"""
    gen = _gen(seed + 1000 * C + V, device)
    stats = torch.cat([_ri(-1, 1, (B, 1, V), gen), 2.0 ** _ri(-1, 1, (B, 1, V), gen)], 1)
    if is_pow2(C):
        x, gl, g = _ri(-3, 3, (B, C, V), gen), _ri(-2, 2, (B, C, V), gen), _gamma(C, gen)
    else:
        P = C // 2
        x = _ri(-3, 3, (B, P, V), gen).repeat_interleave(2, 1)
        gl = _ri(-2, 2, (B, P, V), gen).repeat_interleave(2, 1)
        g = _gamma(P, gen).repeat_interleave(2)
        flip = _ri(0, 1, (P,), gen).bool()         # which of the pair's two factors changes sign
        g[1::2] = torch.where(flip, -g[1::2], g[1::2])
        gl[:, 1::2] = torch.where(flip.view(1, P, 1), gl[:, 1::2], -gl[:, 1::2])
        if C % 2:
            x = torch.cat([x, _ri(-3, 3, (B, 1, V), gen)], 1)
            gl = torch.cat([gl, torch.zeros((B, 1, V), device=device)], 1)
            g = torch.cat([g, _gamma(1, gen)])
    gadd = (_ri(-4, 4, (B, C, V), gen) + 128 * _ri(-1, 1, (B, C, V), gen)) if with_gadd else None
    cast = lambda t: None if t is None else t.to(dtype).contiguous()
    return cast(gl), cast(x), stats.contiguous(), g.contiguous(), cast(gadd)


def exact_dgrad(B, C, Mz, V, dtype, seed=0, device="cpu"):
    """(gz, w2, gl, x, stats, γ, gadd) for the fused dgrad + LayerNorm backward: w2 (Mz, C) has one ±1 per column and gz
    integers in [-2, 2], so gl = w2ᵀ gz is again integers in [-2, 2] — the exactness condition of exact_bwd (C a power of two)"""
    assert is_pow2(C)
    _, x, stats, g, gadd = exact_bwd(B, C, V, dtype, True, seed, device)
    gen = _gen(seed + 77 + Mz, device)
    rows = torch.randint(0, Mz, (C,), generator=gen, device=device)
    w2 = torch.zeros((Mz, C), device=device)
    w2[rows, torch.arange(C, device=device)] = 2 * _ri(0, 1, (C,), gen) - 1
    gz = _ri(-2, 2, (B, Mz, V), gen)
    gl = torch.einsum("mc,bmv->bcv", w2.double(), gz.double())
    assert float(gl.abs().max()) <= 2 and torch.equal(gl, gl.round())
    return gz.to(dtype).contiguous(), w2.contiguous(), gl.to(dtype).contiguous(), x, stats, g, gadd


def exact_fwd(B, C, V, dtype, seed=0, device="cpu"):
    """(x, γ, β): integer x whose channel mean is exact in fp32 (C a power of two, else channels in opposite pairs)"""
    gen = _gen(seed + 1000 * C + V + 7, device)
    if is_pow2(C):
        x = _ri(-3, 3, (B, C, V), gen)
    else:
        x = _ri(-3, 3, (B, C // 2, V), gen).repeat_interleave(2, 1)
        x[:, 1::2] = -x[:, 1::2]
        if C % 2:
            x = torch.cat([x, torch.zeros((B, 1, V), device=device)], 1)
    return x.to(dtype).contiguous(), _gamma(C, gen), _ri(-4, 4, (C,), gen)


# ------------------------------------------------------------------ rounded inputs -----------------------------------------
def _rn(shape, gen):
    return torch.randn(shape, generator=gen, device=gen.device)


ROUNDED = {   # name -> x of shape s from generator k
    "randn": lambda s, k: _rn(s, k),
    "mean_30_std_half": lambda s, k: 30 + 0.5 * _rn(s, k),
    "mean_1000": lambda s, k: 1000 + _rn(s, k),
    "var_near_eps": lambda s, k: 1e-3 * _rn(s, k),
    "scale_1e4_offset_5e5": lambda s, k: 1e4 * _rn(s, k) + 5e5,
    "relu_sparse_gl": lambda s, k: _rn(s, k),
    "gamma_mixed_signs_one_zero": lambda s, k: 2 * _rn(s, k) + 1,
}
LARGE_MEAN = ("mean_30_std_half", "mean_1000", "scale_1e4_offset_5e5")


def rounded(name, B, C, V, dtype, with_gadd=True, seed=0, device="cpu"):
    """(x, γ, β, gl, gadd): x, gl, gadd already rounded to `dtype` (the oracle sees what the kernel sees)"""
    gen = _gen(seed + 31 * sorted(ROUNDED).index(name) + 1000 * C + V, device)
    s = (B, C, V)
    x = ROUNDED[name](s, gen)
    g, b = 1 + 0.5 * _rn((C,), gen), _rn((C,), gen)
    gl = _rn(s, gen)
    if name == "relu_sparse_gl":
        gl = torch.relu(gl) * (_rn(s, gen) > 0.5)
    if name == "gamma_mixed_signs_one_zero":
        g = _rn((C,), gen)
        g[C // 2] = 0
    # the added gradient is one with respect to the same x: of the size of gx, about rs (else a bf16 store hides one from the other)
    scale = {"scale_1e4_offset_5e5": 1e-4, "var_near_eps": 300.0, "mean_30_std_half": 2.0}.get(name, 1.0)
    gadd = scale * _rn(s, gen) if with_gadd else None
    cast = lambda t: None if t is None else t.to(dtype).contiguous()
    return cast(x), g.contiguous(), b.contiguous(), cast(gl), cast(gadd)


def stats_of(x, eps=EPS):
    """the (B, 2, V) fp32 statistics tensor of x (float64 statistics rounded once)"""
    x64 = x.double()
    mu = x64.mean(1, keepdim=True)
    rs = (((x64 - mu) ** 2).mean(1, keepdim=True) + eps).rsqrt()
    return torch.cat([mu, rs], 1).float().contiguous()


# ------------------------------------------------------------------ fp32 emulation in the kernel's channel order ------------
def emulate_fwd(x, g, b, dtype, eps=EPS, reverse=False):
    """ln_fwd_kernel in fp32 on the CPU: sequential channel sums (reverse: from the last channel), same operation order"""
    B, C, V = x.shape
    xf = x.float()
    order = range(C - 1, -1, -1) if reverse else range(C)
    s = torch.zeros((B, V))
    for c in order:
        s = s + xf[:, c]
    inv = torch.tensor(1.0) / torch.tensor(float(C))
    mu = s * inv
    q = torch.zeros((B, V))
    for c in order:
        d = xf[:, c] - mu
        q = q + d * d
    rs = 1.0 / torch.sqrt(q * inv + torch.tensor(eps))
    y = (xf - mu[:, None]) * rs[:, None] * g.view(1, C, 1) + b.view(1, C, 1)
    return mu, rs, y.to(dtype)


def emulate_bwd(gl, x, stats, g, gadd, dtype, lanes=1, reverse=False):
    """the backward kernels in fp32 on the CPU.  lanes = 1: ln_bwd_kernel (one sequential channel sum); lanes = 8·SUB / 8 /
    16: the slice and split kernels (sequential sums over C / lanes consecutive channels, combined pairwise, then in order).
    gγ, gβ: fp32 sums over blocks of 64 quads, then sequentially over the blocks."""
    B, C, V = x.shape
    xf, gf, gv = x.float(), gl.float(), g.view(1, C, 1)
    mu, rs = stats[:, 0:1], stats[:, 1:2]
    n = (xf - mu) * rs
    a = gf * gv
    an = a * n
    cs = -(-C // lanes)

    def tree(t):
        parts = []
        for l in range(lanes):
            idx = list(range(l * cs, min(C, (l + 1) * cs)))
            acc = torch.zeros((B, V))
            for c in (reversed(idx) if reverse else idx):
                acc = acc + t[:, c]
            parts.append(acc)
        while lanes == 32 and len(parts) > 8:                  # the 4 sub-slices of a wave: a butterfly
            parts = [parts[i] + parts[i + 1] for i in range(0, len(parts), 2)]
        acc = torch.zeros((B, V))
        for p in parts:
            acc = acc + p
        return acc[:, None]

    inv = torch.tensor(1.0) / torch.tensor(float(C))
    m1, m2 = tree(a) * inv, tree(an) * inv
    o = rs * (a - m1 - n * m2)
    if gadd is not None:
        o = o + gadd.float()
    t = (gf * n).permute(1, 0, 2).reshape(C, -1)
    d = gf.permute(1, 0, 2).reshape(C, -1)

    def blocks(t):
        pad = (-t.shape[1]) % 256
        rows = F.pad(t, (0, pad)).view(C, -1, 256).sum(2)
        acc = torch.zeros(C)
        for r in range(rows.shape[1]):
            acc = acc + rows[:, r]
        return acc

    return o.to(dtype), blocks(t), blocks(d)


def lanes_of(path):
    return {"slice_sub4": 32, "slice_sub1": 8, "split8": 8, "split16": 16}.get(path, 1)


# ------------------------------------------------------------------ the sweeps shared by the CPU and the GPU file -----------
GENERIC_C = [1, 2, 5, 16, 32, 33, 48, 63]
GENERIC_BV = [(1, 4), (3, 20), (2, 1028)]
SLICE_BV = [(1, 4), (1, 60), (3, 20)]
SPLIT_C = [96, 100, 320, 1024]
SPLIT_BV = [(3, 20), (1, 60)]
FWD_C = [1, 2, 6, 32, 64, 512]
ROUNDED_SHAPES = {   # one representative (B, C, V) per kernel path; the SUB = 1 shape is set at the library's seam
    "generic32": (2, 32, 1028), "generic64": (2, 48, 1028), "slice_sub4_keep": (3, 128, 20), "slice_sub4_c512": (3, 512, 20),
    "split8": (3, 96, 20), "split16": (1, 320, 60),
}
