"""Oracle, inputs, bounds, mutants and seams of the chained-MLP and fused dgrad + wgrad tests (tests/test_mlp_chain_cpu.py:
the tools checked on the CPU; tests/test_gpu_mlp_chain.py: csrc/mlp_chain32.hip, mlp_chain64.hip, mlp_chain_wg.hip, gemm_dw.hip
on the device).  The LayerNorm parts are the ones of tests/ln_cases.py, imported.

Oracle (float64, closed forms; tensors are (B, C, V); every seam is reached by the batch count at V <= 516, so no tensor is large)
  forward   x1 = x + Wo a + bo (PRE), (mu, rs, LN) = LayerNorm(x1), z1 = W1 LN + b1, x2 = x1 + W2 gelu(z1) + b2 (erf-GELU), logits =
            Wh x2 + bh.  With bf16 storage the kernel normalises the STORED x1 and the head reads the STORED x2: `fwd64` takes the
            device's x1 and x2 for those two steps, so no element has to be excluded for a tie broken the other way.
  backward  of (g2, z1, x1, stats, γ, β, W1, W2) with z1 and stats the tensors the kernel reads: gz1 = (W2ᵀ g2) gelu'(z1), gx1 =
            LNbwd(W1ᵀ gz1) + g2, gγ, gβ, gW2 = Σ g2 ⊗ gelu(z1), gb2 = Σ g2, gW1 = Σ gz1 ⊗ LN(x1), gb1 = Σ gz1
  gemm_dw   out_proj form y = Wᵀ g, gw = Σ g ⊗ q, gb = Σ g; in_proj form y = LNbwd(Wᵀ g) + gadd, gγ, gβ, gw = Σ g ⊗ LN(q)
  Every voxel sum also returns its Σ|terms|.

Exact inputs (`exact_mlp_bwd`, `exact_dw`, on ln_cases.exact_bwd / exact_dgrad): x, stats, γ as there, β and g2 small integers, W2
and W1 with one ±1 per column (W2ᵀ g2 and W1ᵀ gz1 stay integers in [-2, 2]), z1 in {-16, +16}: the library's own GELU formula is
exact there in fp32 (fast_erf(±16/√2): expf(-128) = 0, so gelu' in {0, 1}, gelu in {-0, 16}; `emu_gelu`, `emu_gelu_grad` check it;
z = -8 and z = 0 are not exact).  Every operand has at most 16 significant bits: exact under the two- and three-level bf16 split.
Σ|terms| < 2^22: the float64 answer is the only correct one, whatever the tile order, product mode or contraction.

Bounds (a priori, element-wise, first order in u = 2^-24 times SLACK; nothing is tuned on a device)
  dot product of K terms in any order: ((K - 1) u + u_prod) Σ|terms|, u_prod per product mode (csrc/gemm_bx.h):
    fp32 MFMA      u (one rounding per product-accumulate)
    three levels   x = x1 + x2 + x3, |x2| <= 2^-8 |x|, |x3| <= 2^-16 |x|, six products kept; dropped x2 y3, x3 y2, x3 y3:
                   2^-8 2^-16 + 2^-16 2^-8 + 2^-32 of |x||y| = 2^-23 + 2^-32
    two levels     hi = rne(x), lo = rne(x - hi): each operand is represented to 2^-17 (two representation errors) and hi·hi +
                   hi·lo + lo·hi drops lo·lo <= 2^-9 2^-9 = 2^-18: 2^-16 + 2^-18 = 1.25 · 2^-16
    `emu_dot` splits with torch.bfloat16 casts; tests/test_mlp_chain_cpu.py holds it under these and one level fewer over them.
  forward   x1: ((C + 2) u + u_prod) (Σ|Wo a| + |bo| + |x|) [+ half_ulp_bf16].  x̂: ln_cases.fwd_bounds with γ = 1, β = 0 (dn).
            z1 = (W1 γ) x̂ + (W1 β + b1) (the affine is folded into the staged weights: one more u): dz1 = ((C + 3) u + u_prod) T1 +
            Σ_c |W1 γ| dn + u |z1|, T1 = Σ_c |W1 γ x̂| + Σ_c |W1 β| + |b1|.  gelu: dgelu(z) = ½ |z| d_erf + u |gelu| at the computed z,
            and moving z by dz1 moves it by at most 1.13 dz1 (the Lipschitz constant of erf-GELU is below 1.13).
            x2: ((H + 3) u + u_prod) (Σ_h |W2 gelu| + |b2| + |x1|) + Σ_h |W2| (1.13 dz1 + dgelu) + u |x2| [+ half_ulp_bf16].
            logits from the stored x2 (plain fp32 FMAs): (C + 3) u (Σ|Wh x2| + |bh|) [+ half_ulp_bf16].
  backward  gh = W2ᵀ g2: dgh = ((C - 1) u + u_prod) Σ|W2 g2|.  gelu'(z) = cdf + z pdf: dgelu' = ½ d_erf + |z| 2u pdf·(1 + z²/2) + u
            (pdf = c expf(-z²/2): the argument carries 2u z²/2).  gz1 = gh gelu': dgz1 = |gelu'| dgh + |gh| dgelu' + u |gz1|
            [+ half_ulp_bf16 where it is stored].  gl = W1ᵀ gz1: dgl = ((H - 1) u + u_prod) Σ|W1 gz1| + Σ|W1| dgz1.
            gx1: ln_cases.bwd_bounds of the exact gl, plus what dgl moves: rs (|γ| dgl + mean_c |γ| dgl + |n| mean_c(|γ| dgl |n|)),
            plus (two-level arm: x̂ is rebuilt from its two planes, 2^-17 |n|) rs 2^-17 (|n m2| + |n| mean_c |a n|),
            plus (two-level arm, fp32 storage) 2^-17 |g2|: the residual rows g2 are not read again from memory but joined from
            the hi and lo plane GEMM 1 left in LDS (mlp_chain_wg.hip, "the residual rows g2 in the ACCUMULATOR layout, read back
            from Bf") — 16 of their 24 bits; with bf16 storage the hi plane is g2 itself.  The first device run of the family
            g*2^40,w*2^-40 (where nothing else is added to g2) showed this term missing: 126 times the bound without it.
            voxel sums of depth D (below): gβ: D u Σ|gl| + Σ dgl; gγ: (D + 3) u Σ|gl n| + Σ dgl |n|; gb2: D u Σ|g2|;
            gb1: D u Σ|gz1| + Σ dgz1 (two-level arm: the bias sums are dot products on the planes, + 2^-17 Σ|terms|); gW2: ((D + 2) u + u_prod) Σ|g2 gelu| + Σ|g2| dgelu;
            S1 = Σ gz1 ⊗ x̂: ((D + 4) u + u_prod) Σ|gz1 n| + Σ dgz1 |n|; gW1 = γ S1 + β gb1: |γ| dS1 + |β| dgb1 + 2u (|γ S1| + |β gb1|).
  d_erf     the error of the library's fast_erf (Abramowitz-Stegun 7.1.26, fz_common.h) INCLUDING its fp32 evaluation, measured
            against float64 erf with `emu_fast_erf` on a dense grid of z in [-12, 12]: 5.41e-7, D_ERF_MEASURED = 5.5e-7 (the formula
            alone: 1.5e-7; the rest is the fp32 rounding of 1 − poly·exp next to 1 and of the argument z/√2).
            D_ERF = 2 · that: the device's v_rcp_f32 and v_exp_f32 are 1-ulp approximations, torch's are correctly rounded.
  depth D   of the tree behind one voxel sum, from the kernels.  Mode 1 and chain64 (LayerNorm rows only): 2 columns in a lane (1),
            half_sum32 (5), 4 waves (2), then one partial row per TILE into fz_reduce_rows (ln_cases.rows_depth, two stages above
            512 rows).  Mode 2 and gemm_dw: the MFMA reduction runs over the 64 voxels of a wave's tile slice, added to accumulators
            that are carried over the tiles a workgroup walks (64 · ceil(tiles / rows) sequential terms at worst), 4 waves (2), then
            the finish job: rows in 16 strided sequential slices and the 16 slices in order (ceil(rows / 16) + 16).

Seams: fz_mlp_partials gives the tile count (256 voxels a tile, B · ceil(V / 256)); every kernel runs min(tiles, cap) resident
workgroups.  fz_mlp_wgrad_rows and fz_gemm_dw_rows export their cap (`cap_of_rows`).  The others are constants: csrc/mlp_chain32.hip
chain32_launch `knob_mlp_wgs(d->H == 128 || bx ? 512 : 768)`, csrc/mlp_chain64.hip chain64_launch `wgs = p512 ? 256 : knob_mlp_wgs(512)`
(pairs of tiles for the 512-thread form), chain64_lnb_launch `ntiles < 512 ? ntiles : 512`."""
import math

import torch

import ln_cases as LC
from ln_cases import (SLACK, U, bwd64 as ln_bwd64, exact_bwd, exact_dgrad, fraction, half_ulp_bf16, stats_of,  # noqa: F401
                      store)

BF = torch.bfloat16
DTYPES = LC.DTYPES
EPS = LC.EPS
TILE = 256
CAP_512, CAP_768, CAP_PAIRS = 512, 768, 256      # chain32_launch / chain64_launch (module docstring)
D_ERF_MEASURED = 5.5e-7    # 5.41e-7: max |emu_fast_erf(z / √2) − erf(z / √2)| over the grid of `measure_d_erf` (asserted on the CPU)
D_ERF = 2 * D_ERF_MEASURED  # the device's 1-ulp rcp and exp against torch's correctly rounded ones
GELU_LIP = 1.13
U_PROD = {"fp32": U, "three": 2.0 ** -23 + 2.0 ** -32, "two": 1.25 * 2.0 ** -16}


# ------------------------------------------------------------------ seams --------------------------------------------------
def tiles(lib, B, V):
    n = int(lib.fz_mlp_partials(B, V))
    assert n == B * ((V + TILE - 1) // TILE)
    return n


def cap_of_rows(rows):
    """the resident-workgroup cap behind fz_mlp_wgrad_rows / fz_gemm_dw_rows: rows(B, 4) = min(B, cap)"""
    assert rows(1, 4) == 1 and rows(3, 260) == 6
    cap = int(rows(1 << 20, 4))
    assert rows(cap - 1, 4) == cap - 1 and rows(cap, 4) == cap and rows(cap + 1, 4) == cap
    return cap


def seam_bv(cap):
    """(name, B, V, tiles) of one launcher with `cap` resident workgroups: one 4-column tile, one full tile, a full tile and a
    4-column one, then cap, cap + 1 and 2 cap + 1 tiles by batch count (there some workgroups walk 3 tiles and the rest 2) and
    cap + 2 tiles in which full and 4-column tiles alternate"""
    assert cap % 2 == 0
    return [("v4", 1, 4, 1), ("v256", 1, 256, 1), ("v260", 1, 260, 2), ("cap", cap, 4, cap), ("cap+1", cap + 1, 4, cap + 1),
            ("2cap+1", 2 * cap + 1, 4, 2 * cap + 1), ("cap+2_v260", cap // 2 + 1, 260, cap + 2)]


# the 512-thread C = 64 form walks PAIRS of tiles and takes an even tile count: a pair across two samples, three tiles per
# sample (the middle pair straddles), 513 pairs (above 2 · 256: a workgroup walks 3 pairs), and the cap itself
PAIR_BV = [("v260", 1, 260, 2), ("straddle_1pair", 2, 120, 2), ("straddle_mid", 2, 516, 6), ("cap_pairs", CAP_PAIRS, 260, 2 * CAP_PAIRS),
           ("cap+1_pairs", CAP_PAIRS + 1, 260, 2 * CAP_PAIRS + 2), ("2cap+1_pairs", 2 * CAP_PAIRS + 1, 260, 4 * CAP_PAIRS + 2)]
ROUNDED_AT = ("v260", "cap+1", "2cap+1")
ROUNDED_AT_PAIRS = ("v260", "cap+1_pairs", "2cap+1_pairs")


def tile_cols(t, V):
    """(sample, first column, end column) of tile t"""
    tps = (V + TILE - 1) // TILE
    b, k = divmod(t, tps)
    return b, k * TILE, min(V, (k + 1) * TILE)


# ------------------------------------------------------------------ GELU ---------------------------------------------------
def gelu64(z, mutant=None):
    if mutant == "tanh_gelu":
        return 0.5 * z * (1 + torch.tanh(math.sqrt(2 / math.pi) * (z + 0.044715 * z ** 3)))
    return 0.5 * z * (1 + torch.erf(z / math.sqrt(2)))


def gelu_grad64(z, mutant=None):
    cdf = 0.5 * (1 + torch.erf(z / math.sqrt(2)))
    if mutant == "gelu_grad_no_xpdf":
        return cdf
    return cdf + z * torch.exp(-0.5 * z * z) / math.sqrt(2 * math.pi)


def flush(t):
    """magnitudes below 2^-150 round to zero in every fp32 computation (gelu'(-16) = -1.6e-55 is such a number)"""
    return torch.where(t.abs() < 2.0 ** -150, torch.zeros_like(t), t)


def emu_fast_erf(x):
    """fast_erf of fz_common.h in fp32, operation by operation (torch's division and exp are correctly rounded)"""
    assert x.dtype == torch.float32
    f = lambda v: torch.tensor(v, dtype=torch.float32)
    ax = x.abs()
    t = f(1.0) / (f(1.0) + f(0.3275911) * ax)
    poly = t * (f(0.254829592) + t * (f(-0.284496736) + t * (f(1.421413741) + t * (f(-1.453152027) + t * f(1.061405429)))))
    r = f(1.0) - poly * torch.exp(-ax * ax)
    return torch.copysign(r, x)


def emu_gelu(z):
    return (f32(0.5) * z) * (f32(1.0) + emu_fast_erf(z * f32(0.70710678118654752)))


def emu_gelu_grad(z):
    cdf = f32(0.5) * (f32(1.0) + emu_fast_erf(z * f32(0.70710678118654752)))
    return cdf + z * (f32(0.3989422804014327) * torch.exp(f32(-0.5) * z * z))


def f32(v):
    return torch.tensor(v, dtype=torch.float32)


def measure_d_erf():
    """max error of emu_fast_erf(z / √2) against float64 erf(z / √2), z on a dense grid of [-12, 12] and around 0"""
    z = torch.cat([torch.linspace(-12, 12, 2_000_001, dtype=torch.float64), torch.linspace(-1e-3, 1e-3, 20001, dtype=torch.float64)]).float()
    got = emu_fast_erf(z * f32(0.70710678118654752)).double()
    return float((got - torch.erf(z.double() / math.sqrt(2))).abs().max())


def dgelu(z):
    return 0.5 * z.abs() * D_ERF + U * gelu64(z).abs()


def dgelu_grad(z):
    pdf = torch.exp(-0.5 * z * z) / math.sqrt(2 * math.pi)
    return 0.5 * D_ERF + z.abs() * 2 * U * pdf * (1 + 0.5 * z * z) + U


# ------------------------------------------------------------------ split-bf16 products, emulated in fp32 ------------------
def levels_of(t, n):
    """t = t1 + t2 + ... (n round-to-nearest bf16 levels, as bx_split of gemm_bx.h), each level as fp32"""
    out, r = [], t.float()
    for _ in range(n):
        l = r.to(BF).float()
        out.append(l)
        r = r - l
    return out


def emu_dot(a, b, mode, fewer=False):
    """a (M, K) @ b (K, N) in fp32 as the product mode multiplies: "fp32"; "three": six products of three levels; "two": hi·hi +
    hi·lo + lo·hi.  fewer (the mutant): one split level fewer, three -> two -> one.  Each partial product of two bf16 numbers
    is exact in fp32; the accumulation is fp32 in the order of the host's matmul (any order is inside the bound)."""
    a, b = a.float(), b.float()
    if mode == "fp32":
        return a @ b
    n = {"three": 3, "two": 2}[mode] - (1 if fewer else 0)
    la, lb = levels_of(a, n), levels_of(b, n)
    acc = torch.zeros(a.shape[0], b.shape[1])
    for s in range(2 * n - 2, -1, -1):             # smallest products first, as bx_mfma orders them
        for i in range(n):
            j = s - i
            if 0 <= j < n and i + j < n:
                acc = acc + la[i] @ lb[j]
    return acc


def dot_bound(a, b, mode):
    K = a.shape[1]
    return SLACK * ((K - 1) * U + U_PROD[mode]) * (a.double().abs() @ b.double().abs())


# ------------------------------------------------------------------ tile mutants -------------------------------------------
TILE_MUTANTS = ["ragged_last_quad_dropped", "tile_cap_skipped", "tile_cap_twice", "prefetch_last_from_tile0"]
BWD_MUTANTS = TILE_MUTANTS + ["dw1_no_affine", "no_residual", "tanh_gelu", "gelu_grad_no_xpdf"]
# (on the exact inputs z1 = ±16 the two GELU forms and their derivatives agree bit for bit: those two are judged on the rounded
# families alone, as are fp32_z1 — the oracle given the unrounded z1 — and one_pass_var, a forward mutant)
FWD_MUTANTS = ["tanh_gelu", "one_pass_var", "prefetch_last_from_tile0"]


def _col_weights(B, V, mutant, cap, device):
    """how often the voxel sums count each column: 1, but for the tile mutants"""
    w = torch.ones((B, 1, V), dtype=torch.float64, device=device)
    if mutant == "ragged_last_quad_dropped":
        w[-1, :, -4:] = 0
    if mutant in ("tile_cap_skipped", "tile_cap_twice"):
        b, v0, v1 = tile_cols(cap, V)
        assert b < B, "the tile mutants need more than `cap` tiles"
        w[b, :, v0:v1] = 0 if mutant == "tile_cap_skipped" else 2
    return w


def _last_from_tile0(ts, V):
    """the last tile computed from the operands of tile 0 (a prefetch that is not clamped to its own tile)"""
    B = ts[0].shape[0]
    _, v0, v1 = tile_cols(B * ((V + TILE - 1) // TILE) - 1, V)
    out = []
    for t in ts:
        t = t.clone()
        t[B - 1, :, v0:v1] = t[0, :, 0:v1 - v0]
        out.append(t)
    return out


# ------------------------------------------------------------------ oracle -------------------------------------------------
def _c(t):
    return t.double().view(1, -1, 1)


def fwd64(p, x1_stored=None, x2_stored=None, mutant=None):
    """p: dict of x, g, b, w1, b1, w2, b2 and optionally a, wo, bo (PRE), wh, bh (head).  float64 dict: x1 (PRE), mu, rs, ln,
    z1, x2, logits.  x1_stored / x2_stored: the device's stored tensors, read where the kernel reads them."""
    o = {}
    ins = [p["x"]] + ([p["a"]] if "a" in p else [])
    if mutant == "prefetch_last_from_tile0":
        ins = _last_from_tile0(ins, p["x"].shape[2])
    x = ins[0].double()
    if "a" in p:
        o["x1"] = x + torch.einsum("mk,bkv->bmv", p["wo"].double(), ins[1].double()) + (0 if p.get("bo") is None else _c(p["bo"]))
    xin = x1_stored.double() if x1_stored is not None else o.get("x1", x)
    if mutant == "prefetch_last_from_tile0" and x1_stored is not None:
        xin = _last_from_tile0([xin], xin.shape[2])[0]
    o["mu"], o["rs"], o["ln"] = LC.fwd64(xin, p["g"], p["b"], EPS, mutant="one_pass_fp32" if mutant == "one_pass_var" else None)
    o["z1"] = torch.einsum("hc,bcv->bhv", p["w1"].double(), o["ln"]) + _c(p["b1"])
    o["x2"] = xin + torch.einsum("ch,bhv->bcv", p["w2"].double(), gelu64(o["z1"], mutant)) + _c(p["b2"])
    if "wh" in p:
        src = o["x2_read"] = x2_stored.double() if x2_stored is not None else o["x2"]
        o["logits"] = torch.einsum("mc,bcv->bmv", p["wh"].double(), src) + (0 if p.get("bh") is None else _c(p["bh"]))
    return o


def _sums(o, name, terms, w):
    """Σ_{b,v} w·terms and Σ w·|terms| of a (B, R, V) tensor"""
    o[name] = (terms * w).sum((0, 2))
    o[name + "_terms"] = (terms.abs() * w).sum((0, 2))


def bwd64(g2, z1, x1, stats, g, b, w1, w2, mutant=None, cap=None, out_dtype=torch.float64):
    """dict gz1, gx1 (out_dtype), gg, gb, gw1, gb1, gw2, gb2, s1 (= Σ gz1 ⊗ x̂) (float64) and the Σ|terms| of every sum as
    <name>_terms; representable: every element-wise float64 result was a float32 number (the bf16 store then rounds it once)"""
    B, C, V = x1.shape
    ts = [g2, z1, x1, stats]
    if mutant == "prefetch_last_from_tile0":
        ts = _last_from_tile0(ts, V)
    g2d, zd, xd, sd = [t.double() for t in ts]
    w = _col_weights(B, V, mutant, cap, x1.device)
    W1, W2 = w1.double(), w2.double()
    gh = torch.einsum("ch,bcv->bhv", W2, g2d)
    ge = flush(gelu64(zd, mutant))
    gz1 = gh * flush(gelu_grad64(zd, mutant))
    gl = torch.einsum("hc,bhv->bcv", W1, gz1)
    gx1 = ln_bwd64(gl, xd, sd, g, None if mutant == "no_residual" else g2d)["gx"]
    n = (xd - sd[:, 0:1]) * sd[:, 1:2]
    y = n if mutant == "dw1_no_affine" else n * _c(g) + _c(b)
    o = {"gh": gh, "gl": gl, "n": n}
    _sums(o, "gg", gl * n, w)
    _sums(o, "gb", gl, w)
    _sums(o, "gb2", g2d, w)
    _sums(o, "gb1", gz1, w)
    o["gw2"] = torch.einsum("bcv,bhv->ch", g2d * w, ge)
    o["gw2_terms"] = torch.einsum("bcv,bhv->ch", g2d.abs() * w, ge.abs())
    o["gw1"] = torch.einsum("bhv,bcv->hc", gz1 * w, y)
    o["s1"] = torch.einsum("bhv,bcv->hc", gz1 * w, n)
    o["s1_terms"] = torch.einsum("bhv,bcv->hc", gz1.abs() * w, n.abs())
    rep = True
    for k, t in (("gz1", gz1), ("gx1", gx1)):
        if out_dtype == torch.float64:
            o[k] = t
        else:
            o[k] = store(t, out_dtype)
            rep = rep and bool((t.float().double() == t).all())
    o["representable"] = rep
    return o


def dw64(gr, w, q, ln=None, stats=None, gadd=None, mutant=None, cap=None, out_dtype=torch.float64):
    """fz_gemm_dw.  out_proj form (ln None): y = Wᵀ g, gw = Σ g ⊗ q, gb = Σ g.  in_proj form (ln = (γ, β)): y = LNbwd(Wᵀ g; q,
    stats, γ) + gadd, gg, gbt, gw = Σ g ⊗ (γ x̂ + β), s = Σ g ⊗ x̂."""
    B, C, V = q.shape
    ts = [gr, q] + ([stats, gadd] if ln is not None else [])
    if mutant == "prefetch_last_from_tile0":
        ts = _last_from_tile0(ts, V)
    gd, qd = ts[0].double(), ts[1].double()
    wt = _col_weights(B, V, mutant, cap, q.device)
    gl = torch.einsum("mk,bmv->bkv", w.double(), gd)
    o = {"gl": gl}
    _sums(o, "gb", gd, wt)
    if ln is None:
        y, inp = gl, qd
    else:
        sd = ts[2].double()
        y = ln_bwd64(gl, qd, sd, ln[0], None if mutant == "no_residual" else ts[3].double())["gx"]
        n = (qd - sd[:, 0:1]) * sd[:, 1:2]
        inp = n if mutant == "dw1_no_affine" else n * _c(ln[0]) + _c(ln[1])
        o["n"] = n
        _sums(o, "gg", gl * n, wt)
        _sums(o, "gbt", gl, wt)
        o["s"] = torch.einsum("bmv,bkv->mk", gd * wt, n)
    o["gw"] = torch.einsum("bmv,bkv->mk", gd * wt, inp)
    o["s_terms"] = torch.einsum("bmv,bkv->mk", gd.abs() * wt, (o["n"] if ln is not None else qd).abs())
    o["y"] = y if out_dtype == torch.float64 else store(y, out_dtype)
    o["representable"] = out_dtype == torch.float64 or bool((y.float().double() == y).all())
    return o


# ------------------------------------------------------------------ exact inputs -------------------------------------------
def _one_per_column(rows, cols, gen):
    """(rows, cols) with one ±1 in every column"""
    w = torch.zeros((rows, cols), device=gen.device)
    r = torch.randint(0, rows, (cols,), generator=gen, device=gen.device)
    w[r, torch.arange(cols, device=gen.device)] = 2 * LC._ri(0, 1, (cols,), gen) - 1
    return w


def exact_mlp_bwd(B, C, H, V, dtype, seed=0, device="cpu"):
    """(g2, z1, x1, stats, γ, β, W1 (H, C), W2 (C, H)) of the module docstring; g2, z1, x1 of `dtype`"""
    _, x, stats, g, _ = exact_bwd(B, C, V, dtype, False, seed, device)
    gen = LC._gen(seed + 991 + H + 7 * V, device)
    g2 = LC._ri(-2, 2, (B, C, V), gen)
    z1 = 16 * (2 * LC._ri(0, 1, (B, H, V), gen) - 1)
    b = LC._ri(-2, 2, (C,), gen)
    w2, w1 = _one_per_column(C, H, gen), _one_per_column(H, C, gen)
    return g2.to(dtype).contiguous(), z1.to(dtype).contiguous(), x, stats, g, b, w1.contiguous(), w2.contiguous()


def exact_dw(B, V, dtype, ln, seed=0, device="cpu"):
    """(g, w, q, γ, β, stats, gadd) for fz_gemm_dw at C = 32: exact_dgrad's (gz, w2, x, stats, γ, gadd), β small integers"""
    gz, w2, _, x, stats, g, gadd = exact_dgrad(B, 32, 32, V, dtype, seed, device)
    b = LC._ri(-2, 2, (32,), LC._gen(seed + 5, device))
    return (gz, w2, x, g, b, stats, gadd) if ln else (gz, w2, x, None, None, None, None)


def check_exact(ref):
    """the conditions under which the float64 answer is the only correct one"""
    assert ref["representable"]
    for k, v in ref.items():
        if k.endswith("_terms"):
            assert float(v.max()) < 2 ** 22, k
    for k in ("gg", "gb", "gbt", "gw1", "gb1", "gw2", "gb2", "gw", "s", "s1"):
        if k in ref:
            assert torch.equal(ref[k].float().double(), ref[k]), k


# ------------------------------------------------------------------ rounded inputs -----------------------------------------
FAMILIES = ["randn", "mean_1000", "mean_30_std_half", "gelu_tails", "same_sign", "cancel", "g*2^-40", "g*2^40,w*2^-40"]


def _coherent(t):
    """|t| moved to the upper part of its bf16 rounding interval: hi = rne_bf16(|t|), value = hi + (0.5 .. 0.95) of half a unit
    of hi, so every lo = value − hi is positive and close to its largest size (the dropped lo·lo terms then all add up)"""
    hi = (t.abs() + 0.05).to(BF).double()
    frac = 0.5 + 0.45 * ((t.abs() * 1e3) % 1.0).double()
    return (hi + frac * half_ulp_bf16(hi, torch.zeros_like(hi))).float()


def rounded_chain(name, B, C, H, V, dtype, pre=False, head=0, head_bias=True, seed=0, device="cpu"):
    """dict x, g, b, w1, b1, w2, b2, g2 (+ a, wo, bo; + wh, bh): activations already rounded to `dtype`"""
    gen = LC._gen(seed + 31 * FAMILIES.index(name) + 1000 * C + H + V + 7 * B, device)
    rn = lambda *s: LC._rn(s, gen)
    x = rn(B, C, V) * 2 + 0.5
    if name == "mean_1000":
        x = 1000 + rn(B, C, V)
    if name == "mean_30_std_half":
        x = 30 + 0.5 * rn(B, C, V)
    p = {"g": torch.rand(C, generator=gen, device=device) + 0.5, "b": rn(C) * 0.1, "w1": rn(H, C) * 0.2, "b1": rn(H) * 0.1,
         "w2": rn(C, H) * 0.2, "b2": rn(C) * 0.1, "g2": rn(B, C, V)}
    if name == "gelu_tails":      # z1 = s_h x̂_c(h) + b1_h: every fourth row within 1e-3 of 0, the others out to ±12 (s = 4 at 3 σ)
        p["g"], p["b"] = torch.ones(C, device=device), torch.zeros(C, device=device)
        s = torch.where(torch.arange(H, device=device) % 4 == 0, 3e-4, 4.0)
        p["w1"] = torch.zeros((H, C), device=device)
        p["w1"][torch.arange(H, device=device), torch.arange(H, device=device) % C] = s
        p["b1"] = torch.where(torch.arange(H, device=device) % 4 == 0, 0.0, 1.0) * rn(H) * 0.5
    if name == "same_sign":
        p["g2"], p["w1"], p["w2"] = _coherent(p["g2"]), _coherent(p["w1"]), _coherent(p["w2"])
    if name == "cancel":          # a gradient drawn on its own: every voxel sum is about √n of its Σ|terms|
        p["g2"] = LC._rn((B, C, V), LC._gen(seed + 4242 + V + B, device))
    if pre:
        p["a"], p["wo"], p["bo"] = torch.relu(rn(B, C, V)) * 1.5, rn(C, C) * 0.2, rn(C) * 0.1
        if name == "same_sign":
            p["wo"] = _coherent(p["wo"])
    if head:
        p["wh"], p["bh"] = rn(head, C) * 0.2, (rn(head) if head_bias else None)
    p["x"] = x
    for k in ("x", "a", "g2"):
        if k in p:
            p[k] = p[k].to(dtype).contiguous()
    if name == "g*2^-40":
        p["g2"] = p["g2"] * 2.0 ** -40
    if name == "g*2^40,w*2^-40":
        p["g2"], p["w1"], p["w2"] = p["g2"] * 2.0 ** 40, p["w1"] * 2.0 ** -40, p["w2"] * 2.0 ** -40
    return {k: (v if v is None else v.contiguous()) for k, v in p.items()}


def rounded_dw(name, B, V, dtype, ln, seed=0, device="cpu"):
    """(g, w, q, γ, β, stats, gadd) for fz_gemm_dw at C = 32 (γ .. gadd None in the out_proj form)"""
    C = 32
    gen = LC._gen(seed + 57 * FAMILIES.index(name) + V + 7 * B + ln, device)
    rn = lambda *s: LC._rn(s, gen)
    q = {"mean_1000": lambda: 1000 + rn(B, C, V), "mean_30_std_half": lambda: 30 + 0.5 * rn(B, C, V)}.get(name, lambda: rn(B, C, V) * 1.5 + 0.3)()
    gr, w, gadd = rn(B, C, V), rn(C, C) * 0.2, rn(B, C, V)
    if name == "same_sign":
        gr, w, q = _coherent(gr), _coherent(w), _coherent(q)
    if name == "cancel":
        gr = LC._rn((B, C, V), LC._gen(seed + 4242 + V + B, device))
    gr, q, gadd = (t.to(dtype).contiguous() for t in (gr, q, gadd))
    if name == "g*2^-40":
        gr, gadd = gr * 2.0 ** -40, gadd * 2.0 ** -40
    if name == "g*2^40,w*2^-40":
        gr, w = gr * 2.0 ** 40, w * 2.0 ** -40
    if not ln:
        return gr, w.contiguous(), q, None, None, None, None
    g, b = torch.rand(C, generator=gen, device=device) + 0.5, rn(C) * 0.1
    return gr, w.contiguous(), q, g, b, stats_of(q), gadd


# ------------------------------------------------------------------ bounds (module docstring) -----------------------------
def _absmm(eq, a, b):
    return torch.einsum(eq, a.double().abs(), b.double().abs())


def _stored(ref, d, dtype):
    return d + half_ulp_bf16(ref, d) if dtype == BF else d


def two_level_rel(sum_mode, dtype):
    """(dn_rel, gadd_rel) of bwd_bounds: what the two-level arm of gemm_chain_bwd_wg_kernel reads back from its hi / lo planes"""
    if sum_mode != "two":
        return 0.0, 0.0
    return 2.0 ** -17, (2.0 ** -17 if dtype == torch.float32 else 0.0)


def depth_rows(ntiles):
    """mode 1, chain64, dgrad + LayerNorm backward: one partial row per tile into fz_reduce_rows"""
    return 1 + 5 + 2 + LC.rows_depth(ntiles, ntiles > 512)


def depth_carried(ntiles, rows):
    """mode 2, gemm_dw: accumulators carried over the tiles of a workgroup, rows added by the finish job"""
    return 64 * ((ntiles + rows - 1) // rows) + 2 + (rows + 15) // 16 + 16


def fwd_bounds(p, xin, ref, dtype, mode):
    """element-wise bounds around fwd64: dict x1 (PRE), mu, rs, z1, x2, logits.  xin: the tensor the LayerNorm reads (x, or the
    device's stored x1); ref = fwd64(p, x1_stored, x2_stored)"""
    C, H = xin.shape[1], p["w1"].shape[0]
    up = U_PROD[mode]
    d = {}
    if "a" in p:
        t0 = _absmm("mk,bkv->bmv", p["wo"], p["a"]) + (0 if p.get("bo") is None else _c(p["bo"]).abs()) + p["x"].double().abs()
        d["x1"] = SLACK * _stored(ref["x1"], ((C + 2) * U + up) * t0, dtype)
    one, zero = torch.ones(C, device=xin.device), torch.zeros(C, device=xin.device)
    d["mu"], d["rs"], dn = LC.fwd_bounds(xin, one, zero, torch.float32)
    n = (xin.double() - ref["mu"][:, None]) * ref["rs"][:, None]
    A = p["w1"].double() * p["g"].double().view(1, C)
    t1 = _absmm("hc,bcv->bhv", A, n) + (p["w1"].double().abs() @ p["b"].double().abs()).view(1, H, 1) + _c(p["b1"]).abs()
    dz = ((C + 3) * U + up) * t1 + torch.einsum("hc,bcv->bhv", A.abs(), dn) + U * ref["z1"].abs()
    d["z1"] = SLACK * _stored(ref["z1"], dz, dtype)
    ge = gelu64(ref["z1"])
    dge = GELU_LIP * dz + dgelu(ref["z1"].abs() + dz)
    t2 = _absmm("ch,bhv->bcv", p["w2"], ge) + _c(p["b2"]).abs() + xin.double().abs()
    dx2 = ((H + 3) * U + up) * t2 + torch.einsum("ch,bhv->bcv", p["w2"].double().abs(), dge) + U * ref["x2"].abs()
    d["x2"] = SLACK * _stored(ref["x2"], dx2, dtype)
    if "logits" in ref:
        t3 = _absmm("mc,bcv->bmv", p["wh"], ref["x2_read"]) + (0 if p.get("bh") is None else _c(p["bh"]).abs())
        d["logits"] = SLACK * _stored(ref["logits"], (C + 3) * U * t3, dtype)
    return d


def bwd_bounds(g2, z1, x1, stats, g, b, w1, w2, dtype, mode, sum_mode, depth, gz1_stored=True, dn_rel=0.0, gadd_rel=0.0):
    """bounds around bwd64, same keys.  mode: products of the two input-gradient GEMMs; sum_mode: those of the weight-gradient
    passes; depth: of the voxel sums; dn_rel: relative error of the x̂ the LayerNorm backward reads (two-level arm: 2^-17);
    gadd_rel: that of the residual g2 it adds (two-level arm with fp32 storage: 2^-17, `two_level_rel`)"""
    B, C, V = x1.shape
    H = w1.shape[0]
    ref = bwd64(g2, z1, x1, stats, g, b, w1, w2)
    zd, n, gh, gl = z1.double(), ref["n"], ref["gh"], ref["gl"]
    up, ups = U_PROD[mode], U_PROD[sum_mode]
    dgh = ((C - 1) * U + up) * _absmm("ch,bcv->bhv", w2, g2)
    dgz = gelu_grad64(zd).abs() * dgh + gh.abs() * dgelu_grad(zd) + U * ref["gz1"].abs()
    dgl = ((H - 1) * U + up) * _absmm("hc,bhv->bcv", w1, ref["gz1"]) + torch.einsum("hc,bhv->bcv", w1.double().abs(), dgz)
    dgx, _, _, _ = LC.bwd_bounds(gl, x1, stats, g, g2, torch.float32, 0)
    rs = stats[:, 1:2].double()
    da = dgl * _c(g).abs()
    a = gl * _c(g)
    extra = rs * (da + da.mean(1, keepdim=True) + n.abs() * (da * n.abs()).mean(1, keepdim=True))
    extra = extra + rs * dn_rel * ((n * (a * n).mean(1, keepdim=True)).abs() + n.abs() * (a * n).abs().mean(1, keepdim=True))
    extra = extra + gadd_rel * g2.double().abs()
    d = {"gz1": SLACK * (_stored(ref["gz1"], dgz, dtype) if gz1_stored else dgz),
         "gx1": SLACK * _stored(ref["gx1"], dgx / SLACK + extra, dtype)}
    S = lambda t: t.sum((0, 2))
    D = depth
    d["gb"] = SLACK * (D * U * ref["gb_terms"] + S(dgl))
    d["gg"] = SLACK * ((D + 3 + dn_rel / U) * U * ref["gg_terms"] + S(dgl * n.abs()))
    ub = 2.0 ** -17 if sum_mode == "two" else 0.0     # the bias sums run on the two bf16 planes too: one representation error
    d["gb2"] = SLACK * (D * U + ub) * ref["gb2_terms"]
    d["gb1"] = SLACK * ((D * U + ub) * ref["gb1_terms"] + S(dgz))
    d["gw2"] = SLACK * (((D + 2) * U + ups) * ref["gw2_terms"] + torch.einsum("bcv,bhv->ch", g2.double().abs(), dgelu(zd)))
    ds1 = ((D + 4) * U + ups) * ref["s1_terms"] + torch.einsum("bhv,bcv->hc", dgz, n.abs())
    gv, bv = g.double().abs().view(1, C), b.double().abs().view(1, C)
    d["gw1"] = SLACK * (gv * ds1 + bv * d["gb1"].view(H, 1) / SLACK
                        + 2 * U * ((gv * ref["s1"].abs()) + bv * ref["gb1"].abs().view(H, 1)))
    return d, ref


def dw_bounds(gr, w, q, ln, stats, gadd, dtype, depth):
    """bounds around dw64 (fz_gemm_dw multiplies on fp32 MFMAs whatever the products)"""
    B, C, V = q.shape
    ref = dw64(gr, w, q, ln, stats, gadd)
    dgl = C * U * _absmm("mk,bmv->bkv", w, gr)
    S = lambda t: t.sum((0, 2))
    D = depth
    d = {"gb": SLACK * D * U * ref["gb_terms"]}
    ds = (D + 4) * U * ref["s_terms"]
    if ln is None:
        d["y"] = SLACK * _stored(ref["y"], dgl + U * ref["y"].abs(), dtype)
        d["gw"] = SLACK * ds
        return d, ref
    n, gl = ref["n"], ref["gl"]
    dgx, _, _, _ = LC.bwd_bounds(gl, q, stats, ln[0], gadd, torch.float32, 0)
    rs = stats[:, 1:2].double()
    da = dgl * _c(ln[0]).abs()
    extra = rs * (da + da.mean(1, keepdim=True) + n.abs() * (da * n.abs()).mean(1, keepdim=True))
    d["y"] = SLACK * _stored(ref["y"], dgx / SLACK + extra, dtype)
    d["gbt"] = SLACK * (D * U * ref["gbt_terms"] + S(dgl))
    d["gg"] = SLACK * ((D + 3) * U * ref["gg_terms"] + S(dgl * n.abs()))
    gv, bv = ln[0].double().abs().view(1, C), ln[1].double().abs().view(1, C)
    d["gw"] = SLACK * (gv * ds + bv * d["gb"].view(C, 1) / SLACK + 2 * U * (gv * ref["s"].abs() + bv * ref["gb"].abs().view(C, 1)))
    return d, ref


# ------------------------------------------------------------------ fp32 emulation of the chain on the CPU -----------------
def _emm(w, x, mode, fewer=False):
    """w (M, K) against x (B, K, V) with emu_dot, (B, M, V)"""
    B, K, V = x.shape
    return emu_dot(w, x.float().permute(1, 0, 2).reshape(K, B * V), mode, fewer).view(-1, B, V).permute(1, 0, 2)


def emulate_fwd(p, dtype, mode, fewer=False):
    """the forward chain in fp32: dict x1 (PRE, stored), mu, rs, z1 (stored), x2 (stored), logits (stored)"""
    o = {}
    x = p["x"].float()
    if "a" in p:
        x = (_emm(p["wo"], p["a"], mode, fewer) + (0 if p.get("bo") is None else p["bo"].view(1, -1, 1)) + x).to(dtype)
        o["x1"] = x
    C = x.shape[1]
    mu, rs, n = LC.emulate_fwd(x, torch.ones(C), torch.zeros(C), torch.float32)
    o["mu"], o["rs"] = mu, rs
    z = _emm(p["w1"] * p["g"].view(1, C), n, mode, fewer) + (p["w1"] @ p["b"] + p["b1"]).view(1, -1, 1)
    o["z1"] = z.to(dtype)
    x2 = _emm(p["w2"], emu_gelu(z), mode, fewer) + p["b2"].view(1, -1, 1) + x.float()
    o["x2"] = x2.to(dtype)
    if "wh" in p:
        o["logits"] = (torch.einsum("mc,bcv->bmv", p["wh"], o["x2"].float()) + (0 if p.get("bh") is None else p["bh"].view(1, -1, 1))).to(dtype)
    return o


def _vsum(t):
    """a voxel sum in fp32: tiles of 256 columns, then the tiles in order"""
    R = t.shape[1]
    f = t.float().permute(1, 0, 2).reshape(R, -1)
    rows = torch.nn.functional.pad(f, (0, (-f.shape[1]) % TILE)).view(R, -1, TILE).sum(2)
    acc = torch.zeros(R)
    for r in range(rows.shape[1]):
        acc = acc + rows[:, r]
    return acc


def emulate_bwd(g2, z1, x1, stats, g, b, w1, w2, dtype, mode, sum_mode, fewer=False, sum_fewer=False):
    """the backward chain and its weight gradients in fp32, dict as bwd64"""
    B, C, V = x1.shape
    H = w1.shape[0]
    gh = _emm(w2.t(), g2, mode, fewer)
    gz = gh * emu_gelu_grad(z1.float())
    gl = _emm(w1.t(), gz, mode, fewer)
    gx, gg, gb = LC.emulate_bwd(gl, x1, stats, g, g2, dtype)
    n = (x1.float() - stats[:, 0:1]) * stats[:, 1:2]
    flat = lambda t: t.float().permute(1, 0, 2).reshape(t.shape[1], -1)
    o = {"gz1": gz.to(dtype), "gx1": gx, "gg": gg, "gb": gb, "gb2": _vsum(g2), "gb1": _vsum(gz)}
    o["gw2"] = emu_dot(flat(g2), flat(emu_gelu(z1.float())).t(), sum_mode, sum_fewer)
    s1 = emu_dot(flat(gz), flat(n).t(), sum_mode, sum_fewer)
    o["gw1"] = g.view(1, C) * s1 + b.view(1, C) * o["gb1"].view(H, 1)
    return o
