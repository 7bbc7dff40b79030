"""Oracle, inputs, bounds, seams and mutants of the weight-gradient tests (tests/test_wgrad_cpu.py: the tools checked on the
CPU; tests/test_gpu_wgrad.py: csrc/wgrad.hip, wgrad_fast_body.inc and the FK_WGRAD finish jobs of csrc/finish.h on the device).

Oracle (float64; P is (B, M, N), the inputs are (B, Cin, Vq))
  GW[m, k] = Σ_{b, n} gate(P)[b, m, n] · Q(In)[b, k, n],  gb[m] = Σ_{b, n} gate(P)[b, m, n],  each with its Σ|terms|.
  Q by index formula, one per loader (`q_operand`):
    plain    Q[k][n] = in[b, k, n]; two sources: channels [0, c0) from the first, [c0, Cin) from the second
    s2d      k = ((ci·2 + td)·2 + th)·2 + tw, n = (do·Ho + ho)·Wo + wo: in[b, ci, 2do + td, 2ho + th, 2wo + tw]
    k3       k = ci·27 + kd·9 + kh·3 + kw, n = (d·H + h)·W + w: in[b, ci, d + kd − 1, h + kh − 1, w + kw − 1], 0 outside
    s2d_2d   k = (ci·2 + th)·2 + tw on a (Ho, Wo) grid;  k3_2d  k = ci·9 + kh·3 + kw on an (H, W) grid
  Q prologues (plain loader): statistics (x − mean)·rstd from a (B, 2, N) tensor, then ReLU or erf-GELU.  P gate (`pmul`): ReLU
  (e > 0) or GELU'(e).  After the sum: the LayerNorm fold gw = γ_k·S[m, k] + β_k·gb[m], then `accumulate` onto a prior gw / gbias.

Exact inputs (`exact`): P, inputs, pmul integers in [-4, 4] drawn per position (a shifted, repeated or dropped tile changes the
  sum); statistics with means in {-1, 0, 1} and rstd in {1/2, 1, 2}, drawn per sample and per column; GELU and GELU' operands in
  {-16, +16}, where the library's own formula is exact in fp32 (mlp_cases.emu_gelu / emu_gelu_grad: gelu in {-0, 16}, gelu' in
  {0, 1}); γ, β in [-2, 2], priors in [-3, 3].  Every operand has at most 8 significant bits after its prologue (|(x − mean)·rstd|
  <= 10 in halves), so it is a bf16 number: exact under bf16 storage, in the first level of the three-level split and on the fp32
  pipe.  With Σ|terms| < 2^22 (checked per case on the CPU) every partial sum in any order is an fp32 number: the float64 answer is
  the only correct one, bit for bit, in all three product modes.

Rounded inputs (`rounded`): "randn"; "p*2^40,q*2^-40"; "same_sign" (mlp_cases._coherent: no cancellation, every dropped low
  part of a split has the same sign).

Bounds (`bounds`: a priori, element-wise, first order in u = 2^-24 times ln_cases.SLACK; nothing is tuned on a device)
  dS = ((D − 1) u + u_prod) Σ|p q| + Σ|p| dq + Σ dp |q|,   dgb = (D − 1) u Σ|p| + Σ dp
  u_prod   mlp_cases.U_PROD: fp32 MFMA u; three levels 2^-23 + 2^-32; bf16 storage: 0 (the product of two bf16 numbers is an
           fp32 number) — but a prologue result is rounded to bf16 before the bf16 MFMA (wgrad_kernel BF = 1: split_bf16x8 keeps
           `hi` only): half a unit of bf16 on that operand (ln_cases.half_ulp_bf16), in the dq resp. dp of dS alone — the
           bias sums add the fp32 value before that rounding (wgrad_kernel `psum[i] += x8[e]`), so dgb never carries it
  dq       statistics: 2u |q| (a difference, a product); GELU: mlp_cases.dgelu at |z| + dz plus 1.13 dz plus one more u |gelu|
           (the sum 1 + erf is rounded before the product); ReLU: nothing
  dp       ReLU gate: nothing (a select); GELU' gate: |p| mlp_cases.dgelu_grad(e) + u |p gelu'|
  D        depth of the sum behind one element, read from the kernels.  A wave adds the columns of its `tiles_per_chunk` tiles
           to one accumulator: 32 sequential terms a tile at worst, in every product mode; 4 waves: 2; then
           the finish form's tree (`finish_depth`, csrc/finish.h): 8-element form ceil(nchunk / 32) strided sequential terms, a
           4-way tree (2) and 32 groups in order; mid form ceil(nchunk / 4) + 2 + 2; wide forms ceil(nchunk / 4) + 1 + 2
           (counted as sequential: the worst case of any tree with that many leaves).  The bias sums are shallower than that.
  fold     gw = Σ_chunks (γ part + β pb): |γ| dS + |β| dgb + 3u (|γ| Σ|p q| + |β| Σ|p|);  accumulate: + u (|prior| + Σ|terms|)

Seams (`plan`): use_fast and pick_chunks of csrc/wgrad.hip and the `wide` choice of wgrad_finish_job restated; the chunk count
  also comes from the library itself, fz_wgrad_workspace_bytes / 4 = nchunk (M K + M) + M K + M (`lib_nchunk`), and
  tests/test_wgrad_cpu.py holds the two and the literal table REACHED together.  The finish form is NOT exported: the table's
  form is the restatement's alone, so the fin3_*_offset_is_wide1 cases show that an unaligned gw is exact, not which form ran
  (both forms are exact on them).  The seams are reached by the batch count at
  N in {4, 32, 36} wherever a kernel admits it (N = 96: three tiles a sample for the register-operand kernel, which takes
  whole tiles only), so the largest tensor of the table is below 10 MB.

Mutants (`MUTANTS`): oracle variants with one planted defect and the case that must expose each.  On the exact inputs the GELU'
  gate is in {0, 1} and so is the ReLU gate of the same operand: `gelu_gate_as_relu` is judged on its rounded case alone (as
  mlp_cases judges tanh_gelu)."""
import zlib

import torch

import ln_cases as LC
import mlp_cases as MC
from ln_cases import SLACK, U, fraction, half_ulp_bf16  # noqa: F401

BF = torch.bfloat16
TILE = 32
LOADERS = {"plain": 0, "s2d": 1, "k3": 2, "s2d_2d": 3, "k3_2d": 4}
RELU, GELU = 1, 2
# (storage, products): fp32 storage on the fp32 MFMAs / as six products of three bf16 levels, bf16 storage on plain bf16 MFMAs
MODES = {"fp32_mfma": (torch.float32, "fp32"), "fp32_split": (torch.float32, "three"), "bf16": (BF, "bf16")}
TILE_TERMS = 32        # sequential terms a tile adds to a wave's accumulator at worst, in every product mode
U_PROD = {"fp32": MC.U_PROD["fp32"], "three": MC.U_PROD["three"], "bf16": 0.0}


# ------------------------------------------------------------------ cases ---------------------------------------------------
class Case:
    """one weight-gradient problem.  grid: plain None; s2d the COARSE (Do, Ho, Wo); k3 (D, H, W); s2d_2d the coarse (Ho, Wo);
    k3_2d (H, W).  off: gw is a view that starts `off` floats into a larger buffer."""

    def __init__(self, name, loader="plain", B=1, M=32, Cin=32, N=32, grid=None, c0=0, stats=False, qact=0, pmul=0, ln=False,
                 gbias=True, acc=False, off=0):
        self.name, self.loader, self.B, self.M, self.Cin, self.c0 = name, loader, B, M, Cin, c0
        self.stats, self.qact, self.pmul, self.ln, self.gbias, self.acc, self.off = stats, qact, pmul, ln, gbias, acc, off
        self.D = self.H = self.W = self.Ho = self.Wo = 0
        if loader == "plain":
            self.K, self.N, self.Vq = Cin, N, N
        elif loader == "s2d":
            Do, self.Ho, self.Wo = grid
            self.D, self.H, self.W = 2 * Do, 2 * self.Ho, 2 * self.Wo
            self.K, self.N = 8 * Cin, Do * self.Ho * self.Wo
            self.Vq = 8 * self.N
        elif loader == "k3":
            self.D, self.H, self.W = grid
            self.K, self.N = 27 * Cin, self.D * self.H * self.W
            self.Vq = self.N
        elif loader == "s2d_2d":
            self.Ho, self.Wo = grid
            self.D, self.H, self.W = 1, 2 * self.Ho, 2 * self.Wo
            self.K, self.N = 4 * Cin, self.Ho * self.Wo
            self.Vq = 4 * self.N
        else:
            assert loader == "k3_2d"
            self.H, self.W = grid
            self.D = 1
            self.K, self.N = 9 * Cin, self.H * self.W
            self.Vq = self.N
        assert self.N % 4 == 0 and (loader == "plain" or not (c0 or stats or qact))
        assert not ln or stats, "the callers fold the LayerNorm affine behind its statistics"

    @property
    def nsrc(self):
        return 2 if self.c0 else 1

    def __repr__(self):
        return self.name


def _finish_cases():
    out = []
    # 8-element form (M K < 4096): strides 32 / 128 (fold) and 32 / 128 / 256; one 4-column tile per sample, nchunk = ceil(B / 4)
    for n in (1, 33, 97, 129, 257, 512):
        B = 4 * n - (2 if 1 < n < 512 else 0)            # (the last workgroup has two idle waves)
        out.append(Case(f"fin0_n{n}", B=B, M=3, Cin=32, N=4, stats=n == 97, acc=n in (33, 257)))
        out.append(Case(f"fin0_n{n}_fold", B=B, M=3, Cin=32, N=4, stats=True, ln=True, gbias=n not in (97, 512), acc=n == 129))
    # mid form (64 x 64, register-operand kernel): strides 4 / 16
    for n in (1, 4, 5, 16, 17):
        out.append(Case(f"fin2_n{n}", B=4 * n - 1, M=64, Cin=64, gbias=n not in (5, 17), acc=n in (5, 16)))
        out.append(Case(f"fin2_n{n}_fold", B=4 * n - 1, M=64, Cin=64, stats=True, ln=True, gbias=n != 4, acc=n == 17))
    # wide form, one element per thread (128 x 128): stride 4; above 64 chunks the mid form takes over (generic kernel, N = 36)
    for n in (1, 3, 4, 5, 64):
        out.append(Case(f"fin1_n{n}", B=4 * n, M=128, Cin=128, gbias=n != 3, acc=n == 5))
        out.append(Case(f"fin1_n{n}_fold", B=4 * n, M=128, Cin=128, stats=True, ln=True, gbias=n != 5, acc=n == 3))
    out.append(Case("fin1_n65_is_mid", B=130, M=128, Cin=128, N=36, stats=True, ln=True))
    # wide form, four elements per thread (256 x 256): stride 4; a 4-byte-offset gw falls back to one element per thread
    for n in (1, 3, 4, 5, 16):
        out.append(Case(f"fin3_n{n}", B=4 * n, M=256, Cin=256, gbias=n != 3, acc=n == 5))
        out.append(Case(f"fin3_n{n}_fold", B=4 * n, M=256, Cin=256, stats=True, ln=True, gbias=n != 5, acc=n == 3))
    out.append(Case("fin3_n5_offset_is_wide1", B=20, M=256, Cin=256, off=1))
    out.append(Case("fin3_n4_offset_is_wide1_fold", B=16, M=256, Cin=256, stats=True, ln=True, acc=True, off=1))
    return out


CASES = [
    # ---- blocks and tails, generic kernel
    Case("g32x32_m3_k32_n4", M=3, Cin=32, N=4),
    Case("g32x32_m1_k1_n4", B=2, M=1, Cin=1, N=4),
    Case("g32x64_m32_k40_n36", B=2, M=32, Cin=40, N=36),
    Case("g64x32_m33_k32_n32", B=3, M=33, Cin=32, N=32),
    Case("g64x64_m96_k80_n36", B=2, M=96, Cin=80, N=36),
    Case("g64x64_m33_k108_n4", B=5, M=33, Cin=108, N=4),
    # ---- blocks of the register-operand kernel
    Case("f_m64_k64", B=4, M=64, Cin=64),
    Case("f_m128_k64", B=4, M=128, Cin=64),
    Case("f_m64_k128", B=4, M=64, Cin=128),
    Case("f_m128_k128", B=2, M=128, Cin=128, N=64),
    # ---- just outside each term of use_fast, at a tile count where the two kernels are given different chunk counts
    Case("out_m96", B=516, M=96, Cin=64),
    Case("out_k80", B=516, M=64, Cin=80),
    Case("out_n36", B=514, M=64, Cin=64, N=36),
    Case("out_c0_12", B=1028, M=64, Cin=64, c0=12),
    Case("out_pmul", B=1028, M=64, Cin=64, pmul=RELU),
    Case("out_stats_relu", B=1028, M=64, Cin=64, stats=True, qact=RELU, ln=True),
    # ---- chunking, generic kernel (one 4-column tile per sample: tiles = B)
    Case("g_tiles1", B=1, M=3, Cin=32, N=4),
    Case("g_tiles3", B=3, M=3, Cin=32, N=4),
    Case("g_tiles4", B=4, M=3, Cin=32, N=4),
    Case("g_tiles5_idle_waves", B=5, M=3, Cin=32, N=4),
    Case("g_units_target", B=2048, M=3, Cin=32, N=4),
    Case("g_units_target+1", B=2049, M=3, Cin=32, N=4),
    Case("g_tpc3_crosses_samples", B=2049, M=3, Cin=32, N=36),
    # ---- chunking, register-operand kernel
    Case("f_tiles1", B=1, M=64, Cin=64),
    Case("f_tiles3", B=3, M=64, Cin=64),
    Case("f_tiles4", B=4, M=64, Cin=64),
    Case("f_tiles5_idle_waves", B=5, M=64, Cin=64),
    Case("f_units_target", B=1024, M=64, Cin=64),
    Case("f_units_target+1", B=1025, M=64, Cin=64),
    Case("f_tpc2_crosses_samples", B=342, M=64, Cin=64, N=96),
    Case("f_tpc3_m128", B=513, M=128, Cin=128),
    # ---- loaders.  s2d in the conv's role (P = gy, Q = s2d(x), bias sums) and the transposed conv's (P = x, Q = s2d(gy), none)
    Case("s2d_conv_122", "s2d", B=3, M=8, Cin=4, grid=(1, 2, 2)),
    Case("s2d_conv_226", "s2d", B=2, M=33, Cin=5, grid=(2, 2, 6)),
    Case("s2d_conv_342_wo2", "s2d", B=2, M=3, Cin=12, grid=(3, 4, 2)),
    Case("s2d_conv_344_two_tiles", "s2d", B=3, M=40, Cin=8, grid=(3, 4, 4)),
    Case("s2d_tconv_122", "s2d", B=3, M=4, Cin=8, grid=(1, 2, 2), gbias=False),
    Case("s2d_tconv_226", "s2d", B=2, M=5, Cin=4, grid=(2, 2, 6), gbias=False),
    Case("s2d_tconv_342_wo2", "s2d", B=2, M=12, Cin=3, grid=(3, 4, 2), gbias=False, acc=True),
    Case("k3_d1_w4_cin1", "k3", B=2, M=3, Cin=1, grid=(1, 3, 4)),
    Case("k3_w12_cin3", "k3", B=2, M=33, Cin=3, grid=(2, 3, 12)),
    Case("k3_w20_cin4", "k3", B=2, M=8, Cin=4, grid=(3, 2, 20)),
    Case("k3_w4_deep_cin4", "k3", B=1, M=32, Cin=4, grid=(5, 3, 4), gbias=False),
    Case("s2d_2d_14_cin1", "s2d_2d", B=2, M=1, Cin=1, grid=(1, 4)),
    Case("s2d_2d_22", "s2d_2d", B=3, M=3, Cin=2, grid=(2, 2)),
    Case("s2d_2d_66", "s2d_2d", B=2, M=33, Cin=10, grid=(6, 6)),
    Case("k3_2d_14", "k3_2d", B=3, M=3, Cin=1, grid=(1, 4)),
    Case("k3_2d_512", "k3_2d", B=2, M=33, Cin=4, grid=(5, 12)),
    # ---- prologues and the gate
    Case("f_stats", B=5, M=64, Cin=64, stats=True, ln=True),
    Case("f_stats_no_fold", B=5, M=128, Cin=64, stats=True),
    Case("f_gelu", B=5, M=64, Cin=128, qact=GELU),
    Case("f_relu", B=5, M=64, Cin=64, qact=RELU),
    Case("g_stats", B=3, M=32, Cin=40, N=36, stats=True, ln=True),
    Case("g_gelu", B=3, M=33, Cin=32, N=36, qact=GELU),
    Case("g_relu", B=3, M=32, Cin=40, N=36, qact=RELU),
    Case("g_stats_relu", B=3, M=33, Cin=40, N=36, stats=True, qact=RELU, ln=True),
    Case("g_pmul_relu", B=2, M=33, Cin=40, N=36, pmul=RELU),
    Case("g_pmul_gelu", B=2, M=33, Cin=40, N=36, pmul=GELU),
    Case("g_pmul_relu_m64_k64", B=5, M=64, Cin=64, pmul=RELU),
    Case("f_cat_c0_24", B=5, M=64, Cin=64, c0=24),
    Case("f_cat_c0_72_k128", B=5, M=64, Cin=128, c0=72, qact=RELU),
    Case("g_cat_c0_5", B=3, M=32, Cin=40, N=36, c0=5),
    Case("g_cat_c0_4", B=3, M=33, Cin=80, N=36, c0=4, qact=RELU),
    Case("g_cat_c0_12_stats", B=5, M=64, Cin=64, c0=12, stats=True, ln=True),
] + _finish_cases()
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)

# groups of fz_wgrad_group: (name, members); a member with B = 0 and one that is not fast turn the group into single launches
GROUPS = [
    ("grp2", [Case("grp2_a", B=5, M=64, Cin=64), Case("grp2_b", B=3, M=128, Cin=64, stats=True, ln=True)]),
    ("grp3", [Case("grp3_a", B=2, M=64, Cin=64, qact=GELU), Case("grp3_b", B=9, M=64, Cin=128, qact=RELU),
              Case("grp3_c", B=1, M=128, Cin=128, N=64, gbias=False)]),
    ("grp4", [Case("grp4_fc2", B=6, M=64, Cin=128, qact=GELU), Case("grp4_fc1", B=6, M=128, Cin=64, stats=True, ln=True),
              Case("grp4_out", B=3, M=64, Cin=64, N=96, acc=True), Case("grp4_in", B=1030, M=64, Cin=64, stats=True, ln=True)]),
    ("grp3_one_empty", [Case("grpe_a", B=5, M=64, Cin=64), Case("grpe_empty", B=0, M=64, Cin=64),
                        Case("grpe_c", B=3, M=128, Cin=64, qact=RELU)]),
    ("grp3_one_generic", [Case("grpg_a", B=5, M=64, Cin=64), Case("grpg_generic", B=3, M=33, Cin=40, N=36, stats=True, ln=True),
                          Case("grpg_c", B=3, M=128, Cin=64, c0=8)]),
]
GROUP_NAMES = [g[0] for g in GROUPS]

# where the rounded families run on the device: units_target + 1 and the sample-crossing walks of both kernels, every loader,
# every finish form, every prologue and gate
ROUNDED_AT = ["g_units_target+1", "f_units_target+1", "g_tpc3_crosses_samples", "f_tpc2_crosses_samples", "g64x64_m96_k80_n36",
              "s2d_conv_344_two_tiles", "s2d_tconv_226", "k3_w12_cin3", "s2d_2d_66", "k3_2d_512", "fin0_n257_fold", "fin2_n17_fold",
              "fin1_n5_fold", "fin3_n5_fold", "fin3_n4_offset_is_wide1_fold", "f_stats", "f_gelu", "g_gelu", "g_stats_relu",
              "g_pmul_gelu", "g_pmul_relu", "g_cat_c0_5", "f_cat_c0_24"]

# name -> (kernel, block, finish form, nchunk, tiles_per_chunk) each case reaches: tests/test_wgrad_cpu.py holds `plan`, the library's
# own chunk count and this list together, and asserts that every path of PATHS has a case
REACHED = {}    # filled below from _REACHED_TEXT


# ------------------------------------------------------------------ seams, restated from csrc/wgrad.hip --------------------
def blocks(c):
    return (64 if c.M > 32 else 32), (64 if c.K > 32 else 32)


def use_fast(c):
    PR, QR = blocks(c)
    c0 = c.c0 if c.c0 > 0 else c.Cin
    return (PR == 64 and QR == 64 and c.loader == "plain" and not c.pmul and c.M % PR == 0 and c.K % QR == 0
            and c.N % TILE == 0 and c.N == c.Vq and c0 % 8 == 0 and not (c.stats and c.qact) and 8 * c.N < 1 << 30)


def pick_chunks(total_tiles, out_blocks, fast):
    """(workgroups, tiles_per_chunk)"""
    units_target = max((1024 if fast else 2048) // max(out_blocks, 1), 16)
    tpc = max((total_tiles + units_target - 1) // units_target, 1)
    units = (total_tiles + tpc - 1) // tpc
    return (units + 3) // 4, tpc


def finish_form(M, K, nchunk, aligned=True):
    """`wide` of wgrad_finish_job: 0 = 8 elements a block, 2 = 64 x 4 slices, 1 = one per thread, 3 = four per thread"""
    MK = M * K
    wide = 1 if (nchunk <= 64 and MK >= 16384) else (2 if (nchunk <= 256 and MK >= 4096) else 0)
    if wide == 1 and MK >= 65536 and M % 4 == 0 and K % 4 == 0 and aligned:
        wide = 3
    return wide


def total_tiles(c):
    return ((c.N + TILE - 1) // TILE) * c.B


def plan(c, fast=None):
    """(kernel, block, wide, nchunk, tiles_per_chunk); fast: force the answer of use_fast (what the OTHER kernel would get)"""
    PR, QR = blocks(c)
    f = use_fast(c) if fast is None else fast
    ob = ((c.M + PR - 1) // PR) * ((c.K + QR - 1) // QR)
    nchunk, tpc = pick_chunks(total_tiles(c), ob, f)
    return ("fast" if f else "generic", f"{PR}x{QR}", finish_form(c.M, c.K, nchunk, c.off % 4 == 0), nchunk, tpc)


def desc_of(c):
    """the fz_wgrad_desc of a case with dummy non-null pointers (for the host-side entry points only)"""
    from factorizer_amd import _native
    d = _native.WgradDesc()
    d.p = d.q[0] = d.gw = 256
    if c.nsrc == 2:
        d.q[1] = 256
    if c.pmul:
        d.pmul, d.pmul_kind = 256, c.pmul
    if c.stats:
        d.stats = 256
    if c.ln:
        d.ln_g = d.ln_b = 256
    d.M, d.nsrc, d.c0, d.Cin, d.K, d.Vq, d.N, d.B = c.M, c.nsrc, c.c0, c.Cin, c.K, c.Vq, c.N, c.B
    d.D, d.H, d.W, d.Ho, d.Wo, d.qact, d.loader = c.D, c.H, c.W, c.Ho, c.Wo, c.qact, LOADERS[c.loader]
    d.act_dtype = _native.STORE_F32
    return d


def lib_nchunk(lib, c):
    """the library's chunk count, from fz_wgrad_workspace_bytes / 4 = nchunk (M K + M) + M K + M"""
    import ctypes
    by = int(lib.fz_wgrad_workspace_bytes(ctypes.byref(desc_of(c))))
    assert by > 0 and by % 4 == 0
    per = c.M * c.K + c.M
    assert (by // 4 - per) % per == 0
    return (by // 4 - per) // per


def finish_depth(wide, nchunk):
    if wide == 0:
        return (nchunk + 31) // 32 + 2 + 32
    if wide == 2:
        return (nchunk + 3) // 4 + 2 + 2
    return (nchunk + 3) // 4 + 1 + 2


def depth(c, mode):
    _, _, wide, nchunk, tpc = plan(c)
    return TILE_TERMS * tpc + 2 + finish_depth(wide, nchunk)


# ------------------------------------------------------------------ mutants -------------------------------------------------
MUTANTS = {   # mutant -> (exact case or None, rounded case)
    "partial_tile_dropped": ("g32x64_m32_k40_n36", "g32x64_m32_k40_n36"),
    "chunk_tile_dropped": ("g_units_target+1", "f_tpc2_crosses_samples"),
    "chunk_tile_doubled": ("f_units_target+1", "g_tpc3_crosses_samples"),
    "concat_off_by_one": ("g_cat_c0_5", "f_cat_c0_24"),
    "stats_sample0": ("f_stats", "g_stats"),
    "k3_clamped": ("k3_w12_cin3", "k3_2d_512"),
    "s2d_rows_reversed": ("s2d_conv_226", "s2d_tconv_226"),
    "fold_no_beta": ("fin2_n5_fold", "fin0_n33_fold"),
    "accumulate_ignored": ("fin1_n5", "fin2_n17_fold"),
    "bias_extra_kblock": ("g64x64_m96_k80_n36", "f_gelu"),
    "gelu_gate_as_relu": (None, "g_pmul_gelu"),
}


def tile_cols(c, t):
    tps = (c.N + TILE - 1) // TILE
    b, k = divmod(t, tps)
    return b, k * TILE, min(c.N, (k + 1) * TILE)


def _col_weights(c, mutant, device):
    """how often the sums count each column: 1, but for the tile mutants"""
    w = torch.ones((max(c.B, 1), 1, c.N), dtype=torch.float64, device=device)
    if mutant == "partial_tile_dropped":
        assert c.N % TILE
        w[:, :, c.N // TILE * TILE:] = 0
    if mutant in ("chunk_tile_dropped", "chunk_tile_doubled"):
        tpc = plan(c)[4]
        assert total_tiles(c) > tpc, "the chunk mutants need a second (workgroup, wave) unit"
        b, n0, n1 = tile_cols(c, tpc)                 # the first tile of the second unit
        w[b, :, n0:n1] = 0 if mutant == "chunk_tile_dropped" else 2
    return w


# ------------------------------------------------------------------ oracle --------------------------------------------------
def q_operand(c, qs, mutant=None):
    """(B, K, N) float64: the Q operand of the loader, before any prologue, by index formula"""
    xs = [t.double() for t in qs]
    if c.loader == "plain":
        if mutant == "concat_off_by_one":
            # the split taken at c0 - 1: rows [0, c0 - 1) from the first source, row k >= c0 - 1 is channel k - (c0 - 1) of the
            # second, whose last row then lies one channel past the sample (the next sample's channel 0; nothing after the last)
            past = torch.cat([xs[1][1:, :1], torch.zeros_like(xs[1][:1, :1])], 0)
            return torch.cat([xs[0][:, :c.c0 - 1], xs[1], past], 1)
        return torch.cat(xs, 1) if len(xs) == 2 else xs[0]
    dev = xs[0].device
    X = xs[0].reshape(xs[0].shape[0], c.Cin, c.Vq)
    k = torch.arange(c.K, device=dev).view(-1, 1)
    n = torch.arange(c.N, device=dev).view(1, -1)
    if c.loader in ("s2d", "s2d_2d"):
        taps = 8 if c.loader == "s2d" else 4
        ci, tap = k // taps, k % taps
        td, th, tw = ((tap >> 2) & 1 if taps == 8 else 0 * tap), (tap >> 1) & 1, tap & 1
        if mutant == "s2d_rows_reversed":
            assert taps == 8
            td, tw = tw, td
        wo, ho, do = n % c.Wo, (n // c.Wo) % c.Ho, n // (c.Wo * c.Ho)
        idx = ((2 * do + td) * c.H + 2 * ho + th) * c.W + 2 * wo + tw
        return X[:, ci.expand(-1, c.N), idx]
    nt = 27 if c.loader == "k3" else 9
    ci, tap = k // nt, k % nt
    kd, kh, kw = (tap // 9 if nt == 27 else 0 * tap + 1), (tap // 3) % 3, tap % 3
    w, h, d = n % c.W, (n // c.W) % c.H, n // (c.W * c.H)
    zd, zh, zw = d + kd - 1, h + kh - 1, w + kw - 1
    ok = (zd >= 0) & (zd < c.D) & (zh >= 0) & (zh < c.H) & (zw >= 0) & (zw < c.W)
    idx = (zd.clamp(0, c.D - 1) * c.H + zh.clamp(0, c.H - 1)) * c.W + zw.clamp(0, c.W - 1)
    Q = X[:, ci.expand(-1, c.N), idx]
    return Q if mutant == "k3_clamped" else Q * ok


def operands64(c, t, mutant=None):
    """(gated P, Q after its prologue), float64"""
    P = t["p"].double()
    if c.pmul == RELU:
        P = P * (t["pmul"].double() > 0)
    elif c.pmul == GELU:
        e = t["pmul"].double()
        P = P * ((e > 0).double() if mutant == "gelu_gate_as_relu" else MC.flush(MC.gelu_grad64(e)))
    Q = q_operand(c, t["q"], mutant)
    if c.stats:
        st = t["stats"].double()
        if mutant == "stats_sample0":
            st = st[:1].expand_as(st)
        Q = (Q - st[:, 0:1]) * st[:, 1:2]
    if c.qact == RELU:
        Q = Q.clamp_min(0)
    elif c.qact == GELU:
        Q = MC.flush(MC.gelu64(Q))
    return P, Q


def ref64(c, t, mutant=None):
    """dict s, gb_sum (the sums), gw, gb (after fold and accumulate) and the Σ|terms| of each as <name>_terms"""
    P, Q = operands64(c, t, mutant)
    Pw = P * _col_weights(c, mutant, P.device)
    o = {"s": torch.einsum("bmn,bkn->mk", Pw, Q), "s_terms": torch.einsum("bmn,bkn->mk", Pw.abs(), Q.abs()),
         "gb_sum": Pw.sum((0, 2)), "gb_sum_terms": Pw.abs().sum((0, 2))}
    if mutant == "bias_extra_kblock":
        assert c.K > 64
        o["gb_sum"] = 2 * o["gb_sum"]
    gw, gwt, gb, gbt = o["s"], o["s_terms"], o["gb_sum"], o["gb_sum_terms"]
    if c.ln:
        g, b = t["ln_g"].double().view(1, -1), t["ln_b"].double().view(1, -1)
        gwt = g.abs() * gwt + b.abs() * gbt.view(-1, 1)
        gw = g * gw + (0 if mutant == "fold_no_beta" else b * gb.view(-1, 1))
    if c.acc:
        gwt, gbt = gwt + t["gw0"].double().abs(), gbt + t["gb0"].double().abs()
        if mutant != "accumulate_ignored":
            gw, gb = gw + t["gw0"].double(), gb + t["gb0"].double()
    o.update(gw=gw, gw_terms=gwt, gb=gb, gb_terms=gbt)
    return o


def check_exact(c, t, ref):
    """the conditions under which the float64 answer is the only correct fp32 result"""
    P, Q = operands64(c, t)
    for x in (P, Q):                    # at most 8 significant bits: a bf16 number
        assert torch.equal(x.float().to(BF).double(), x), c.name
    for k in ("s_terms", "gb_sum_terms", "gw_terms", "gb_terms"):
        assert float(ref[k].max()) < 2 ** 22, (c.name, k, float(ref[k].max()))
    for k in ("s", "gb_sum", "gw", "gb"):
        assert torch.equal(ref[k].float().double(), ref[k]), (c.name, k)


# ------------------------------------------------------------------ inputs --------------------------------------------------
def _gen(c, salt=0):
    return torch.Generator().manual_seed(zlib.crc32(c.name.encode()) + salt)


def _q_shapes(c):
    B = max(c.B, 1)
    if c.nsrc == 2:
        return [(B, c.c0, c.Vq), (B, c.Cin - c.c0, c.Vq)]
    return [(B, c.Cin, c.Vq)]


def _finish_inputs(t, dtype, device):
    for k in ("p", "pmul"):
        if k in t:
            t[k] = t[k].to(dtype)
    t["q"] = [q.to(dtype) for q in t["q"]]
    mv = lambda v: v.to(device).contiguous()
    return {k: ([mv(q) for q in v] if k == "q" else mv(v)) for k, v in t.items()}


def exact(c, dtype, device="cpu"):
    """dict p, q (list), [pmul, stats, ln_g, ln_b, gw0, gb0]: p, q, pmul of `dtype` (module docstring)"""
    gen = _gen(c)
    ri = lambda lo, hi, s: torch.randint(lo, hi + 1, s, generator=gen).float()
    pm16 = lambda s: 16 * (2 * ri(0, 1, s) - 1)
    B = max(c.B, 1)
    t = {"p": ri(-4, 4, (B, c.M, c.N))}
    if c.pmul:
        t["pmul"] = ri(-4, 4, (B, c.M, c.N)) if c.pmul == RELU else pm16((B, c.M, c.N))
    t["q"] = [(pm16(s) if c.qact == GELU else ri(-4, 4, s)) for s in _q_shapes(c)]
    if c.stats:
        assert c.qact != GELU
        t["stats"] = torch.cat([ri(-1, 1, (B, 1, c.N)), 2.0 ** ri(-1, 1, (B, 1, c.N))], 1)
    if c.ln:
        t["ln_g"], t["ln_b"] = ri(-2, 2, (c.K,)), ri(-2, 2, (c.K,))
    if c.acc:
        t["gw0"], t["gb0"] = ri(-3, 3, (c.M, c.K)), ri(-3, 3, (c.M,))
    return _finish_inputs(t, dtype, device)


FAMILIES = ["randn", "p*2^40,q*2^-40", "same_sign"]


def rounded(c, family, dtype, device="cpu"):
    """as `exact`, the activations already rounded to `dtype` (the oracle sees what the kernel sees)"""
    gen = _gen(c, 1 + FAMILIES.index(family))
    rn = lambda *s: torch.randn(s, generator=gen)
    B = max(c.B, 1)
    t = {"p": rn(B, c.M, c.N)}
    if c.pmul:
        t["pmul"] = 1.5 * rn(B, c.M, c.N)
    t["q"] = [(1.5 * rn(*s) + 0.3 if c.qact == GELU else rn(*s)) for s in _q_shapes(c)]
    if family == "same_sign":
        t["p"], t["q"] = MC._coherent(t["p"]), [MC._coherent(q) for q in t["q"]]
    t["p"], t["q"] = t["p"].to(dtype), [q.to(dtype) for q in t["q"]]
    if c.stats:
        t["stats"] = LC.stats_of(torch.cat([q.float() for q in t["q"]], 1))
    if family == "p*2^40,q*2^-40":
        t["p"], t["q"] = t["p"] * 2.0 ** 40, [q * 2.0 ** -40 for q in t["q"]]
        if c.stats:         # the statistics of the scaled tensor (eps scaled with it): x̂ stays of order 1, S and β gb of one size
            t["stats"] = t["stats"] * torch.tensor([2.0 ** -40, 2.0 ** 40]).view(1, 2, 1)
    if c.ln:
        t["ln_g"], t["ln_b"] = 1 + 0.5 * rn(c.K), rn(c.K)
    if c.acc:
        scaled = family == "p*2^40,q*2^-40"      # priors of the size of what is added to them
        t["gw0"], t["gb0"] = 4 * rn(c.M, c.K) * (2.0 ** 40 if scaled and c.stats else 1), 4 * rn(c.M) * (2.0 ** 40 if scaled else 1)
    return _finish_inputs(t, dtype, device)


# ------------------------------------------------------------------ bounds (module docstring) ------------------------------
def bounds(c, t, mode, dtype):
    """(dict gw, gb of element-wise bounds around ref64(c, t), that reference)"""
    ref = ref64(c, t)
    P, Q = operands64(c, t)
    D, up = depth(c, mode), U_PROD[mode]
    dq, dp = torch.zeros_like(Q), torch.zeros_like(P)
    if c.stats:
        st = t["stats"].double()
        n = (q_operand(c, t["q"]) - st[:, 0:1]) * st[:, 1:2]
        dq = 2 * U * n.abs()
    if c.qact == GELU:
        z = q_operand(c, t["q"])
        dq = MC.GELU_LIP * dq + MC.dgelu(z.abs() + dq) + U * Q.abs()
    if c.pmul == GELU:
        e = t["pmul"].double()
        dp = t["p"].double().abs() * MC.dgelu_grad(e) + U * P.abs()
    dgb = (D - 1) * U * ref["gb_sum_terms"] + dp.sum((0, 2))      # (the bias sums add the gated P before any bf16 rounding)
    if dtype == BF:
        if c.stats or c.qact == GELU:
            dq = dq + half_ulp_bf16(Q, dq)
        if c.pmul == GELU:
            dp = dp + half_ulp_bf16(P, dp)
    mm = lambda a, b: torch.einsum("bmn,bkn->mk", a, b)
    ds = ((D - 1) * U + up) * ref["s_terms"] + mm(P.abs(), dq) + mm(dp, Q.abs()) + mm(dp, dq)
    dgw = ds
    if c.ln:
        g, b = t["ln_g"].double().abs().view(1, -1), t["ln_b"].double().abs().view(1, -1)
        dgw = g * ds + b * dgb.view(-1, 1) + 3 * U * (g * ref["s_terms"] + b * ref["gb_sum_terms"].view(-1, 1))
    if c.acc:
        dgw, dgb = dgw + U * ref["gw_terms"], dgb + U * ref["gb_terms"]
    return {"gw": SLACK * dgw, "gb": SLACK * dgb}, ref


# ------------------------------------------------------------------ fp32 emulation of the kernels on the CPU ---------------
def emulate(c, t, mode, dtype, fewer=False):
    """(gw, gb) in fp32: the prologues as the kernels compute them (mlp_cases.emu_gelu / emu_gelu_grad), the products as the
    mode multiplies (mlp_cases.emu_dot; bf16: operands rounded to bf16), sums in the order of the host's matmul.
    fewer (the mutant): one split level fewer."""
    P = t["p"].float()
    if c.pmul == RELU:
        P = torch.where(t["pmul"].float() > 0, P, torch.zeros_like(P))
    elif c.pmul == GELU:
        P = P * MC.emu_gelu_grad(t["pmul"].float())
    Q = q_operand(c, t["q"]).float()
    if c.stats:
        Q = (Q - t["stats"][:, 0:1]) * t["stats"][:, 1:2]
    if c.qact == RELU:
        Q = Q.clamp_min(0)
    elif c.qact == GELU:
        Q = MC.emu_gelu(Q)
    flat = lambda x: x.permute(1, 0, 2).reshape(x.shape[1], -1)
    gb = flat(P).sum(1)
    if mode == "bf16":
        s = flat(P.to(BF).float()) @ flat(Q.to(BF).float()).t()
    else:
        s = MC.emu_dot(flat(P), flat(Q).t(), mode, fewer)
    gw = s
    if c.ln:
        gw = t["ln_g"].view(1, -1) * s + t["ln_b"].view(1, -1) * gb.view(-1, 1)
    if c.acc:
        gw, gb = gw + t["gw0"], gb + t["gb0"]
    return gw, gb


# ------------------------------------------------------------------ the launch ---------------------------------------------
def launch_kwargs(c, t, gw, gb):
    """the keyword arguments of pointwise._wgrad / a problem of pointwise._wgrad_group"""
    kw = dict(B=c.B, M=c.M, Cin=c.Cin, K=c.K, Vq=c.Vq, Ncols=c.N, gbias=gb, c0=c.c0, qact=c.qact, loader=LOADERS[c.loader],
              D=c.D, H=c.H, W=c.W, Ho=c.Ho, Wo=c.Wo, accumulate=c.acc)
    if c.pmul:
        kw.update(pmul=t["pmul"], pmul_kind=c.pmul)
    if c.stats:
        kw["stats"] = t["stats"]
    if c.ln:
        kw["ln"] = (t["ln_g"], t["ln_b"])
    return kw


def outputs(c, t, device):
    """(gw, gbias or None): NaN, or the prior where the case accumulates; gw a view `off` floats into its buffer"""
    buf = torch.full((c.M * c.K + c.off,), float("nan"), device=device)
    gw = buf[c.off:].view(c.M, c.K)
    gb = torch.full((c.M,), float("nan"), device=device) if c.gbias else None
    if c.acc:
        gw.copy_(t["gw0"])
        if gb is not None:
            gb.copy_(t["gb0"])
    return gw, gb


# ------------------------------------------------------------------ the paths every table must reach -----------------------
_REACHED_TEXT = """
g32x32_m3_k32_n4 generic 32x32 0 1 1
g32x32_m1_k1_n4 generic 32x32 0 1 1
s2d_2d_14_cin1 generic 32x32 0 1 1
g32x64_m32_k40_n36 generic 32x64 0 1 1
g64x32_m33_k32_n32 generic 64x32 0 1 1
g64x64_m96_k80_n36 generic 64x64 2 1 1
g64x64_m33_k108_n4 generic 64x64 0 2 1
f_m64_k64 fast 64x64 2 1 1
f_m128_k64 fast 64x64 2 1 1
f_m64_k128 fast 64x64 2 1 1
f_m128_k128 fast 64x64 1 1 1
out_m96 generic 64x64 2 129 1
out_k80 generic 64x64 2 129 1
out_n36 generic 64x64 0 257 1
out_c0_12 generic 64x64 0 257 1
out_pmul generic 64x64 0 257 1
out_stats_relu generic 64x64 0 257 1
g_tiles1 generic 32x32 0 1 1
g_tiles3 generic 32x32 0 1 1
g_tiles4 generic 32x32 0 1 1
g_tiles5_idle_waves generic 32x32 0 2 1
g_units_target generic 32x32 0 512 1
g_units_target+1 generic 32x32 0 257 2
g_tpc3_crosses_samples generic 32x32 0 342 3
f_tiles1 fast 64x64 2 1 1
f_tiles3 fast 64x64 2 1 1
f_tiles4 fast 64x64 2 1 1
f_tiles5_idle_waves fast 64x64 2 2 1
f_units_target fast 64x64 2 256 1
f_units_target+1 fast 64x64 2 129 2
f_tpc2_crosses_samples fast 64x64 2 129 2
f_tpc3_m128 fast 64x64 1 43 3
s2d_conv_122 generic 32x32 0 1 1
s2d_conv_226 generic 64x64 0 1 1
s2d_conv_342_wo2 generic 32x64 0 1 1
s2d_conv_344_two_tiles generic 64x64 0 2 1
s2d_tconv_122 generic 32x64 0 1 1
s2d_tconv_226 generic 32x32 0 1 1
s2d_tconv_342_wo2 generic 32x32 0 1 1
k3_d1_w4_cin1 generic 32x32 0 1 1
k3_w12_cin3 generic 64x64 0 2 1
k3_w20_cin4 generic 32x64 0 2 1
k3_w4_deep_cin4 generic 32x64 0 1 1
s2d_2d_22 generic 32x32 0 1 1
s2d_2d_66 generic 64x64 0 1 1
k3_2d_14 generic 32x32 0 1 1
k3_2d_512 generic 64x64 0 1 1
f_stats fast 64x64 2 2 1
f_stats_no_fold fast 64x64 2 2 1
f_gelu fast 64x64 2 2 1
f_relu fast 64x64 2 2 1
g_stats generic 32x64 0 2 1
g_gelu generic 64x32 0 2 1
g_relu generic 32x64 0 2 1
g_stats_relu generic 64x64 0 2 1
g_pmul_relu generic 64x64 0 1 1
g_pmul_gelu generic 64x64 0 1 1
g_pmul_relu_m64_k64 generic 64x64 2 2 1
f_cat_c0_24 fast 64x64 2 2 1
f_cat_c0_72_k128 fast 64x64 2 2 1
g_cat_c0_5 generic 32x64 0 2 1
g_cat_c0_4 generic 64x64 0 2 1
g_cat_c0_12_stats generic 64x64 2 2 1
fin0_n1 generic 32x32 0 1 1
fin0_n1_fold generic 32x32 0 1 1
fin0_n33 generic 32x32 0 33 1
fin0_n33_fold generic 32x32 0 33 1
fin0_n97 generic 32x32 0 97 1
fin0_n97_fold generic 32x32 0 97 1
fin0_n129 generic 32x32 0 129 1
fin0_n129_fold generic 32x32 0 129 1
fin0_n257 generic 32x32 0 257 1
fin0_n257_fold generic 32x32 0 257 1
fin0_n512 generic 32x32 0 512 1
fin0_n512_fold generic 32x32 0 512 1
fin2_n1 fast 64x64 2 1 1
fin2_n1_fold fast 64x64 2 1 1
fin2_n4 fast 64x64 2 4 1
fin2_n4_fold fast 64x64 2 4 1
fin2_n5 fast 64x64 2 5 1
fin2_n5_fold fast 64x64 2 5 1
fin2_n16 fast 64x64 2 16 1
fin2_n16_fold fast 64x64 2 16 1
fin2_n17 fast 64x64 2 17 1
fin2_n17_fold fast 64x64 2 17 1
fin1_n1 fast 64x64 1 1 1
fin1_n1_fold fast 64x64 1 1 1
fin1_n3 fast 64x64 1 3 1
fin1_n3_fold fast 64x64 1 3 1
fin1_n4 fast 64x64 1 4 1
fin1_n4_fold fast 64x64 1 4 1
fin1_n5 fast 64x64 1 5 1
fin1_n5_fold fast 64x64 1 5 1
fin1_n64 fast 64x64 1 64 1
fin1_n64_fold fast 64x64 1 64 1
fin1_n65_is_mid generic 64x64 2 65 1
fin3_n1 fast 64x64 3 1 1
fin3_n1_fold fast 64x64 3 1 1
fin3_n3 fast 64x64 3 3 1
fin3_n3_fold fast 64x64 3 3 1
fin3_n4 fast 64x64 3 4 1
fin3_n4_fold fast 64x64 3 4 1
fin3_n5 fast 64x64 3 5 1
fin3_n5_fold fast 64x64 3 5 1
fin3_n16 fast 64x64 3 16 1
fin3_n16_fold fast 64x64 3 16 1
fin3_n5_offset_is_wide1 fast 64x64 1 5 1
fin3_n4_offset_is_wide1_fold fast 64x64 1 4 1
grp2_a fast 64x64 2 2 1
grp2_b fast 64x64 2 1 1
grp3_a fast 64x64 2 1 1
grp3_b fast 64x64 2 3 1
grp3_c fast 64x64 1 1 1
grp4_fc2 fast 64x64 2 2 1
grp4_fc1 fast 64x64 2 2 1
grp4_out fast 64x64 2 3 1
grp4_in fast 64x64 2 129 2
grpe_a fast 64x64 2 2 1
grpe_empty fast 64x64 2 0 1
grpe_c fast 64x64 2 1 1
grpg_a fast 64x64 2 2 1
grpg_generic generic 64x64 0 2 1
grpg_c fast 64x64 2 1 1
"""


def _parse_reached():
    for line in _REACHED_TEXT.strip().splitlines():
        name, kernel, blk, wide, nchunk, tpc = line.split()
        REACHED[name] = (kernel, blk, int(wide), int(nchunk), int(tpc))


_parse_reached()
ALL_CASES = CASES + [m for _, ms in GROUPS for m in ms]
PATHS = {
    "kernel x block": {("generic", "32x32"), ("generic", "32x64"), ("generic", "64x32"), ("generic", "64x64"), ("fast", "64x64")},
    "loader": set(LOADERS),
    "generic loader x block": {(l, b) for l in LOADERS for b in ("32x32", "64x64")},
    "finish form": {0, 1, 2, 3},
    "Q prologue x kernel": {(k, p) for k in ("generic", "fast") for p in ("none", "stats", "gelu", "relu")} | {("generic", "stats+relu")},
    "gate": {0, RELU, GELU},
}


def prologue_of(c):
    return {(False, 0): "none", (True, 0): "stats", (False, GELU): "gelu", (False, RELU): "relu", (True, RELU): "stats+relu"}[(c.stats, c.qact)]


def reached_paths(cases):
    got = {k: set() for k in PATHS}
    for c in cases:
        kernel, blk, wide, _, _ = plan(c)
        got["kernel x block"].add((kernel, blk))
        got["loader"].add(c.loader)
        if kernel == "generic":
            got["generic loader x block"].add((c.loader, blk))
        got["finish form"].add(wide)
        got["Q prologue x kernel"].add((kernel, prologue_of(c)))
        got["gate"].add(c.pmul)
    return got
