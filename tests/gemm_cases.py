"""Oracle, inputs, bounds, case table and mutants of the fz_gemm tests (tests/test_gemm_cpu.py: the tools, the form table and the
refusals checked on the CPU; tests/test_gpu_gemm.py: every kernel form fz_gemm's dispatcher can launch, on the device).

Oracle (float64, from include/factorizer_hip.h; activations are (B, C, V))
  Out[b, m, n] = epilogue( Σ_k A[m, k] · prologue(In)[b, k, n] )
  In        by index formula, one per loader (wgrad_cases.q_operand: the two entry points share their loaders): plain with one
            source or two concatenated at c0, s2d, k3, s2d_2d, k3_2d
  prologue  LayerNorm over the Cin channels (two-pass statistics; `stats_out` = mean, rstd), then GELU (erf) or ReLU, or the ReLU
            gate In · (bmul > 0)
  A         w_t ? w[k · ldw + m] : w[m · ldw + k], ldw >= the row length
  epilogue  plain: + bias[m], (LayerNorm β: + Σ_k A[m, k] β[k], part of the sum), eact, · act'(emul) by emul_kind, + res
            d2s: + bias[m / 8], rows (o, td, th, tw) scattered to the fine grid, + res on the fine grid;  d2s_2d: bias[m / 4]
            lnbwd: gl = the sum; y = LayerNorm backward of gl (ln_cases.bwd64) [+ lnb_gadd]; (gγ | gβ) partial rows, summed in
            row order (their count is fz_gemm_lnbwd_partials)
  storage   bf16: the oracle reads the stored values and its result is rounded once to bf16 (ln_cases.store)
  Every sum also returns its Σ|terms|.

Exact inputs (`exact`): x, w, bias, res, bmul and a ReLU emul are integers in [-4, 4] (at most 8 significant bits: bf16
  numbers, so the first level of the three-level split is the value and bf16 storage holds them); the GELU prologue's operand
  and a GELU emul are in {-16, +16}, where the library's formula gives gelu in {-0, 16} and gelu' in {0, 1} in fp32
  (mlp_cases.emu_gelu).  Σ|terms| + |bias| + |res| < 2^22 (`check_exact`): every partial sum in any order, tile and product mode is
  an fp32 number and the float64 answer the only correct one.  LayerNorm has no exact family (rstd is irrational); the lnbwd
  cases take ln_cases.exact_dgrad.  eact = GELU is judged on rounded inputs only (its operand is the sum).

Rounded inputs (`rounded`): "randn"; "same_sign" (mlp_cases._coherent); "w*2^40,x*2^-40"; "mean_1000" (LayerNorm cases only).

Bounds (`bounds`; a priori, element-wise, first order in u = 2^-24, times ln_cases.SLACK; nothing is fitted to a device)
  sum       ((K + 3) u + u_prod) Σ_k |A| |In'| + Σ_k |A| dIn': K terms in ANY order cost at most (K − 1) u — that covers the 32-term
            tiles, the four partial sums of the K-split forms and the chunk order —, the bias, the LayerNorm fold of γ into the
            staged weight and the final operation one u each.  u_prod: mlp_cases.U_PROD (fp32 MFMA u; three levels 2^-23 + 2^-32).
            bf16 storage: the split family multiplies a one-level activation (or a three-level prologue result, gemm_bx.h
            bx_terms_b) by three-level weights — never worse than the three-level figure, which is the one used.
  dIn'      GELU: mlp_cases.dgelu at |z| + dz plus 1.13 dz plus u |gelu|; ReLU and the gate: nothing (selects)
  LayerNorm two evaluation orders exist; the bound is the one of the form the case reaches (`ln_order`, from REACHED):
            two-pass (resident kernel, p32): x̂ with ln_cases.fwd_bounds (γ = 1, β = 0) as dIn' of the sum over A γ;
            pivoted one-pass (streaming forms, split and fp32): rs (S − m s) + t with d = x − x[channel 0], S = Σ_k A γ d,
            s = Σ_k A γ, m = mean(d), t = Σ_k A β.  NEW TERM: dS = ((K + 3) u + u_prod) Σ|A γ||d|, ds = (K + 1) u Σ|A γ|,
            dm as ln_cases.stats_bounds, so d(S − m s) = dS + |m| ds + |s| dm + 2u |m s| + u |S − m s| — the cancellation of S
            against m s is paid for with |m| Σ|A γ| (the mean of d, not of x: the pivot removes a common offset) — then
            times rs (1 + drs / rs + u), plus (K + 1) u Σ|A β| for t.
            stats_out: ln_cases.stats_bounds.
  epilogue  eact GELU: dgelu; emul GELU: |v| mlp_cases.dgelu_grad(e) + u |v gelu'|; each further operation u of its result
  d2s       the scatter moves values only
  lnbwd     mlp_cases' derivation: ln_cases.bwd_bounds of the exact gl plus what dgl moves, depth 12 (4 columns in a lane 3,
            half_sum32 5, 4 waves 2, two spare; the rows are added in float64 by the test)
  bf16      + ln_cases.half_ulp_bf16 at the stored result

Forms (`FORMS`): every kernel form the launchers of csrc/gemm.hip, gemm_bx.hip, gemm_bxk.hip, gemm_stream.hip, gemm_p32.hip,
  mlp_chain64.hip (chain64_lnb_launch) and headbwd.hip (fz_head_fwd) can select, one line per form, written from the launch
  macros.  The form a case reaches is NOT restated here: it is asked of the library (fz_gemm_plan, the dispatcher's own dry
  run; `plan`), recorded next to the case in _REACHED_TEXT and held to the library's answer by tests/test_gemm_cpu.py, which also
  asserts that the table reaches all of FORMS.

Mutants (`MUTANTS`): oracle variants with one planted defect, the exact case that must differ and the rounded case that must
  leave its bound.  NO_EXACT lists the mutants without an exact case, with the reason."""
import ctypes
import zlib

import torch

import ln_cases as LC
import mlp_cases as MC
import wgrad_cases as W
from ln_cases import SLACK, U, fraction, half_ulp_bf16, store  # noqa: F401

BF = torch.bfloat16
LOADERS = W.LOADERS
EPIS = {"plain": 0, "d2s": 1, "lnbwd": 2, "d2s_2d": 3}
RELU, GELU = 1, 2
# mode -> (storage, products name, FZ_PRODUCTS_* value).  bf16 storage runs with the split family asked for by name, so that
# the process default (environment) cannot change which form a case reaches
MODES = {"fp32_mfma": (torch.float32, "fp32", 2), "fp32_split": (torch.float32, "three", 1), "bf16": (BF, "three", 1),
         "bf16_mfma": (BF, "fp32", 2)}     # (bf16 storage on the fp32 MFMA kernels: given to every case that lists fp32_mfma and bf16)
U_PROD = {"fp32": MC.U_PROD["fp32"], "three": MC.U_PROD["three"]}
PTR = 4096        # a dummy pointer: non-null, 16-byte aligned, never dereferenced by fz_gemm_plan


class Case:
    """one fz_gemm problem.  grid: plain None (N columns); s2d / d2s the COARSE (Do, Ho, Wo); k3 (D, H, W); s2d_2d / d2s_2d the
    coarse (Ho, Wo); k3_2d (H, W).  pad: ldw = row length + pad.  emul: the emul_kind (0 = no emul tensor)."""

    def __init__(self, name, loader="plain", epi="plain", B=1, M=32, Cin=32, N=None, grid=None, c0=0, ln=False, stats=False,
                 bact=0, bmul=False, eact=0, emul=None, res=False, bias=True, w_t=0, pad=0, gadd=False, tune=0, modes=None):
        self.name, self.loader, self.epi, self.B, self.M, self.Cin, self.c0 = name, loader, epi, B, M, Cin, c0
        self.ln, self.stats, self.bact, self.bmul, self.eact, self.emul, self.res = ln, stats, bact, bmul, eact, emul, res
        self.bias, self.w_t, self.pad, self.gadd, self.tune = bias and epi != "lnbwd", w_t, pad, gadd, tune
        self.modes = tuple(modes or MODES)
        if "fp32_mfma" in self.modes and "bf16" in self.modes and "bf16_mfma" not in self.modes:
            self.modes += ("bf16_mfma",)
        self.D = self.H = self.W = self.Ho = self.Wo = 0
        if loader == "plain":
            self.K = Cin
            if epi == "d2s":
                Do, self.Ho, self.Wo = grid
                N = Do * self.Ho * self.Wo
            elif epi == "d2s_2d":
                self.Ho, self.Wo = grid
                N = self.Ho * self.Wo
            self.N = self.Vq = N
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
        self.grid = grid
        self.ldw = (self.M if w_t else self.K) + pad
        self.taps = {"d2s": 8, "d2s_2d": 4}.get(epi, 1)
        assert not stats or ln
        assert not (ln and bact) and not (bmul and (ln or bact)), "refused by fz_gemm"

    @property
    def nsrc(self):
        return 2 if self.c0 else 1

    @property
    def yshape(self):
        return (max(self.B, 1), self.M // self.taps, self.N * self.taps)

    def __repr__(self):
        return self.name


# ------------------------------------------------------------------ the library's own answer --------------------------------
def desc_of(c, mode, ptrs=None):
    """fz_gemm_desc of a case from its shapes alone; ptrs: name -> address (the device run), else dummy aligned pointers"""
    from factorizer_amd import _native
    p = (lambda k: ptrs[k]) if ptrs is not None else (lambda k: PTR)
    dtype, _, products = MODES[mode]
    d = _native.GemmDesc()
    d.x[0] = p("x0")
    if c.nsrc == 2:
        d.x[1] = p("x1")
    d.nsrc, d.src_mode, d.c0, d.Cin, d.Vin = c.nsrc, 0, c.c0, c.Cin, c.Vq
    d.Di, d.Hi, d.Wi = c.D, c.H, c.W
    d.w, d.w_t, d.ldw, d.M, d.K = p("w"), c.w_t, c.ldw, c.M, c.K
    if c.bias:
        d.bias = p("bias")
    if c.ln:
        d.ln, d.ln_g, d.ln_b, d.ln_eps = 1, p("ln_g"), p("ln_b"), LC.EPS
    if c.stats:
        d.stats_out = p("stats")
    d.bact = c.bact
    if c.bmul:
        d.bmul, d.bmul_kind = p("bmul"), RELU
    d.eact = c.eact
    if c.res:
        d.res = p("res")
    if c.emul is not None:
        d.emul, d.emul_kind = p("emul"), c.emul
    d.y, d.Ncol, d.Ho, d.Wo, d.B = p("y"), c.N, c.Ho, c.Wo, c.B
    d.loader, d.epilogue = LOADERS[c.loader], EPIS[c.epi]
    if c.epi == "lnbwd":
        d.lnb_x, d.lnb_stats, d.lnb_g, d.lnb_part = p("lnb_x"), p("lnb_stats"), p("lnb_g"), p("lnb_part")
        if c.gadd:
            d.lnb_gadd = p("lnb_gadd")
    d.act_dtype = _native.STORE_BF16 if dtype == BF else _native.STORE_F32
    d.products, d.tune = products, c.tune
    return d


def plan_desc(lib, d):
    """(return code, form string) of fz_gemm_plan"""
    buf = ctypes.create_string_buffer(192)
    rc = lib.fz_gemm_plan(ctypes.byref(d), buf, 192)
    return rc, buf.value.decode()


def form_of(text):
    """the form proper: the string without the launch geometry (the key=value tokens) and without `wt` — the split family
    compiles every form for both weight layouts, and the table asks for both only where the issue does: the streaming
    form's two s2d tiles"""
    tok = [t for t in text.split() if "=" not in t]
    return " ".join(t for t in tok if t != "wt" or (tok[0] == "bx_stream" and "s2d" in tok))


def grid_of(text):
    g = [t for t in text.split() if t.startswith("grid=")][0][5:].split("x")
    return int(g[0]), int(g[1])


def plan(lib, c, mode):
    rc, text = plan_desc(lib, desc_of(c, mode))
    assert rc == 0, (c.name, mode, rc, lib.fz_last_error_string())
    return text


# ------------------------------------------------------------------ oracle --------------------------------------------------
MUTANTS = {   # mutant -> (exact case or None, rounded case)
    "s2d_taps_swapped": ("bx_s2d_mb1", "str_s2d"),
    "d2s_bias_by_m": ("bx_d2s_mb1_n2", "res_d2s_k32"),
    "res_before_eact": ("res_pf0_relu_res", "res_pf0_relu_res"),
    "emul_before_eact": (None, "bxk_emul_gelu"),
    "emul_kind_ignored": ("bxk_emul_gelu", "bxk_emul_gelu"),
    "c0_off_by_one": ("bx_c0_16", "res_c0_k15"),
    "w_t_ignored": ("bx_plain_mb1_n2_wt", "res_k2_m1"),
    "ldw_as_k": ("bx_plain_mb2_n2", "res_k16_m40"),
    "last_col_dropped": ("bx_tile_plus4", "res_n516"),
    "last_rowblock_dropped": ("bx_m96", "res_m288"),
    "k3_clamped": ("str_k3_mb1", "str_k3_2d_mb1"),
    "ln_beta_w_dropped": (None, "bx_ln_mb1"),
    "stats_rstd_as_var": (None, "res_pf2_stats"),
    "gelu_as_relu": (None, "bx_gelu_mb1_n2"),
}
NO_EXACT = {
    "emul_before_eact": "on the exact inputs every gate is 0 or 1 and commutes with the ReLU; eact = GELU has no exact family",
    "ln_beta_w_dropped": "LayerNorm has no exact family (rstd is irrational)",
    "stats_rstd_as_var": "LayerNorm has no exact family (rstd is irrational)",
    "gelu_as_relu": "on the exact operands ±16 GELU and ReLU agree (gelu(-16) = -0): that is what makes them exact",
}


def _weights(c, t, mutant=None):
    """A (M, K), float64"""
    w = t["w"].double()
    if mutant == "w_t_ignored":
        assert c.w_t
        flat = w.reshape(-1)
        idx = (torch.arange(c.M, device=w.device).view(-1, 1) * c.ldw + torch.arange(c.K, device=w.device).view(1, -1)) % flat.numel()
        return flat[idx]
    if mutant == "ldw_as_k":
        assert not c.w_t and c.pad
        return w.reshape(-1)[:c.M * c.K].view(c.M, c.K)
    return w[:, :c.M].t() if c.w_t else w[:, :c.K]


def operand64(c, t, mutant=None):
    """dict: X the operand after its prologue (B, K, N); mu, rs of the LayerNorm prologue; raw the operand before it"""
    wm = {"s2d_taps_swapped": "s2d_rows_reversed", "c0_off_by_one": "concat_off_by_one", "k3_clamped": "k3_clamped"}.get(mutant)
    raw = W.q_operand(c, t["x"], wm)
    o = {"raw": raw, "X": raw}
    if c.ln:
        mu = raw.mean(1, keepdim=True)
        rs = (((raw - mu) ** 2).mean(1, keepdim=True) + LC.EPS).rsqrt()
        o.update(mu=mu, rs=rs, X=(raw - mu) * rs)
    if c.bact == GELU:
        o["X"] = o["X"].clamp_min(0) if mutant == "gelu_as_relu" else MC.flush(MC.gelu64(o["X"]))
    elif c.bact == RELU:
        o["X"] = o["X"].clamp_min(0)
    if c.bmul:
        o["X"] = o["X"] * (t["bmul"].double() > 0)
    return o


def _act(kind, v):
    return v.clamp_min(0) if kind == RELU else (MC.flush(MC.gelu64(v)) if kind == GELU else v)


def _act_grad(kind, e):
    return (e > 0).double() if kind == RELU else (MC.flush(MC.gelu_grad64(e)) if kind == GELU else torch.ones_like(e))


def scatter(c, acc):
    """rows (o, taps) x coarse columns -> (B, O, fine voxels)"""
    B = acc.shape[0]
    if c.epi == "d2s":
        Do, Ho, Wo = c.grid
        return acc.reshape(B, c.M // 8, 2, 2, 2, Do, Ho, Wo).permute(0, 1, 5, 2, 6, 3, 7, 4).reshape(B, c.M // 8, 8 * c.N)
    Ho, Wo = c.grid
    return acc.reshape(B, c.M // 4, 2, 2, Ho, Wo).permute(0, 1, 4, 2, 5, 3).reshape(B, c.M // 4, 4 * c.N)


def ref64(c, t, mutant=None):
    """dict y (float64, before the storage rounding), terms (Σ|terms| behind y, same shape), acc / acc_terms (the sum alone),
    [mu, rs], [lnbwd: gg, gb and their terms]"""
    op = operand64(c, t, mutant)
    A, X = _weights(c, t, mutant), op["X"]
    if c.ln:
        g, b = t["ln_g"].double(), t["ln_b"].double()
        Ag = A * g.view(1, -1)
        acc = torch.einsum("mk,bkn->bmn", Ag, X)
        terms = torch.einsum("mk,bkn->bmn", Ag.abs(), X.abs())
        if mutant != "ln_beta_w_dropped":
            acc = acc + (A @ b).view(1, -1, 1)
            terms = terms + (A.abs() @ b.abs()).view(1, -1, 1)
    else:
        acc = torch.einsum("mk,bkn->bmn", A, X)
        terms = torch.einsum("mk,bkn->bmn", A.abs(), X.abs())
    if mutant == "last_col_dropped":
        acc = acc.clone()
        acc[:, :, -1] = 0
    if mutant == "last_rowblock_dropped":
        assert c.M > 32
        acc = acc.clone()
        acc[:, (c.M - 1) // 32 * 32:] = 0
    o = {"acc": acc, "acc_terms": terms}
    if c.ln:
        o["mu"], o["rs"] = op["mu"][:, 0], (op["rs"][:, 0] ** -2 - LC.EPS if mutant == "stats_rstd_as_var" else op["rs"][:, 0])
    if c.epi == "lnbwd":
        r = LC.bwd64(acc, t["lnb_x"], t["lnb_stats"], t["lnb_g"], t.get("lnb_gadd"))
        o.update(y=r["gx"], gg=r["gg"], gb=r["gb"], gg_terms=r["gg_terms"], gb_terms=r["gb_terms"], terms=None)
        return o
    v = acc
    if c.bias:
        bias = t["bias"].double()
        if mutant == "d2s_bias_by_m":
            assert c.taps > 1
            bm = bias[torch.arange(c.M, device=bias.device) % bias.numel()]
        else:
            bm = bias.repeat_interleave(c.taps)
        v, terms = v + bm.view(1, -1, 1), terms + bm.abs().view(1, -1, 1)
    if c.taps > 1:
        v, terms = scatter(c, v), scatter(c, terms)
        if c.res:
            v, terms = v + t["res"].double(), terms + t["res"].double().abs()
        o.update(y=v, terms=terms, pre=None)
        return o
    res = t["res"].double() if c.res else None
    if mutant == "res_before_eact":
        v = v + res
    o["pre"] = v                    # the operand of eact
    if c.emul is not None and mutant == "emul_before_eact":
        v = _act(c.eact, v * _act_grad(c.emul, t["emul"].double()))
    else:
        v = _act(c.eact, v)
        if c.emul is not None and mutant != "emul_kind_ignored":
            v = v * _act_grad(c.emul, t["emul"].double())
    if c.res and mutant != "res_before_eact":
        v = v + res
        terms = terms + res.abs()
    o.update(y=v, terms=terms)
    return o


def stored(c, ref, dtype):
    """the tensor fz_gemm must leave in y"""
    return store(ref["y"], dtype)


def check_exact(c, t, ref):
    """the conditions under which the float64 answer is the only correct result in every product mode"""
    assert not c.ln and c.eact != GELU, c.name
    if c.epi == "lnbwd":
        gl = ref["acc"]
        assert float(gl.abs().max()) <= 2 and torch.equal(gl, gl.round()), c.name
        assert torch.equal(ref["y"].float().double(), ref["y"]), c.name
        return
    X, A = operand64(c, t)["X"], _weights(c, t)
    for x in (X, A):
        assert torch.equal(x.float().to(BF).double(), x), c.name
    assert float(ref["terms"].max()) < 2 ** 22, (c.name, float(ref["terms"].max()))
    for k in ("acc", "y"):
        assert torch.equal(ref[k].float().double(), ref[k]), (c.name, k)


# ------------------------------------------------------------------ inputs --------------------------------------------------
def _gen(c, salt=0):
    return torch.Generator().manual_seed(zlib.crc32(c.name.encode()) + salt)


def _x_shapes(c):
    B = max(c.B, 1)
    if c.nsrc == 2:
        return [(B, c.c0, c.Vq), (B, c.Cin - c.c0, c.Vq)]
    return [(B, c.Cin, c.Vq)]


def _w_shape(c):
    return (c.K if c.w_t else c.M, c.ldw)


def _res_shape(c):
    return c.yshape


ACT_KEYS = ("bmul", "emul", "res", "lnb_x", "lnb_gadd")


def _finish(t, dtype, device):
    t["x"] = [x.to(dtype) for x in t["x"]]
    for k in ACT_KEYS:
        if t.get(k) is not None:
            t[k] = t[k].to(dtype)
    mv = lambda v: v.to(device).contiguous()
    return {k: ([mv(x) for x in v] if k == "x" else mv(v)) for k, v in t.items() if v is not None}


def exact(c, dtype, device="cpu"):
    gen = _gen(c)
    ri = lambda lo, hi, s: torch.randint(lo, hi + 1, s, generator=gen).float()
    pm16 = lambda s: 16 * (2 * ri(0, 1, s) - 1)
    B = max(c.B, 1)
    if c.epi == "lnbwd":
        gz, w2, _, x, st, g, gadd = LC.exact_dgrad(B, c.M, c.K, c.N, torch.float32, seed=zlib.crc32(c.name.encode()) % 1000)
        assert c.w_t and not c.pad
        t = {"x": [gz], "w": w2, "lnb_x": x, "lnb_stats": st, "lnb_g": g, "lnb_gadd": gadd if c.gadd else None}
        return _finish(t, dtype, device)
    t = {"x": [(pm16(s) if c.bact == GELU else ri(-4, 4, s)) for s in _x_shapes(c)], "w": ri(-4, 4, _w_shape(c))}
    if c.bias:
        t["bias"] = ri(-3, 3, (c.M // c.taps,))
    if c.bmul:
        t["bmul"] = ri(-4, 4, (B, c.Cin, c.N))
    if c.emul is not None:
        t["emul"] = pm16((B, c.M, c.N)) if c.emul == GELU else ri(-4, 4, (B, c.M, c.N))
    if c.res:
        t["res"] = ri(-4, 4, _res_shape(c))
    return _finish(t, dtype, device)


FAMILIES = ["randn", "same_sign", "w*2^40,x*2^-40", "mean_1000"]


def families_of(c):
    return [f for f in FAMILIES if (f != "mean_1000" or c.ln) and not (f == "w*2^40,x*2^-40" and (c.ln or c.epi == "lnbwd"))]


def rounded(c, family, dtype, device="cpu"):
    """as `exact`, the activations already rounded to `dtype` (the oracle sees what the kernel sees)"""
    gen = _gen(c, 1 + FAMILIES.index(family))
    rn = lambda *s: torch.randn(s, generator=gen)
    B = max(c.B, 1)
    if c.epi == "lnbwd":
        x, g, _, _, gadd = LC.rounded("randn", B, c.M, c.N, dtype, c.gadd, seed=zlib.crc32(c.name.encode()) % 1000)
        gz, w = rn(B, c.K, c.N), rn(*_w_shape(c)) / c.K ** 0.5
        if family == "same_sign":
            gz, w = MC._coherent(gz), MC._coherent(w)
        t = {"x": [gz], "w": w, "lnb_x": x, "lnb_stats": LC.stats_of(x.float()), "lnb_g": g, "lnb_gadd": gadd}
        return _finish(t, dtype, device)
    t = {"x": [(1.5 * rn(*s) + 0.3 if c.bact == GELU else rn(*s)) for s in _x_shapes(c)], "w": rn(*_w_shape(c))}
    if family == "same_sign":
        t["x"], t["w"] = [MC._coherent(x) for x in t["x"]], MC._coherent(t["w"])
    if family == "mean_1000":
        t["x"] = [1000 + x for x in t["x"]]
    if family == "w*2^40,x*2^-40":
        t["x"], t["w"] = [x * 2.0 ** -40 for x in t["x"]], t["w"] * 2.0 ** 40
    if c.ln:
        t["ln_g"], t["ln_b"] = 1 + 0.5 * rn(c.K), rn(c.K)
    if c.bias:
        t["bias"] = rn(c.M // c.taps)
    if c.bmul:
        t["bmul"] = rn(B, c.Cin, c.N)
    if c.emul is not None:
        t["emul"] = 1.5 * rn(B, c.M, c.N)
    if c.res:
        t["res"] = rn(*_res_shape(c))
    return _finish(t, dtype, device)


# ------------------------------------------------------------------ bounds (module docstring) ------------------------------
LNB_DEPTH = 12


def ln_order(c, mode):
    """how the form a case reaches evaluates its LayerNorm prologue: "two_pass" (resident and persistent kernels: exact statistics,
    then the sum over A γ x̂) or "pivot" (every streaming form, split and fp32: one pass around x[channel 0], module docstring)"""
    return "two_pass" if REACHED[(c.name, mode)].split()[0] in ("resident", "p32") else "pivot"


def bounds(c, t, mode, dtype):
    """(dict of element-wise bounds: y [, mu, rs, gg, gb]; the reference they surround)"""
    ref = ref64(c, t)
    up = U_PROD[MODES[mode][1]]
    op = operand64(c, t)
    A, X, K = _weights(c, t), op["X"], c.K
    mm = lambda a, x: torch.einsum("mk,bkn->bmn", a, x)
    out = {}
    if c.ln:
        g, b = t["ln_g"].double(), t["ln_b"].double()
        Ag = (A * g.view(1, -1)).abs()
        raw = op["raw"]
        one, zero = torch.ones(K, device=raw.device), torch.zeros(K, device=raw.device)
        if ln_order(c, mode) == "two_pass":
            _, _, dn = LC.fwd_bounds(raw, one, zero, torch.float32)
            dacc = ((K + 3) * U + up) * ref["acc_terms"] + mm(Ag, dn / SLACK)
        else:
            dacc = _pivot_bound(A, g, b, raw, op["rs"], up)
        if c.stats:
            out["mu"], out["rs"] = LC.stats_bounds(raw)
    else:
        dX = torch.zeros_like(X)
        if c.bact == GELU:
            dX = MC.dgelu(op["raw"].abs()) + U * X.abs()
        dacc = ((K + 3) * U + up) * ref["acc_terms"] + mm(A.abs(), dX)
    return _epilogue_bounds(c, t, dtype, ref, dacc, out)


def _pivot_bound(A, g, b, raw, rs, up):
    """the pivoted one-pass LayerNorm prologue (module docstring)"""
    K = raw.shape[1]
    mm = lambda a, x: torch.einsum("mk,bkn->bmn", a, x)
    Ag = (A * g.view(1, -1)).abs()
    d = raw - raw[:, :1]
    m = d.mean(1, keepdim=True)
    dm = (K - 1) * U * d.abs().sum(1, keepdim=True) / K + 2 * U * m.abs()
    S, s = mm(A * g.view(1, -1), d), (A * g.view(1, -1)).sum(1).view(1, -1, 1)
    dS = ((K + 3) * U + up) * mm(Ag, d.abs())
    ds = (K + 1) * U * Ag.sum(1).view(1, -1, 1)
    core = S - m * s
    dcore = dS + m.abs() * ds + s.abs() * dm + 2 * U * (m * s).abs() + U * core.abs()
    _, drs = LC.stats_bounds(raw)
    drs_rel = (drs / SLACK).unsqueeze(1) / rs
    return rs * (dcore + core.abs() * (drs_rel + U)) + (K + 1) * U * (A.abs() @ b.abs()).view(1, -1, 1)


def _epilogue_bounds(c, t, dtype, ref, dacc, out):
    """what the epilogue adds to the bound dacc of the sum"""
    if c.epi == "lnbwd":
        dgx, dgg, dgb, r = LC.bwd_bounds(ref["acc"], t["lnb_x"], t["lnb_stats"], t["lnb_g"], t.get("lnb_gadd"), torch.float32, LNB_DEPTH)
        dgx, dgg, dgb = dgx / SLACK, dgg / SLACK, dgb / SLACK
        C = c.M
        rs = t["lnb_stats"][:, 1:2].double()
        n = (t["lnb_x"].double() - t["lnb_stats"][:, 0:1].double()) * rs
        ga = t["lnb_g"].double().abs().view(1, C, 1)
        moved = rs * (ga * dacc + (ga * dacc).mean(1, keepdim=True) + n.abs() * (ga * dacc * n.abs()).mean(1, keepdim=True))
        dy = dgx + moved
        if dtype == BF:
            dy = dy + half_ulp_bf16(ref["y"], dy)
        out.update(y=SLACK * dy, gg=SLACK * (dgg + (dacc * n.abs()).sum((0, 2))), gb=SLACK * (dgb + dacc.sum((0, 2))))
        return out, ref
    if c.taps > 1:
        dv = scatter(c, dacc) + 2 * U * ref["terms"]
    else:
        pre = ref["pre"]
        dv = dacc + U * pre.abs()
        if c.eact == GELU:
            dv = MC.GELU_LIP * dv + MC.dgelu(pre.abs() + dv) + U * _act(GELU, pre).abs()
        v = _act(c.eact, pre)
        if c.emul is not None:
            e = t["emul"].double()
            gr = _act_grad(c.emul, e)
            dgr = MC.dgelu_grad(e) if c.emul == GELU else torch.zeros_like(e)
            dv = gr.abs() * dv + v.abs() * dgr + U * (v * gr).abs()
        if c.res:
            dv = dv + U * ref["y"].abs()
    if dtype == BF:
        dv = dv + half_ulp_bf16(ref["y"], dv)
    out["y"] = SLACK * dv
    return out, ref


# ------------------------------------------------------------------ fp32 emulation on the CPU -------------------------------
def emulate(c, t, prod, dtype, fewer=False, pivot=False):
    """y in the storage type: the prologues in fp32 as the kernels compute them (mlp_cases.emu_gelu; LayerNorm in two passes, or
    with `pivot` in one pass around channel 0 as the streaming forms), the products as the mode multiplies (mlp_cases.emu_dot),
    sums in the order of the host's matmul.  fewer: one split level fewer."""
    assert c.epi != "lnbwd"
    X = W.q_operand(c, t["x"]).float()
    A = _weights(c, t).float()
    add = torch.zeros(c.M)
    post = None
    if c.ln and pivot:
        X = X - X[:, :1]
        m = X.mean(1, keepdim=True)
        var = ((X * X).mean(1, keepdim=True) - m * m).clamp_min(0)
        rs = 1 / torch.sqrt(var + MC.f32(LC.EPS))
        A = A * t["ln_g"].view(1, -1)
        tw = _weights(c, t).float() @ t["ln_b"]
        post = lambda acc: rs * (acc - m * A.sum(1).view(1, -1, 1)) + tw.view(1, -1, 1)
    elif c.ln:
        mu = X.mean(1, keepdim=True)
        rs = 1 / torch.sqrt(((X - mu) ** 2).mean(1, keepdim=True) + MC.f32(LC.EPS))
        X = (X - mu) * rs
        add = A @ t["ln_b"]
        A = A * t["ln_g"].view(1, -1)
    if c.bact == GELU:
        X = MC.emu_gelu(X)
    elif c.bact == RELU:
        X = X.clamp_min(0)
    if c.bmul:
        X = torch.where(t["bmul"].float() > 0, X, torch.zeros_like(X))
    acc = torch.stack([MC.emu_dot(A, X[b], prod, fewer) for b in range(X.shape[0])])
    if post is not None:
        acc = post(acc)
    if c.bias:
        add = add + t["bias"].repeat_interleave(c.taps)
    v = acc + add.view(1, -1, 1)
    if c.taps > 1:
        v = scatter(c, v)
    else:
        v = MC.emu_gelu(v) if c.eact == GELU else (v.clamp_min(0) if c.eact == RELU else v)
        if c.emul is not None:
            e = t["emul"].float()
            v = v * (MC.emu_gelu_grad(e) if c.emul == GELU else ((e > 0).float() if c.emul == RELU else torch.ones_like(e)))
    if c.res:
        v = v + t["res"].float()
    return v.to(dtype)


# ------------------------------------------------------------------ cases ---------------------------------------------------
def _split_cases():
    o = []
    S = ("fp32_split", "bf16")
    # streaming form, every tile through `tune` = 100 + 10 nacc + mb at one 512-column (nacc 4) / 256-column (nacc 2) tile
    for mb in (1, 2):
        for na in (2, 4):
            tn = 100 + 10 * na + mb
            M = 32 * mb
            o.append(Case(f"bx_plain_mb{mb}_n{na}", B=2, M=M, Cin=64, N=128 * na + 4, tune=tn, pad=4 if (mb, na) == (2, 2) else 0, res=mb == 1, modes=S))
            o.append(Case(f"bx_gelu_mb{mb}_n{na}", B=1, M=M, Cin=64, N=128 * na + 4, bact=GELU, tune=tn, modes=S))
            o.append(Case(f"bx_d2s_mb{mb}_n{na}", epi="d2s", B=1, M=M, Cin=64, grid=(2, 4, 8 * na + 4), tune=tn, w_t=1, res=na == 2, modes=S))
        o.append(Case(f"bx_ln_mb{mb}", B=2, M=32 * mb, Cin=64, N=260, ln=True, stats=True, tune=120 + mb, modes=S))
        o.append(Case(f"bx_bmul_mb{mb}", B=2, M=32 * mb, Cin=64, N=260, bmul=True, w_t=1, tune=120 + mb, modes=S))
        o.append(Case(f"bx_s2d_mb{mb}", "s2d", B=2, M=32 * mb, Cin=8, grid=(2, 4, 10), tune=120 + mb, modes=S))
        o.append(Case(f"bx_s2d_mb{mb}_wt", "s2d", B=1, M=32 * mb, Cin=8, grid=(2, 4, 10), w_t=1, pad=4, tune=120 + mb, modes=S))
    o.append(Case("bx_plain_mb1_n2_wt", B=2, M=32, Cin=64, N=260, w_t=1, pad=8, tune=121, eact=RELU, modes=S))
    # seams of the streaming form: one tile, a tile straddling two samples, K = 96 (trailing half chunk), K = 32 on bf16
    # storage, M = 96 (mb = 2 falls back), the concat at c0 = 16 and 48 of 64
    o.append(Case("bx_tile_one", B=1, M=32, Cin=64, N=256, tune=121, modes=S))
    o.append(Case("bx_tile_plus4", B=1, M=32, Cin=64, N=260, tune=121, modes=S))
    o.append(Case("bx_tile_two_samples", B=2, M=32, Cin=64, N=132, tune=121, modes=S))
    o.append(Case("bx_k96", B=2, M=64, Cin=96, N=132, tune=122, emul=RELU, modes=S))
    o.append(Case("bx_k32_bf16", B=2, M=32, Cin=32, N=132, tune=121, modes=("bf16",)))
    o.append(Case("bx_m96", B=2, M=96, Cin=64, N=132, tune=122, modes=S))
    o.append(Case("bx_c0_16", B=2, M=32, Cin=64, N=132, c0=16, tune=121, modes=S))
    o.append(Case("bx_c0_48", B=2, M=64, Cin=64, N=132, c0=48, tune=142, modes=S))
    # the library's own choice (tune = 0) on either side of the 512-workgroup thresholds of the streaming form
    o.append(Case("bx_auto_n4_mb2", B=1, M=64, Cin=64, N=512 * 512, modes=("fp32_split",)))
    o.append(Case("bx_auto_n2_mb2", B=1, M=64, Cin=64, N=512 * 511, modes=("fp32_split",)))
    o.append(Case("bx_auto_n2_mb1", B=1, M=64, Cin=64, N=512 * 127, modes=("fp32_split",)))
    # K-split form, every tile through `tune` = 200 + 10 nacc + mb
    for mb in (1, 2):
        for na in (1, 2):
            tn = 200 + 10 * na + mb
            M = 32 * mb
            o.append(Case(f"bxk_plain_mb{mb}_n{na}", B=2, M=M, Cin=64, N=32 * na + 4, tune=tn, res=na == 1, modes=S))
            o.append(Case(f"bxk_ln_mb{mb}_n{na}", B=2, M=M, Cin=64, N=32 * na + 4, ln=True, stats=mb == 1, tune=tn, modes=S))
            o.append(Case(f"bxk_gelu_mb{mb}_n{na}", B=2, M=M, Cin=64, N=32 * na + 4, bact=GELU, w_t=1, tune=tn, modes=S))
            o.append(Case(f"bxk_bmul_mb{mb}_n{na}", B=2, M=M, Cin=64, N=32 * na + 4, bmul=True, tune=tn, modes=S))
            o.append(Case(f"bxk_d2s_mb{mb}_n{na}", epi="d2s", B=2, M=M, Cin=64, grid=(1, 3, 12), tune=tn, w_t=1, modes=S))
        o.append(Case(f"bxk_s2d_mb{mb}", "s2d", B=2, M=32 * mb, Cin=8, grid=(1, 3, 12), tune=220 + mb, modes=S))
    o.append(Case("bxk_emul_gelu", B=2, M=32, Cin=64, N=36, emul=GELU, eact=RELU, tune=211, modes=S))
    o.append(Case("bxk_c0_48", B=2, M=32, Cin=128, N=36, c0=48, tune=211, modes=S))
    # tune = 0: Ncol B = 4096 (K-split) and 4100 (streaming); 8192 columns with K = 512 (K-split) and K = 256 (streaming)
    o.append(Case("bxk_auto_4096", B=1, M=64, Cin=64, N=4096, modes=("fp32_split",)))
    o.append(Case("bx_auto_4100", B=1, M=64, Cin=64, N=4100, modes=("fp32_split",)))
    o.append(Case("bxk_auto_8192_k512", B=2, M=64, Cin=512, N=4096, modes=("fp32_split",)))
    o.append(Case("bx_auto_8192_k256", B=2, M=64, Cin=256, N=4096, modes=("fp32_split",)))
    # the padded 1-D grid: 2 and 8 row-block groups, tiles B in {64, 65, 71}
    for groups, tb in ((2, 64), (2, 65), (8, 71)):
        o.append(Case(f"bx_grid1d_g{groups}_t{tb}", B=tb, M=32 * groups, Cin=64, N=132, tune=121, modes=("fp32_split",)))
        o.append(Case(f"str_grid1d_g{groups}_t{tb}", B=tb, M=32 * groups, Cin=40, N=68, modes=("fp32_mfma",)))
    return o


def _resident_cases():
    o = []
    A = tuple(MODES)
    F = ("fp32_mfma", "fp32_split")
    o.append(Case("res_k2_m1", B=2, M=1, Cin=2, N=4, w_t=1, pad=3, modes=F))
    o.append(Case("res_c0_k15", B=2, M=32, Cin=15, N=516, c0=7, res=True, modes=F))
    o.append(Case("res_k16_m40", B=2, M=40, Cin=16, N=512, pad=5, res=True, modes=A))
    o.append(Case("res_k32_m64", B=1, M=64, Cin=32, N=516, eact=RELU, modes=F))
    o.append(Case("res_m288", B=1, M=288, Cin=16, N=4, modes=F))
    o.append(Case("res_n516", B=2, M=64, Cin=32, N=516, modes=F))
    o.append(Case("res_pf0_relu_res", B=2, M=64, Cin=32, N=36, eact=RELU, res=True, modes=F))
    o.append(Case("res_eact_emul_relu", B=2, M=64, Cin=32, N=36, eact=RELU, emul=RELU, modes=F))
    o.append(Case("res_pf1_gelu", B=2, M=64, Cin=32, N=36, bact=GELU, modes=F))
    o.append(Case("res_pf1_relu", B=2, M=32, Cin=32, N=36, bact=RELU, emul=GELU, modes=F))
    o.append(Case("res_pf2_stats", B=2, M=64, Cin=32, N=516, ln=True, stats=True, modes=A))
    o.append(Case("res_bmul", B=2, M=32, Cin=32, N=36, bmul=True, w_t=1, modes=A))
    o.append(Case("res_respf", B=2, M=32, Cin=32, N=516, res=True, modes=A))
    o.append(Case("res_respf_gelu", B=2, M=32, Cin=16, N=36, res=True, bact=GELU, eact=RELU, modes=F))
    o.append(Case("res_d2s_k32", epi="d2s", B=2, M=64, Cin=32, grid=(2, 3, 6), w_t=1, res=True, modes=A))
    o.append(Case("res_d2s_k16_m16", epi="d2s", B=1, M=16, Cin=16, grid=(1, 2, 6), modes=F))
    o.append(Case("res_d2s_relu", epi="d2s", B=1, M=16, Cin=16, grid=(1, 2, 6), bact=RELU, w_t=1, modes=F))
    for K in (32, 64):
        for ga in (False, True):
            o.append(Case(f"res_lnbwd_k{K}{'_gadd' if ga else ''}", epi="lnbwd", B=2, M=32, Cin=K, N=516, w_t=1, gadd=ga, modes=A if K == 64 else F))
    o.append(Case("res_lnbwd_k32_relu", epi="lnbwd", B=2, M=32, Cin=32, N=36, w_t=1, gadd=True, bact=RELU, modes=F))
    return o


def _stream_cases():
    o = []
    F = ("fp32_mfma",)
    o.append(Case("str_small_k16", B=2, M=32, Cin=16, N=132, eact=RELU, modes=F))
    o.append(Case("str_small_k32_ln", B=2, M=3, Cin=32, N=132, ln=True, stats=True, modes=F + ("bf16",)))
    pro = {"none": {}, "ln": {"ln": True, "stats": True}, "gelu": {"bact": GELU}, "bmul": {"bmul": True}}
    for pn, kw in pro.items():
        # (MB, nacc) of FZ_STR_SHAPES by the workgroup thresholds: 1 x 1 (few columns), 1 x 2, 1 x 4 (one row block); 2 x 4 below
        o.append(Case(f"str_{pn}_mb1_n1", B=2, M=64, Cin=40, N=36, res=pn == "none", **kw, modes=F))
        o.append(Case(f"str_{pn}_mb1_n2", B=64, M=64, Cin=40, N=260, **kw, modes=F))
        o.append(Case(f"str_{pn}_mb1_n4", B=64, M=64, Cin=40, N=516, w_t=pn == "gelu", **kw, modes=F))
        o.append(Case(f"str_{pn}_mb2_n4", B=128, M=256, Cin=34, N=36, **kw, modes=F))
    o.append(Case("str_ks4_n2", B=1, M=32, Cin=256, N=260, modes=F))
    o.append(Case("str_ks4_ln", B=1, M=32, Cin=256, N=260, ln=True, stats=True, modes=F))
    o.append(Case("str_ks4_gelu", B=1, M=32, Cin=256, N=260, bact=GELU, w_t=1, modes=F))
    o.append(Case("str_ks4_bmul", B=1, M=32, Cin=256, N=260, bmul=True, modes=F))
    o.append(Case("str_ks4_k258", B=1, M=32, Cin=258, N=36, modes=F))
    o.append(Case("str_s2d", "s2d", B=2, M=40, Cin=5, grid=(2, 3, 6), res=True, modes=F + ("fp32_split",)))
    o.append(Case("str_s2d_ks4", "s2d", B=1, M=32, Cin=32, grid=(1, 3, 6), modes=F))
    o.append(Case("str_s2d_ks4_cin33", "s2d", B=2, M=40, Cin=33, grid=(1, 3, 6), modes=F))     # odd Cin: the last channel pair is half empty
    o.append(Case("str_s2d_2d_cin5", "s2d_2d", B=2, M=40, Cin=5, grid=(6, 6), modes=F + ("bf16",)))
    o.append(Case("str_s2d_2d_ks4_cin65", "s2d_2d", B=1, M=32, Cin=65, grid=(2, 6), modes=F))
    o.append(Case("str_s2d_2d", "s2d_2d", B=2, M=40, Cin=10, grid=(6, 6), modes=F + ("bf16",)))
    o.append(Case("str_s2d_2d_ks4", "s2d_2d", B=1, M=32, Cin=64, grid=(2, 6), modes=F))
    o.append(Case("str_k3_mb1", "k3", B=2, M=32, Cin=2, grid=(2, 3, 12), eact=RELU, modes=F + ("bf16",)))
    o.append(Case("str_k3_mb2", "k3", B=512, M=64, Cin=2, grid=(2, 3, 4), modes=F))
    o.append(Case("str_k3_2d_mb1", "k3_2d", B=2, M=33, Cin=4, grid=(5, 12), modes=F + ("bf16",)))
    o.append(Case("str_k3_2d_mb2", "k3_2d", B=512, M=64, Cin=2, grid=(3, 4), modes=F))
    o.append(Case("str_d2s_mb1", epi="d2s", B=2, M=40, Cin=40, grid=(2, 3, 6), w_t=1, res=True, modes=F + ("bf16",)))
    o.append(Case("str_d2s_mb2", epi="d2s", B=512, M=64, Cin=34, grid=(1, 2, 4), w_t=1, modes=F))
    o.append(Case("str_d2s_2d_mb1", epi="d2s_2d", B=2, M=36, Cin=10, grid=(6, 6), w_t=1, res=True, modes=F + ("bf16",)))
    o.append(Case("str_d2s_2d_mb2", epi="d2s_2d", B=512, M=64, Cin=34, grid=(2, 4), w_t=1, modes=F))
    return o


def _other_cases():
    o = []
    A = tuple(MODES)
    # persistent 32 -> 32: B ceil(Ncol / 128) at 4095 (resident / streaming) and 4096 (taken); Ncol % 128 != 0 with B = 3
    o.append(Case("p32_4095_not_taken", B=1, M=32, Cin=32, N=4095 * 128, ln=True, stats=True, modes=("fp32_mfma",)))
    o.append(Case("p32_4096_ln", B=1, M=32, Cin=32, N=4096 * 128, ln=True, stats=True, modes=("fp32_mfma", "bf16")))
    o.append(Case("p32_b3_ln_m3", B=3, M=3, Cin=32, N=1366 * 128 - 4, ln=True, stats=True, modes=("fp32_mfma",)))
    o.append(Case("p32_plain_eact", B=3, M=32, Cin=32, N=1366 * 128 - 4, eact=RELU, modes=("fp32_mfma", "bf16")))
    o.append(Case("chain64_lnb", epi="lnbwd", B=2, M=64, Cin=64, N=260, w_t=1, gadd=True, modes=A))
    o.append(Case("head_m3", B=2, M=3, Cin=32, N=132, modes=("fp32_mfma", "bf16")))
    o.append(Case("head_m2_nobias", B=2, M=2, Cin=32, N=132, bias=False, modes=("fp32_mfma",)))
    return o


CASES = _split_cases() + _resident_cases() + _stream_cases() + _other_cases()
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)


def has_exact(c):
    """LayerNorm has no exact family, and a GELU of the sum none either: those cases are judged on rounded inputs"""
    return not c.ln and c.eact != GELU


def elements(c):
    """elements of the largest tensor of a case"""
    return max(c.B, 1) * max(c.M * c.N, c.Cin * c.Vq)


# the rounded families run where a form's arithmetic differs: every family, prologue, loader and epilogue once
ROUNDED_AT = ["bx_plain_mb2_n4", "bx_gelu_mb1_n2", "bx_d2s_mb1_n2", "bx_ln_mb1", "bx_ln_mb2", "bx_bmul_mb1", "bx_s2d_mb2", "bx_k96",
              "bx_k32_bf16", "bx_tile_plus4", "bx_m96", "bxk_plain_mb1_n1", "bxk_ln_mb1_n2", "bxk_ln_mb2_n1", "bxk_gelu_mb2_n2",
              "bxk_bmul_mb1_n1", "bxk_d2s_mb1_n2", "bxk_s2d_mb1", "bxk_emul_gelu", "bxk_auto_8192_k512", "res_k2_m1", "res_c0_k15",
              "res_k16_m40", "res_m288", "res_n516", "res_pf0_relu_res", "res_eact_emul_relu", "res_pf1_gelu", "res_pf2_stats",
              "res_bmul", "res_respf", "res_d2s_k32", "res_lnbwd_k32", "res_lnbwd_k64_gadd", "str_small_k32_ln",
              "str_none_mb1_n1", "str_ln_mb1_n2", "str_gelu_mb1_n4", "str_bmul_mb1_n2", "str_ks4_n2", "str_ks4_k258", "str_ks4_ln", "str_ks4_gelu", "str_ks4_bmul", "str_s2d",
              "str_s2d_ks4", "str_s2d_ks4_cin33", "str_s2d_2d", "str_s2d_2d_cin5", "str_s2d_2d_ks4_cin65", "str_k3_mb1", "str_k3_2d_mb1", "str_d2s_mb1", "str_d2s_2d_mb1", "chain64_lnb", "head_m3",
              "bx_grid1d_g8_t71", "str_grid1d_g8_t71"]

# ------------------------------------------------------------------ every form the launchers can select --------------------
_FORMS_TEXT = """
# gemm_bx.hip FZ_BX: s2d loader (two tiles), then FZ_BX_TILES for d2s / gelu / none and FZ_BX_TILES2 for ln (rd 4) / bmul (rd 2)
bx_stream mb1 nacc2 s2d rd4 | bx_stream mb2 nacc2 s2d rd4 | bx_stream mb1 nacc2 s2d wt rd4 | bx_stream mb2 nacc2 s2d wt rd4
bx_stream mb1 nacc2 plain rd4 | bx_stream mb2 nacc2 plain rd4 | bx_stream mb1 nacc4 plain rd2 | bx_stream mb2 nacc4 plain rd1
bx_stream mb1 nacc2 plain d2s rd4 | bx_stream mb2 nacc2 plain d2s rd4 | bx_stream mb1 nacc4 plain d2s rd2 | bx_stream mb2 nacc4 plain d2s rd1
bx_stream mb1 nacc2 plain gelu rd4 | bx_stream mb2 nacc2 plain gelu rd4 | bx_stream mb1 nacc4 plain gelu rd2 | bx_stream mb2 nacc4 plain gelu rd1
bx_stream mb1 nacc2 plain ln rd4 | bx_stream mb2 nacc2 plain ln rd4
bx_stream mb1 nacc2 plain bmul rd4 | bx_stream mb2 nacc2 plain bmul rd2
# gemm_bxk.hip FZ_BXK: s2d (mb 1 rd 4, mb 2 rd 2), FZ_BXK_TILES: light (none, gelu, d2s) rd 4 4 4 2, heavy (ln, bmul) rd 2 2 2 1
bxk mb1 nacc2 s2d rd4 | bxk mb2 nacc2 s2d rd2
bxk mb1 nacc1 plain rd4 | bxk mb2 nacc1 plain rd4 | bxk mb1 nacc2 plain rd4 | bxk mb2 nacc2 plain rd2
bxk mb1 nacc1 plain gelu rd4 | bxk mb2 nacc1 plain gelu rd4 | bxk mb1 nacc2 plain gelu rd4 | bxk mb2 nacc2 plain gelu rd2
bxk mb1 nacc1 plain d2s rd4 | bxk mb2 nacc1 plain d2s rd4 | bxk mb1 nacc2 plain d2s rd4 | bxk mb2 nacc2 plain d2s rd2
bxk mb1 nacc1 plain ln rd2 | bxk mb2 nacc1 plain ln rd2 | bxk mb1 nacc2 plain ln rd2 | bxk mb2 nacc2 plain ln rd1
bxk mb1 nacc1 plain bmul rd2 | bxk mb2 nacc1 plain bmul rd2 | bxk mb1 nacc2 plain bmul rd2 | bxk mb2 nacc2 plain bmul rd1
# gemm.hip: FZ_RES (ns 16 x pf 0..2; pf 3 = LayerNorm + activation is refused: see test_gemm_cpu.py) for plain and d2s (d2s: pf 0 and 1 — LayerNorm in front of it is refused too), pf 0 for bmul (the gate takes no second prologue); the residual-prefetch
# form; FZ_RES_LNB.  (The ns 32 arms of FZ_RES are dead: outside lnbwd the resident kernel takes K <= 32, so nA <= 16.)
resident ns16 plain pf0 | resident ns16 plain pf1 | resident ns16 plain pf2
resident ns16 plain pf0 bmul
resident ns16 plain d2s pf0 | resident ns16 plain d2s pf1
resident ns16 plain pf0 respf | resident ns16 plain pf1 respf
resident ns16 plain lnbwd pf3 | resident ns16 plain lnbwd pf3 gadd | resident ns32 plain lnbwd pf3 | resident ns32 plain lnbwd pf3 gadd
# gemm_stream.hip FZ_STR / FZ_STRK.  (FZ_STRK(1, 1, plain) is dead in the shipped library: nacc = 1 is chosen only when
# wgs(1) >= 256, and ks = 4 needs the same count below 256; only the probe knob FZ_GEMM_CFG reaches it.)
stream mb1 nacc2 s2d | stream mb1 nacc2 s2d ks4 | stream mb1 nacc2 s2d2 | stream mb1 nacc2 s2d2 ks4
stream mb1 nacc4 k3_2 | stream mb2 nacc4 k3_2 | stream mb1 nacc4 k3 | stream mb2 nacc4 k3
stream mb1 nacc4 plain d2s2 | stream mb2 nacc4 plain d2s2 | stream mb1 nacc4 plain d2s | stream mb2 nacc4 plain d2s
stream mb1 nacc1 plain | stream mb1 nacc2 plain | stream mb1 nacc4 plain | stream mb2 nacc4 plain | stream mb1 nacc2 plain ks4
stream mb1 nacc1 plain ln | stream mb1 nacc2 plain ln | stream mb1 nacc4 plain ln | stream mb2 nacc4 plain ln | stream mb1 nacc2 plain ln ks4
stream mb1 nacc1 plain gelu | stream mb1 nacc2 plain gelu | stream mb1 nacc4 plain gelu | stream mb2 nacc4 plain gelu | stream mb1 nacc2 plain gelu ks4
stream mb1 nacc1 plain bmul | stream mb1 nacc2 plain bmul | stream mb1 nacc4 plain bmul | stream mb2 nacc4 plain bmul | stream mb1 nacc2 plain bmul ks4
# gemm_p32.hip, mlp_chain64.hip chain64_lnb_launch, headbwd.hip head_fwd_launch
p32 pf0 | p32 pf2
chain64_lnb split | chain64_lnb fp32
head m2 | head m4
"""
FORMS = set()
for _l in _FORMS_TEXT.strip().splitlines():
    if not _l.startswith("#"):
        for _f in _l.split("|"):
            FORMS.add(_f.strip())

# ------------------------------------------------------------------ the form each case reaches -----------------------------
# "<case> <mode> | <what fz_gemm_plan answers>", recorded from the library; tests/test_gemm_cpu.py holds every line to the
# library's answer (a change of the dispatcher that moves a case to another form fails there, not silently on the device)
_REACHED_TEXT = """
bx_plain_mb1_n2 fp32_split | bx_stream mb1 nacc2 plain rd4 grid=4x1
bx_plain_mb1_n2 bf16 | bx_stream mb1 nacc2 plain rd4 grid=4x1
bx_gelu_mb1_n2 fp32_split | bx_stream mb1 nacc2 plain gelu rd4 grid=2x1
bx_gelu_mb1_n2 bf16 | bx_stream mb1 nacc2 plain gelu rd4 grid=2x1
bx_d2s_mb1_n2 fp32_split | bx_stream mb1 nacc2 plain d2s wt rd4 grid=1x1
bx_d2s_mb1_n2 bf16 | bx_stream mb1 nacc2 plain d2s wt rd4 grid=1x1
bx_plain_mb1_n4 fp32_split | bx_stream mb1 nacc4 plain rd2 grid=4x1
bx_plain_mb1_n4 bf16 | bx_stream mb1 nacc4 plain rd2 grid=4x1
bx_gelu_mb1_n4 fp32_split | bx_stream mb1 nacc4 plain gelu rd2 grid=2x1
bx_gelu_mb1_n4 bf16 | bx_stream mb1 nacc4 plain gelu rd2 grid=2x1
bx_d2s_mb1_n4 fp32_split | bx_stream mb1 nacc4 plain d2s wt rd2 grid=1x1
bx_d2s_mb1_n4 bf16 | bx_stream mb1 nacc4 plain d2s wt rd2 grid=1x1
bx_ln_mb1 fp32_split | bx_stream mb1 nacc2 plain ln rd4 grid=4x1
bx_ln_mb1 bf16 | bx_stream mb1 nacc2 plain ln rd4 grid=4x1
bx_bmul_mb1 fp32_split | bx_stream mb1 nacc2 plain bmul wt rd4 grid=4x1
bx_bmul_mb1 bf16 | bx_stream mb1 nacc2 plain bmul wt rd4 grid=4x1
bx_s2d_mb1 fp32_split | bx_stream mb1 nacc2 s2d rd4 grid=2x1
bx_s2d_mb1 bf16 | bx_stream mb1 nacc2 s2d rd4 grid=2x1
bx_s2d_mb1_wt fp32_split | bx_stream mb1 nacc2 s2d wt rd4 grid=1x1
bx_s2d_mb1_wt bf16 | bx_stream mb1 nacc2 s2d wt rd4 grid=1x1
bx_plain_mb2_n2 fp32_split | bx_stream mb2 nacc2 plain rd4 grid=4x1
bx_plain_mb2_n2 bf16 | bx_stream mb2 nacc2 plain rd4 grid=4x1
bx_gelu_mb2_n2 fp32_split | bx_stream mb2 nacc2 plain gelu rd4 grid=2x1
bx_gelu_mb2_n2 bf16 | bx_stream mb2 nacc2 plain gelu rd4 grid=2x1
bx_d2s_mb2_n2 fp32_split | bx_stream mb2 nacc2 plain d2s wt rd4 grid=1x1
bx_d2s_mb2_n2 bf16 | bx_stream mb2 nacc2 plain d2s wt rd4 grid=1x1
bx_plain_mb2_n4 fp32_split | bx_stream mb2 nacc4 plain rd1 grid=4x1
bx_plain_mb2_n4 bf16 | bx_stream mb2 nacc4 plain rd1 grid=4x1
bx_gelu_mb2_n4 fp32_split | bx_stream mb2 nacc4 plain gelu rd1 grid=2x1
bx_gelu_mb2_n4 bf16 | bx_stream mb2 nacc4 plain gelu rd1 grid=2x1
bx_d2s_mb2_n4 fp32_split | bx_stream mb2 nacc4 plain d2s wt rd1 grid=1x1
bx_d2s_mb2_n4 bf16 | bx_stream mb2 nacc4 plain d2s wt rd1 grid=1x1
bx_ln_mb2 fp32_split | bx_stream mb2 nacc2 plain ln rd4 grid=4x1
bx_ln_mb2 bf16 | bx_stream mb2 nacc2 plain ln rd4 grid=4x1
bx_bmul_mb2 fp32_split | bx_stream mb2 nacc2 plain bmul wt rd2 grid=4x1
bx_bmul_mb2 bf16 | bx_stream mb2 nacc2 plain bmul wt rd2 grid=4x1
bx_s2d_mb2 fp32_split | bx_stream mb2 nacc2 s2d rd4 grid=2x1
bx_s2d_mb2 bf16 | bx_stream mb2 nacc2 s2d rd4 grid=2x1
bx_s2d_mb2_wt fp32_split | bx_stream mb2 nacc2 s2d wt rd4 grid=1x1
bx_s2d_mb2_wt bf16 | bx_stream mb2 nacc2 s2d wt rd4 grid=1x1
bx_plain_mb1_n2_wt fp32_split | bx_stream mb1 nacc2 plain wt rd4 grid=4x1
bx_plain_mb1_n2_wt bf16 | bx_stream mb1 nacc2 plain wt rd4 grid=4x1
bx_tile_one fp32_split | bx_stream mb1 nacc2 plain rd4 grid=1x1
bx_tile_one bf16 | bx_stream mb1 nacc2 plain rd4 grid=1x1
bx_tile_plus4 fp32_split | bx_stream mb1 nacc2 plain rd4 grid=2x1
bx_tile_plus4 bf16 | bx_stream mb1 nacc2 plain rd4 grid=2x1
bx_tile_two_samples fp32_split | bx_stream mb1 nacc2 plain rd4 grid=2x1
bx_tile_two_samples bf16 | bx_stream mb1 nacc2 plain rd4 grid=2x1
bx_k96 fp32_split | bx_stream mb2 nacc2 plain rd4 grid=2x1
bx_k96 bf16 | bx_stream mb2 nacc2 plain rd4 grid=2x1
bx_k32_bf16 bf16 | bx_stream mb1 nacc2 plain rd4 grid=2x1
bx_m96 fp32_split | bx_stream mb1 nacc2 plain rd4 grid=2x3
bx_m96 bf16 | bx_stream mb1 nacc2 plain rd4 grid=2x3
bx_c0_16 fp32_split | bx_stream mb1 nacc2 plain rd4 grid=2x1
bx_c0_16 bf16 | bx_stream mb1 nacc2 plain rd4 grid=2x1
bx_c0_48 fp32_split | bx_stream mb2 nacc4 plain rd1 grid=2x1
bx_c0_48 bf16 | bx_stream mb2 nacc4 plain rd1 grid=2x1
bx_auto_n4_mb2 fp32_split | bx_stream mb2 nacc4 plain rd1 grid=512x1
bx_auto_n2_mb2 fp32_split | bx_stream mb2 nacc2 plain rd4 grid=1022x1
bx_auto_n2_mb1 fp32_split | bx_stream mb1 nacc2 plain rd4 grid=512x1
bxk_plain_mb1_n1 fp32_split | bxk mb1 nacc1 plain rd4 grid=4x1
bxk_plain_mb1_n1 bf16 | bxk mb1 nacc1 plain rd4 grid=4x1
bxk_ln_mb1_n1 fp32_split | bxk mb1 nacc1 plain ln rd2 grid=4x1
bxk_ln_mb1_n1 bf16 | bxk mb1 nacc1 plain ln rd2 grid=4x1
bxk_gelu_mb1_n1 fp32_split | bxk mb1 nacc1 plain gelu wt rd4 grid=4x1
bxk_gelu_mb1_n1 bf16 | bxk mb1 nacc1 plain gelu wt rd4 grid=4x1
bxk_bmul_mb1_n1 fp32_split | bxk mb1 nacc1 plain bmul rd2 grid=4x1
bxk_bmul_mb1_n1 bf16 | bxk mb1 nacc1 plain bmul rd2 grid=4x1
bxk_d2s_mb1_n1 fp32_split | bxk mb1 nacc1 plain d2s wt rd4 grid=4x1
bxk_d2s_mb1_n1 bf16 | bxk mb1 nacc1 plain d2s wt rd4 grid=4x1
bxk_plain_mb1_n2 fp32_split | bxk mb1 nacc2 plain rd4 grid=4x1
bxk_plain_mb1_n2 bf16 | bxk mb1 nacc2 plain rd4 grid=4x1
bxk_ln_mb1_n2 fp32_split | bxk mb1 nacc2 plain ln rd2 grid=4x1
bxk_ln_mb1_n2 bf16 | bxk mb1 nacc2 plain ln rd2 grid=4x1
bxk_gelu_mb1_n2 fp32_split | bxk mb1 nacc2 plain gelu wt rd4 grid=4x1
bxk_gelu_mb1_n2 bf16 | bxk mb1 nacc2 plain gelu wt rd4 grid=4x1
bxk_bmul_mb1_n2 fp32_split | bxk mb1 nacc2 plain bmul rd2 grid=4x1
bxk_bmul_mb1_n2 bf16 | bxk mb1 nacc2 plain bmul rd2 grid=4x1
bxk_d2s_mb1_n2 fp32_split | bxk mb1 nacc2 plain d2s wt rd4 grid=2x1
bxk_d2s_mb1_n2 bf16 | bxk mb1 nacc2 plain d2s wt rd4 grid=2x1
bxk_s2d_mb1 fp32_split | bxk mb1 nacc2 s2d rd4 grid=2x1
bxk_s2d_mb1 bf16 | bxk mb1 nacc2 s2d rd4 grid=2x1
bxk_plain_mb2_n1 fp32_split | bxk mb2 nacc1 plain rd4 grid=4x1
bxk_plain_mb2_n1 bf16 | bxk mb2 nacc1 plain rd4 grid=4x1
bxk_ln_mb2_n1 fp32_split | bxk mb2 nacc1 plain ln rd2 grid=4x1
bxk_ln_mb2_n1 bf16 | bxk mb2 nacc1 plain ln rd2 grid=4x1
bxk_gelu_mb2_n1 fp32_split | bxk mb2 nacc1 plain gelu wt rd4 grid=4x1
bxk_gelu_mb2_n1 bf16 | bxk mb2 nacc1 plain gelu wt rd4 grid=4x1
bxk_bmul_mb2_n1 fp32_split | bxk mb2 nacc1 plain bmul rd2 grid=4x1
bxk_bmul_mb2_n1 bf16 | bxk mb2 nacc1 plain bmul rd2 grid=4x1
bxk_d2s_mb2_n1 fp32_split | bxk mb2 nacc1 plain d2s wt rd4 grid=4x1
bxk_d2s_mb2_n1 bf16 | bxk mb2 nacc1 plain d2s wt rd4 grid=4x1
bxk_plain_mb2_n2 fp32_split | bxk mb2 nacc2 plain rd2 grid=4x1
bxk_plain_mb2_n2 bf16 | bxk mb2 nacc2 plain rd2 grid=4x1
bxk_ln_mb2_n2 fp32_split | bxk mb2 nacc2 plain ln rd1 grid=4x1
bxk_ln_mb2_n2 bf16 | bxk mb2 nacc2 plain ln rd1 grid=4x1
bxk_gelu_mb2_n2 fp32_split | bxk mb2 nacc2 plain gelu wt rd2 grid=4x1
bxk_gelu_mb2_n2 bf16 | bxk mb2 nacc2 plain gelu wt rd2 grid=4x1
bxk_bmul_mb2_n2 fp32_split | bxk mb2 nacc2 plain bmul rd1 grid=4x1
bxk_bmul_mb2_n2 bf16 | bxk mb2 nacc2 plain bmul rd1 grid=4x1
bxk_d2s_mb2_n2 fp32_split | bxk mb2 nacc2 plain d2s wt rd2 grid=2x1
bxk_d2s_mb2_n2 bf16 | bxk mb2 nacc2 plain d2s wt rd2 grid=2x1
bxk_s2d_mb2 fp32_split | bxk mb2 nacc2 s2d rd2 grid=2x1
bxk_s2d_mb2 bf16 | bxk mb2 nacc2 s2d rd2 grid=2x1
bxk_emul_gelu fp32_split | bxk mb1 nacc1 plain rd4 grid=4x1
bxk_emul_gelu bf16 | bxk mb1 nacc1 plain rd4 grid=4x1
bxk_c0_48 fp32_split | bxk mb1 nacc1 plain rd4 grid=4x1
bxk_c0_48 bf16 | bxk mb1 nacc1 plain rd4 grid=4x1
bxk_auto_4096 fp32_split | bxk mb1 nacc1 plain rd4 grid=256x1
bx_auto_4100 fp32_split | bx_stream mb1 nacc2 plain rd4 grid=17x2
bxk_auto_8192_k512 fp32_split | bxk mb1 nacc1 plain rd4 grid=512x1
bx_auto_8192_k256 fp32_split | bx_stream mb1 nacc2 plain rd4 grid=32x2
bx_grid1d_g2_t64 fp32_split | bx_stream mb1 nacc2 plain rd4 grid=128x1
str_grid1d_g2_t64 fp32_mfma | stream mb1 nacc1 plain grid=128x1
bx_grid1d_g2_t65 fp32_split | bx_stream mb1 nacc2 plain rd4 grid=144x1
str_grid1d_g2_t65 fp32_mfma | stream mb1 nacc1 plain grid=144x1
bx_grid1d_g8_t71 fp32_split | bx_stream mb1 nacc2 plain rd4 grid=576x1
str_grid1d_g8_t71 fp32_mfma | stream mb1 nacc4 plain grid=576x1
res_k2_m1 fp32_mfma | resident ns16 plain pf0 rb=1 grid=2x1
res_k2_m1 fp32_split | resident ns16 plain pf0 rb=1 grid=2x1
res_c0_k15 fp32_mfma | resident ns16 plain pf0 respf rb=1 grid=4x1
res_c0_k15 fp32_split | resident ns16 plain pf0 respf rb=1 grid=4x1
res_k16_m40 fp32_mfma | resident ns16 plain pf0 rb=2 grid=2x1
res_k16_m40 fp32_split | resident ns16 plain pf0 rb=2 grid=2x1
res_k16_m40 bf16 | resident ns16 plain pf0 rb=2 grid=2x1
res_k16_m40 bf16_mfma | resident ns16 plain pf0 rb=2 grid=2x1
res_k32_m64 fp32_mfma | resident ns16 plain pf0 rb=2 grid=2x1
res_k32_m64 fp32_split | resident ns16 plain pf0 rb=2 grid=2x1
res_m288 fp32_mfma | resident ns16 plain pf0 rb=8 grid=1x2
res_m288 fp32_split | resident ns16 plain pf0 rb=8 grid=1x2
res_n516 fp32_mfma | resident ns16 plain pf0 rb=2 grid=4x1
res_n516 fp32_split | resident ns16 plain pf0 rb=2 grid=4x1
res_pf0_relu_res fp32_mfma | resident ns16 plain pf0 rb=2 grid=2x1
res_pf0_relu_res fp32_split | resident ns16 plain pf0 rb=2 grid=2x1
res_eact_emul_relu fp32_mfma | resident ns16 plain pf0 rb=2 grid=2x1
res_eact_emul_relu fp32_split | resident ns16 plain pf0 rb=2 grid=2x1
res_pf1_gelu fp32_mfma | resident ns16 plain pf1 rb=2 grid=2x1
res_pf1_gelu fp32_split | resident ns16 plain pf1 rb=2 grid=2x1
res_pf1_relu fp32_mfma | resident ns16 plain pf1 rb=1 grid=2x1
res_pf1_relu fp32_split | resident ns16 plain pf1 rb=1 grid=2x1
res_pf2_stats fp32_mfma | resident ns16 plain pf2 rb=2 grid=4x1
res_pf2_stats fp32_split | resident ns16 plain pf2 rb=2 grid=4x1
res_pf2_stats bf16 | resident ns16 plain pf2 rb=2 grid=4x1
res_pf2_stats bf16_mfma | resident ns16 plain pf2 rb=2 grid=4x1
res_bmul fp32_mfma | resident ns16 plain pf0 bmul rb=1 grid=2x1
res_bmul fp32_split | resident ns16 plain pf0 bmul rb=1 grid=2x1
res_bmul bf16 | bx_stream mb1 nacc2 plain bmul wt rd4 grid=2x1
res_bmul bf16_mfma | resident ns16 plain pf0 bmul rb=1 grid=2x1
res_respf fp32_mfma | resident ns16 plain pf0 respf rb=1 grid=4x1
res_respf fp32_split | resident ns16 plain pf0 respf rb=1 grid=4x1
res_respf bf16 | bx_stream mb1 nacc2 plain rd4 grid=6x1
res_respf bf16_mfma | resident ns16 plain pf0 respf rb=1 grid=4x1
res_respf_gelu fp32_mfma | resident ns16 plain pf1 respf rb=1 grid=2x1
res_respf_gelu fp32_split | resident ns16 plain pf1 respf rb=1 grid=2x1
res_d2s_k32 fp32_mfma | resident ns16 plain d2s pf0 rb=2 grid=2x1
res_d2s_k32 fp32_split | resident ns16 plain d2s pf0 rb=2 grid=2x1
res_d2s_k32 bf16 | bx_stream mb1 nacc2 plain d2s wt rd4 grid=2x2
res_d2s_k32 bf16_mfma | resident ns16 plain d2s pf0 rb=2 grid=2x1
res_d2s_k16_m16 fp32_mfma | resident ns16 plain d2s pf0 rb=1 grid=1x1
res_d2s_k16_m16 fp32_split | resident ns16 plain d2s pf0 rb=1 grid=1x1
res_d2s_relu fp32_mfma | resident ns16 plain d2s pf1 rb=1 grid=1x1
res_d2s_relu fp32_split | resident ns16 plain d2s pf1 rb=1 grid=1x1
res_lnbwd_k32 fp32_mfma | resident ns16 plain lnbwd pf3 rb=1 grid=4x1
res_lnbwd_k32 fp32_split | resident ns16 plain lnbwd pf3 rb=1 grid=4x1
res_lnbwd_k32_gadd fp32_mfma | resident ns16 plain lnbwd pf3 gadd rb=1 grid=4x1
res_lnbwd_k32_gadd fp32_split | resident ns16 plain lnbwd pf3 gadd rb=1 grid=4x1
res_lnbwd_k64 fp32_mfma | resident ns32 plain lnbwd pf3 rb=1 grid=4x1
res_lnbwd_k64 fp32_split | resident ns32 plain lnbwd pf3 rb=1 grid=4x1
res_lnbwd_k64 bf16 | resident ns32 plain lnbwd pf3 rb=1 grid=4x1
res_lnbwd_k64 bf16_mfma | resident ns32 plain lnbwd pf3 rb=1 grid=4x1
res_lnbwd_k64_gadd fp32_mfma | resident ns32 plain lnbwd pf3 gadd rb=1 grid=4x1
res_lnbwd_k64_gadd fp32_split | resident ns32 plain lnbwd pf3 gadd rb=1 grid=4x1
res_lnbwd_k64_gadd bf16 | resident ns32 plain lnbwd pf3 gadd rb=1 grid=4x1
res_lnbwd_k64_gadd bf16_mfma | resident ns32 plain lnbwd pf3 gadd rb=1 grid=4x1
res_lnbwd_k32_relu fp32_mfma | resident ns16 plain lnbwd pf3 gadd rb=1 grid=2x1
res_lnbwd_k32_relu fp32_split | resident ns16 plain lnbwd pf3 gadd rb=1 grid=2x1
str_small_k16 fp32_mfma | stream mb1 nacc1 plain grid=4x1
str_small_k32_ln fp32_mfma | stream mb1 nacc1 plain ln grid=4x1
str_small_k32_ln bf16 | stream mb1 nacc1 plain ln grid=4x1
str_small_k32_ln bf16_mfma | stream mb1 nacc1 plain ln grid=4x1
str_none_mb1_n1 fp32_mfma | stream mb1 nacc1 plain grid=2x2
str_none_mb1_n2 fp32_mfma | stream mb1 nacc2 plain grid=256x1
str_none_mb1_n4 fp32_mfma | stream mb1 nacc4 plain grid=256x1
str_none_mb2_n4 fp32_mfma | stream mb2 nacc4 plain grid=512x1
str_ln_mb1_n1 fp32_mfma | stream mb1 nacc1 plain ln grid=2x2
str_ln_mb1_n2 fp32_mfma | stream mb1 nacc2 plain ln grid=256x1
str_ln_mb1_n4 fp32_mfma | stream mb1 nacc4 plain ln grid=256x1
str_ln_mb2_n4 fp32_mfma | stream mb2 nacc4 plain ln grid=512x1
str_gelu_mb1_n1 fp32_mfma | stream mb1 nacc1 plain gelu grid=2x2
str_gelu_mb1_n2 fp32_mfma | stream mb1 nacc2 plain gelu grid=256x1
str_gelu_mb1_n4 fp32_mfma | stream mb1 nacc4 plain gelu grid=256x1
str_gelu_mb2_n4 fp32_mfma | stream mb2 nacc4 plain gelu grid=512x1
str_bmul_mb1_n1 fp32_mfma | stream mb1 nacc1 plain bmul grid=2x2
str_bmul_mb1_n2 fp32_mfma | stream mb1 nacc2 plain bmul grid=256x1
str_bmul_mb1_n4 fp32_mfma | stream mb1 nacc4 plain bmul grid=256x1
str_bmul_mb2_n4 fp32_mfma | stream mb2 nacc4 plain bmul grid=512x1
str_ks4_n2 fp32_mfma | stream mb1 nacc2 plain ks4 grid=5x1
str_ks4_ln fp32_mfma | stream mb1 nacc2 plain ln ks4 grid=5x1
str_ks4_gelu fp32_mfma | stream mb1 nacc2 plain gelu ks4 grid=5x1
str_ks4_bmul fp32_mfma | stream mb1 nacc2 plain bmul ks4 grid=5x1
str_ks4_k258 fp32_mfma | stream mb1 nacc2 plain ks4 grid=1x1
str_s2d fp32_mfma | stream mb1 nacc2 s2d grid=2x2
str_s2d fp32_split | stream mb1 nacc2 s2d grid=2x2
str_s2d_ks4 fp32_mfma | stream mb1 nacc2 s2d ks4 grid=1x1
str_s2d_ks4_cin33 fp32_mfma | stream mb1 nacc2 s2d ks4 grid=2x2
str_s2d_2d_cin5 fp32_mfma | stream mb1 nacc2 s2d2 grid=2x2
str_s2d_2d_cin5 bf16 | stream mb1 nacc2 s2d2 grid=2x2
str_s2d_2d_cin5 bf16_mfma | stream mb1 nacc2 s2d2 grid=2x2
str_s2d_2d_ks4_cin65 fp32_mfma | stream mb1 nacc2 s2d2 ks4 grid=1x1
str_s2d_2d fp32_mfma | stream mb1 nacc2 s2d2 grid=2x2
str_s2d_2d bf16 | stream mb1 nacc2 s2d2 grid=2x2
str_s2d_2d bf16_mfma | stream mb1 nacc2 s2d2 grid=2x2
str_s2d_2d_ks4 fp32_mfma | stream mb1 nacc2 s2d2 ks4 grid=1x1
str_k3_mb1 fp32_mfma | stream mb1 nacc4 k3 grid=2x1
str_k3_mb1 bf16 | stream mb1 nacc4 k3 grid=2x1
str_k3_mb1 bf16_mfma | stream mb1 nacc4 k3 grid=2x1
str_k3_mb2 fp32_mfma | stream mb2 nacc4 k3 grid=512x1
str_k3_2d_mb1 fp32_mfma | stream mb1 nacc4 k3_2 grid=2x2
str_k3_2d_mb1 bf16 | stream mb1 nacc4 k3_2 grid=2x2
str_k3_2d_mb1 bf16_mfma | stream mb1 nacc4 k3_2 grid=2x2
str_k3_2d_mb2 fp32_mfma | stream mb2 nacc4 k3_2 grid=512x1
str_d2s_mb1 fp32_mfma | stream mb1 nacc4 plain d2s grid=2x2
str_d2s_mb1 bf16 | stream mb1 nacc4 plain d2s grid=2x2
str_d2s_mb1 bf16_mfma | stream mb1 nacc4 plain d2s grid=2x2
str_d2s_mb2 fp32_mfma | stream mb2 nacc4 plain d2s grid=512x1
str_d2s_2d_mb1 fp32_mfma | stream mb1 nacc4 plain d2s2 grid=2x2
str_d2s_2d_mb1 bf16 | stream mb1 nacc4 plain d2s2 grid=2x2
str_d2s_2d_mb1 bf16_mfma | stream mb1 nacc4 plain d2s2 grid=2x2
str_d2s_2d_mb2 fp32_mfma | stream mb2 nacc4 plain d2s2 grid=512x1
p32_4095_not_taken fp32_mfma | stream mb1 nacc4 plain ln grid=1024x1
p32_4096_ln fp32_mfma | p32 pf2 grid=512x1
p32_4096_ln bf16 | p32 pf2 grid=512x1
p32_4096_ln bf16_mfma | p32 pf2 grid=512x1
p32_b3_ln_m3 fp32_mfma | p32 pf2 grid=512x1
p32_plain_eact fp32_mfma | p32 pf0 grid=512x1
p32_plain_eact bf16 | bx_stream mb1 nacc4 plain rd2 grid=1026x1
p32_plain_eact bf16_mfma | p32 pf0 grid=512x1
chain64_lnb fp32_mfma | chain64_lnb fp32 grid=4x1
chain64_lnb fp32_split | chain64_lnb split grid=4x1
chain64_lnb bf16 | chain64_lnb split grid=4x1
chain64_lnb bf16_mfma | chain64_lnb fp32 grid=4x1
head_m3 fp32_mfma | head m4 grid=512x1
head_m3 bf16 | head m4 grid=512x1
head_m3 bf16_mfma | head m4 grid=512x1
head_m2_nobias fp32_mfma | head m2 grid=512x1
"""
REACHED = {}
for _l in _REACHED_TEXT.strip().splitlines():
    _k, _v = _l.split(" | ")
    REACHED[tuple(_k.split())] = _v
