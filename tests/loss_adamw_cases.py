"""Inputs, float64 references and bounds shared by tests/test_gpu_loss.py, tests/test_gpu_adamw.py and their CPU-side
companion tests/test_loss_adamw_cpu.py (which pins that the references alone stay well inside the bounds).

Loss: every regime below is one way a training run feeds csrc/loss.hip — the reference is the package's composed
form evaluated on the CPU in float64.  AdamW: the reference is `adamw64`, a restatement of torch.optim.AdamW's
single-tensor update in float64 (checked against torch itself in the CPU file)."""
from __future__ import annotations

import math

import torch

from factorizer_amd.losses import dice_bce_loss_composed, dice_ce_loss_composed

COMPOSED = {"ce": dice_ce_loss_composed, "bce": dice_bce_loss_composed}

REGIMES = ["randn3", "saturated", "saturated_1pct", "empty_m20", "empty_randn", "soft", "onehot", "ones", "zeros"]

# Regimes whose gradient NO fp32 evaluation holds to 1e-4 of a plane's own maximum: with every voxel saturated AND correct,
# the largest gradient of a plane is itself a rounding residue — sigmoid(z) − t with sigmoid(z) = 1 − e^-z rounding to 1.0f for
# z > 17 (BCE term), softmax_c · Σt − t with softmax_c = 1 − O(e^-40) (CE term).  The bound there carries the measured
# fp32-vs-float64 distance of the composed path times 30 (`kink`), as tests/test_gpu_nmf_solvers.py does;
# tests/test_loss_adamw_cpu.py::test_kink_regimes_are_the_ones_fp32_cannot_hold shows that exactly these need it.
KINK = {("bce", "saturated"): "every voxel saturated and correct: max|grad| of a plane is sigmoid(z) − t below 2^-24, "
                              "lost by any fp32 sigmoid; bound carries 30 x (composed fp32 − float64)"}


def make_inputs(regime: str, B: int, C: int, V: int, seed: int = 0):
    """(logits, target) as fp32 CPU tensors of shape (B, C, V)."""
    g = torch.Generator().manual_seed(1000 * seed + REGIMES.index(regime))
    t = (torch.rand(B, C, V, generator=g) > 0.5).float()
    z = torch.randn(B, C, V, generator=g) * 3
    if regime == "randn3":
        pass
    elif regime in ("saturated", "saturated_1pct"):
        z = (2 * t - 1) * (20 + 40 * torch.rand(B, C, V, generator=g))
        if regime == "saturated_1pct":
            z = torch.where(torch.rand(B, C, V, generator=g) < 0.01, -z, z)
    elif regime in ("empty_m20", "empty_randn"):
        # one (b, c) plane and one whole batch item without foreground (BraTS crops outside the tumour)
        z = torch.randn(B, C, V, generator=g)
        bg = -20 + 0.5 * torch.randn(B, C, V, generator=g)
        t[0, C - 1] = 0
        t[B - 1] = 0
        if regime == "empty_m20":
            z[0, C - 1] = bg[0, C - 1]
            z[B - 1] = bg[B - 1]
    elif regime == "soft":
        t = torch.rand(B, C, V, generator=g)
    elif regime == "onehot":
        idx = torch.randint(0, C, (B, 1, V), generator=g)
        t = torch.zeros(B, C, V).scatter_(1, idx, 1.0)
    elif regime == "ones":
        t = torch.ones(B, C, V)
    elif regime == "zeros":
        t = torch.zeros(B, C, V)
    else:
        raise KeyError(regime)
    return z.contiguous(), t.contiguous()


def reference(kind: str, z, t, scale: float = 1.0, dtype=torch.float64):
    """(loss, d(scale·loss)/dz) of the composed form on the CPU in `dtype`."""
    zz = z.detach().cpu().to(dtype).requires_grad_(True)
    loss = COMPOSED[kind](zz, t.detach().cpu().to(dtype))
    (g,) = torch.autograd.grad(loss * scale, zz)
    return loss.detach(), g


LOSS_REL, LOSS_FLOOR = 1e-5, 1e-6      # |l − l64| ≤ 1e-5·|l64| + 1e-6
GRAD_REL = 1e-4                        # max|g − g64| ≤ 1e-4·max|g64|, over the tensor and over every (b, c) plane
# The gradients are O(1/(B·V)) — 1e-7 at 128^3 — so parity.close's default absolute floor of 1e-6 would make every
# gradient comparison vacuous: they run with floor = 0.


def plane_errors(g, g64):
    """per (b, c) plane: (max|g − g64|, max|g64|), each of shape (B, C)"""
    B, C = g64.shape[:2]
    d = (g.detach().cpu().double().reshape(B, C, -1) - g64.reshape(B, C, -1)).abs().amax(2)
    return d, g64.reshape(B, C, -1).abs().amax(2)


def kink(g32, g64):
    """30 x the fp32-vs-float64 distance of the composed path, over the tensor and per plane"""
    d, _ = plane_errors(g32, g64)
    return 30.0 * d.max().item(), 30.0 * d


# ---- AdamW ------------------------------------------------------------------------------------------------------------------
def adamw64(p, g, m, v, t, lr, betas=(0.9, 0.999), eps=1e-8, wd=1e-2):
    """torch.optim.AdamW's single-tensor update (decoupled decay, no amsgrad) on float64 tensors; returns (p, m, v)."""
    b1, b2 = betas
    p = p * (1.0 - lr * wd)
    m = b1 * m + (1.0 - b1) * g
    v = b2 * v + (1.0 - b2) * g * g
    denom = v.sqrt() / math.sqrt(1.0 - b2 ** t) + eps
    return p - (lr / (1.0 - b1 ** t)) * (m / denom), m, v


GRAD_REGIMES = ["randn", "loguniform", "zeros10", "allzero"]


def make_grad(regime: str, n: int, gen):
    """one fp32 CPU gradient of n elements"""
    if regime == "randn":
        return torch.randn(n, generator=gen)
    if regime == "allzero":
        return torch.zeros(n)
    sign = torch.where(torch.rand(n, generator=gen) < 0.5, -1.0, 1.0)
    g = sign * 10.0 ** (-8 + 6 * torch.rand(n, generator=gen))   # |g| log-uniform in 1e-8 .. 1e-2, as real gradients are
    if regime == "zeros10":
        g = torch.where(torch.rand(n, generator=gen) < 0.1, torch.zeros(n), g)
    return g


def make_state(n: int, gen):
    """(p0, m0, v0): weight-like parameters (randn·0.05) and non-trivial moments of a run in progress"""
    p0 = torch.randn(n, generator=gen) * 0.05
    m0 = torch.randn(n, generator=gen) * 1e-3
    v0 = (torch.randn(n, generator=gen) * 1e-3) ** 2 + 1e-12
    return p0, m0, v0


def param_bound_terms(dp64, p64, steps):
    """the two terms of  max|Δp − Δp64| ≤ 1e-4·max|Δp64| + steps·2^-23·max|p|  (the kernel rounds p twice per step — at the
    decay multiply and at the subtract — half an ulp of p each)"""
    return 1e-4 * dp64.abs().max().item(), steps * 2.0 ** -23 * p64.abs().max().item()
