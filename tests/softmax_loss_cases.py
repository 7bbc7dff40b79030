"""Inputs, the float64 reference and the closed-form gradient shared by tests/test_softmax_loss_cpu.py and
tests/test_gpu_softmax_loss.py: the class-index form DiceCELoss(softmax=True, to_onehot_y=True, include_background,
squared_pred) of factorizer_amd/losses.py.

`reference` is an independent restatement on the CPU — softmax, a masked one-hot, F.cross_entropy with ignore_index for the
labels that name no class and the mean taken over B·V — not `dice_ce_softmax_loss_composed` itself; the CPU file holds the
composed form to it.  The bounds are the ones the sigmoid kernels are held to (tests/loss_adamw_cases.py: LOSS_REL,
LOSS_FLOOR, GRAD_REL): the same arithmetic class."""
from __future__ import annotations

import torch
import torch.nn.functional as F

REGIMES = ["randn3", "saturated", "saturated_1pct", "absent", "oneclass", "zeros", "shift1e4", "oob_1pct"]

# With every voxel saturated AND correct, p_y = 1 − (C − 1)·e^-40 rounds to 1.0f (and to 1.0 in float64: the reference's own
# gradient at the labelled channel is exactly 0): at the labelled channel p − t and a_y − Σ a_c p_c are rounding residues of
# any fp32 evaluation, while every gradient of the tensor is itself O(e^-40).  The
# bound there carries 30 x the fp32-vs-float64 distance of this file's reference (loss_adamw_cases.kink), as the saturated
# BCE regime of tests/test_gpu_loss.py does; test_softmax_loss_cpu.py shows that only this regime needs it.
KINK = {"saturated": "every voxel saturated and correct: softmax_y rounds to 1.0f, the gradient at the labelled channel is "
                     "below fp32 resolution of 1; bound carries 30 x (reference in fp32 − float64)"}


def make_inputs(regime: str, B: int, C: int, V: int, seed: int = 0):
    """(logits fp32 (B, C, V), labels uint8 (B, 1, V)) on the CPU"""
    g = torch.Generator().manual_seed(1000 * seed + 31 * REGIMES.index(regime) + C)
    y = torch.randint(0, C, (B, 1, V), generator=g)
    z = torch.randn(B, C, V, generator=g) * 3
    if regime in ("randn3",):
        pass
    elif regime in ("saturated", "saturated_1pct"):
        z = torch.full((B, C, V), -20.0).scatter_(1, y, 20.0)            # z_y = +20, the others −20
        if regime == "saturated_1pct":                                    # 1 % of the voxels carry another label
            wrong = torch.rand(B, 1, V, generator=g) < 0.01
            y = torch.where(wrong, (y + 1 + torch.randint(0, C - 1, (B, 1, V), generator=g)) % C, y)
    elif regime == "absent":                                              # class C − 1 does not occur in sample 0
        y[0] = y[0] % (C - 1)
    elif regime == "oneclass":                                            # the last sample is class 1 throughout
        y[B - 1] = 1
    elif regime == "zeros":
        z = torch.zeros(B, C, V)
    elif regime == "shift1e4":
        # multiples of 2^-8 below 2^5 in magnitude: z + 1e4 is exact in fp32 (ulp 2^-10), so the shifted logits differ from
        # `unshifted(z)` by the common shift alone, which softmax and the CE term ignore
        z = torch.round(z.clamp(-30, 30) * 256) / 256 + 1e4
    elif regime == "oob_1pct":                                            # 1 % of the labels name no class: C and 255
        r = torch.rand(B, 1, V, generator=g)
        y = torch.where(r < 0.005, torch.full_like(y, C), y)
        y = torch.where(r > 0.995, torch.full_like(y, 255), y)
    else:
        raise KeyError(regime)
    return z.contiguous(), y.to(torch.uint8).contiguous()


def unshifted(z):
    """the logits of the shift1e4 regime without their shift (exact)"""
    return z - 1e4


def label_classes(y, C):
    """(idx int64 (B, *S), ok bool) of a label map (B, 1, *S): .long() conversion, ok iff 0 <= idx < C"""
    lab = y.detach().cpu()[:, 0]
    ok = torch.ones_like(lab, dtype=torch.bool)
    if lab.is_floating_point():
        ok = torch.isfinite(lab)
        lab = torch.where(ok, lab, torch.zeros_like(lab))
    idx = lab.long()
    ok = ok & (idx >= 0) & (idx < C)
    return idx, ok


def reference(z, y, sq: bool, ib: bool, scale: float = 1.0, smooth: float = 1e-5, dtype=torch.float64):
    """(loss, d(scale·loss)/dz) of the class-index DiceCE on the CPU in `dtype`; z (B, C, *S), y (B, 1, *S)"""
    zz = z.detach().cpu().to(dtype).requires_grad_(True)
    C = zz.shape[1]
    idx, ok = label_classes(y, C)
    t = (F.one_hot(torch.where(ok, idx, torch.zeros_like(idx)), C).movedim(-1, 1) * ok.unsqueeze(1)).to(dtype)
    p = torch.softmax(zz, dim=1)
    dims = tuple(range(2, zz.ndim))
    c0 = 0 if ib else 1
    inter, ground = (p * t).sum(dims), t.sum(dims)
    pred = (p * p).sum(dims) if sq else p.sum(dims)
    dice = (1.0 - (2.0 * inter + smooth) / (pred + ground + smooth))[:, c0:].mean()
    ce = F.cross_entropy(zz, torch.where(ok, idx, torch.full_like(idx, -100)), ignore_index=-100, reduction="sum") / ok.numel()
    loss = dice + ce
    (g,) = torch.autograd.grad(loss * scale, zz)
    return loss.detach(), g


def closed_form_grad(z, y, sq: bool, ib: bool, g: float = 1.0, smooth: float = 1e-5):
    """dL/dz by the formula of the module docstring of factorizer_amd/losses.py, in float64"""
    zz = z.detach().cpu().double()
    B, C = zz.shape[:2]
    V = zz[0, 0].numel()
    idx, ok = label_classes(y, C)
    t = (F.one_hot(torch.where(ok, idx, torch.zeros_like(idx)), C).movedim(-1, 1) * ok.unsqueeze(1)).double()
    p = torch.softmax(zz, dim=1)
    dims = tuple(range(2, zz.ndim))
    c0 = 0 if ib else 1
    shape = (B, C) + (1,) * (zz.ndim - 2)
    num = (2.0 * (p * t).sum(dims) + smooth).view(shape)
    den = (((p * p) if sq else p).sum(dims) + t.sum(dims) + smooth).view(shape)
    cd, cb = 1.0 / (B * (C - c0)), 1.0 / (B * V)
    a = cd * (-2.0 * t / den + num * (2.0 * p if sq else torch.ones_like(p)) / den ** 2)
    a[:, :c0] = 0.0
    return g * (p * (a - (a * p).sum(1, keepdim=True)) + cb * (p - t) * ok.unsqueeze(1))   # no CE term without a class
