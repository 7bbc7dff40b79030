"""Inputs, float64 references and bounds shared by tests/test_gpu_deep_supervision.py and its CPU-side companion
tests/test_deep_supervision_cpu.py (which pins that the references alone stay inside half of the bounds).

The reference is written independently of the package's composed path: the target of a coarse level is the STRIDED SLICE
target[..., r//2::r] per axis (what nearest-exact is for an integer ratio r), taken in float64, followed by the composed
loss of tests/loss_adamw_cases.py in float64.  Bounds are that file's: LOSS_REL / LOSS_FLOOR per level and GRAD_REL per
level gradient (over the tensor and over every (b, c) plane, floor = 0); the weighted sum adds L·2^-23·Σ w|l| for its L
products and L − 1 additions in fp32."""
from __future__ import annotations

import functools

import torch
from torch import nn

import factorizer_amd as ft
import loss_adamw_cases as L
import parity as P

KIND_OF = {1: "bce"}          # C = 1 is Dice + BCE, C >= 2 Dice + CE (what ft.DiceCELoss evaluates)

# name: (target extents, extents of the coarse levels); level 0 always has the target's extents
GEOMS = {
    "3d": ((16, 12, 8), ((8, 6, 4), (4, 3, 2))),
    "mixed_1_2_4": ((8, 12, 16), ((8, 6, 4),)),
    "ratio3": ((12, 12, 12), ((4, 4, 4),)),
    "2d": ((32, 24), ((16, 12), (8, 6))),
    "1d": ((64,), ((32,), (16,))),
    "two_chunks": ((128, 64, 64), ((64, 32, 32),)),   # 65 536 level voxels: two chunks of fz_dice_bce_chunks
    # the input regimes: 1 536 level voxels, so that every plane of "saturated_1pct" holds wrong voxels (at the 24 .. 192 voxels
    # of the levels above, 0.99^V of its planes hold none and ARE the regime "saturated", whose bound carries the kink term)
    "regimes": ((32, 24, 16), ((16, 12, 8),)),
}
MATRIX = [(geom, B, C) for geom in ("3d", "mixed_1_2_4", "ratio3", "2d", "1d") for B in (1, 2, 9) for C in (1, 2, 3, 8)] \
    + [("two_chunks", 1, 2)]
REGIME_CASES = [(C, regime) for C in (3, 1) for regime in L.REGIMES]      # through geometry "regimes" at B = 2
SCALE = 1.7


def kind_of(C):
    return KIND_OF.get(C, "ce")


def prod(s):
    n = 1
    for v in s:
        n *= v
    return n


def slice_target(t, size):
    """the strided pick r·i + r//2 on every spatial axis (integer ratios only)"""
    for ax, (st, sl) in enumerate(zip(t.shape[2:], size)):
        assert st % sl == 0
        r = st // sl
        t = t[(slice(None),) * (2 + ax) + (slice(r // 2, None, r),)]
    assert tuple(t.shape[2:]) == tuple(size)
    return t


def weights_of(mode, n, explicit=None):
    """the specification's level weights, restated"""
    if explicit is not None and len(explicit) >= n:
        return list(explicit[:n])
    return {"same": [1.0] * n, "exp": [max(0.5 ** l, 0.0625) for l in range(n)], "two": [1.0] + [0.5] * (n - 1)}[mode][:n]


@functools.lru_cache(maxsize=None)
def make_case(geom, B, C, regime="randn3", seed=0):
    """(list of fp32 CPU logits, finest first; fp32 CPU target at the finest extents).  Every level is one regime of
    loss_adamw_cases against ITS target — the slice of the full-resolution one: for the saturated regimes, whose logits are
    built from their target, the drawn logits change sign where the drawn target and the slice differ."""
    St, coarse = GEOMS[geom]
    z0, t0 = L.make_inputs(regime, B, C, prod(St), seed)
    t = t0.reshape(B, C, *St)
    zs = [z0.reshape(B, C, *St)]
    for l, S in enumerate(coarse, 1):
        z, td = L.make_inputs(regime, B, C, prod(S), seed + 17 * l)
        z, td = z.reshape(B, C, *S), td.reshape(B, C, *S)
        if regime in ("saturated", "saturated_1pct"):
            z = torch.where(slice_target(t, S) == td, z, -z)
        zs.append(z.contiguous())
    return zs, t.contiguous()


def level_reference(kind, z, t, wscale, dtype=torch.float64):
    """(loss_l, d(wscale·loss_l)/dz) of one level from the sliced target, on the CPU in `dtype`"""
    return L.reference(kind, z, slice_target(t.detach().cpu().to(dtype), z.shape[2:]), wscale, dtype=dtype)


def reference(zs, t, w, scale=SCALE, dtype=torch.float64):
    """([loss_l], [d(scale·Σ w·loss)/dz_l], Σ w_l·loss_l) in `dtype`"""
    kind = kind_of(zs[0].shape[1])
    out = [level_reference(kind, z, t, wl * scale, dtype) for wl, z in zip(w, zs)]
    ls = [o[0] for o in out]
    return ls, [o[1] for o in out], sum(wl * l.item() for wl, l in zip(w, ls))


@functools.lru_cache(maxsize=None)
def case_reference(geom, B, C, regime="randn3", seed=0, mode="exp"):
    zs, t = make_case(geom, B, C, regime, seed)
    return reference(zs, t, tuple(weights_of(mode, len(zs))))


def loss_bound(l64s, w):
    """Σ w·(LOSS_REL·|l64_l| + LOSS_FLOOR) + L·2^-23·Σ w·|l64_l|"""
    wl = sum(wi * abs(li.item()) for wi, li in zip(w, l64s))
    return sum(wi * (L.LOSS_REL * abs(li.item()) + L.LOSS_FLOOR) for wi, li in zip(w, l64s)) + len(w) * 2.0 ** -23 * wl


def check(name, zs, t, w, loss, grads, regime="randn3", scale=SCALE, frac=1.0, ref=None):
    """the total loss and every level's gradient against float64 (`ref`: a `reference` of these inputs computed before), at
    `frac` of the bounds (KINK regimes: as tests/test_gpu_loss.py treats them — the bound carries 30 x the fp32-vs-float64
    distance of the composed form)"""
    kind = kind_of(zs[0].shape[1])
    l64s, g64s, l64 = ref or reference(zs, t, w, scale)
    err, bound = abs(float(loss) - l64), frac * loss_bound(l64s, w)
    P.note(f"{name}: total loss", err=err, bound=bound)
    assert err <= bound, f"{name}: |l - l64| = {err:.3e} > {bound:.3e}"
    why = L.KINK.get((kind, regime))
    for l, (z, gd, g64) in enumerate(zip(zs, grads, g64s)):
        k, kp = 0.0, None
        if why:
            _, g32 = level_reference(kind, z, t, w[l] * scale, dtype=torch.float32)
            k, kp = L.kink(g32, g64)
        gd = gd.detach().float().cpu()
        P.close(f"{name}: level {l} dL/dz", gd, g64, rel=frac * L.GRAD_REL, floor=0.0, extra=frac * k, why=why)
        d, s = L.plane_errors(gd, g64)
        lim = frac * (L.GRAD_REL * s + (kp if why else 0.0))
        assert (d <= lim).all(), f"{name}: level {l} plane {(d - lim).argmax().item()}: {d.max().item():.3e}"


# ---- the num_deep_supr networks: a 3-D Factorizer with three heads, a 2-D Deconver with two ----------------------------------
def tiny_factorizer(width=(8, 16, 32), spatial=(16, 16, 16), num_deep_supr=3):
    return ft.Factorizer(2, 3, spatial, encoder_depth=(1, 1, 1), encoder_width=width, strides=(1, 2, 2),
                         decoder_depth=(1, 1), reshape=(ft.SWMatricize, {"head_dim": 8, "patch_size": 4}), rank=1,
                         num_iters=2, num_deep_supr=num_deep_supr)


def tiny_deconver2d(width=(8, 16, 32), num_deep_supr=2):
    return ft.Deconver(3, 1, spatial_dims=2, encoder_depth=(1, 1, 1), encoder_width=width, strides=(1, 2, 2),
                       decoder_depth=(1, 1), norm=nn.InstanceNorm2d, groups=-1, ratio=1, kernel_size=(3, 3), num_iters=1,
                       num_deep_supr=num_deep_supr)
