"""Cases, reference and bounds of the group norm tests (tests/test_group_norm_cpu.py: the host emulation;
tests/test_gpu_group_norm.py: the kernels).

Reference: F.group_norm, then the activation, and its autograd in float64 on the CPU, on the very inputs the kernel sees (bf16
inputs upcast).  Bounds: those of tests/inorm_cases.py — y and gx element-wise |got − ref| <= u (|ref| + 1e-3 max|ref|),
u = 2^-23 (fp32) / 2^-7 (bf16); dγ, dβ: |got − ref| <= 2^-23 |ref| + 2^-30 Σ|terms|.

Condition on the inputs, asserted by `reference`: no float64 pre-activation z lies within 2^-30 max|z| of zero, so that a gate is
never a matter of float64 rounding (the constant group, where z = β exactly, is the exception and is tested on its own)."""
import torch
import torch.nn.functional as F

import inorm_cases as IC
from inorm_cases import DTYPES, U, _randn, ratio_elementwise, ratio_param, to_device  # noqa: F401

EPS = 1e-5
ACTS = [None, "relu", "leaky_relu"]
ACT_IDS = ["none", "relu", "leaky_relu"]
SLOPE = 0.01


def seams(one_pass_max, chunks):
    """spans at which the code takes another path, from the library's own answers (chunks(cg, V)); each realised with cg = 1
    (V = span) and with cg = 8 (V = span / 8: the span is moved to the next multiple of 8 on the same side of the seam)"""
    s = IC.seams(one_pass_max, lambda n: chunks(1, n))
    L = s["chunk_last_of_1"]
    assert one_pass_max % 8 == 0 and L % 8 == 0
    s8 = {"one_pass_max-1": one_pass_max - 8, "one_pass_max": one_pass_max, "one_pass_max+1": one_pass_max + 8,
          "chunk_last_of_1": L, "chunk_first_of_2": L + 8, "chunk_3_plus_5": 3 * L + 8}
    assert chunks(8, (L + 8) // 8) == 2 and chunks(8, L // 8) == 1 and chunks(8, (3 * L + 8) // 8) == 4
    out = {f"{k}_cg1": (1, v) for k, v in s.items()}
    out.update({f"{k}_cg8": (8, v // 8) for k, v in s8.items()})
    return out


# name: (tensor, G)
FIXED = {
    "cg3_odd_v": lambda: (_randn((3, 24, 777), 1), 8),
    "odd_v_two_launch": lambda: (_randn((2, 16, 4099), 2), 8),
    "smallest_v": lambda: (_randn((2, 8, 2), 3), 8),
    "one_group": lambda: (_randn((2, 6, 301), 4), 1),
    "one_group_two_launch": lambda: (_randn((2, 12, 1001), 14), 1),
    "group_per_channel": lambda: (_randn((2, 6, 301), 5), 6),
    "tiny_planes_3d": lambda: (_randn((2, 512, 2, 2, 2), 6), 8),
    "v_below_the_access": lambda: (_randn((2, 40, 3), 15), 2),
    "mean_far_from_zero": lambda: (1000 + _randn((2, 16, 1025), 8), 8),
    "large_scale_offset": lambda: (1e4 * _randn((2, 6, 1023), 9) + 5e5, 2),
    "var_near_eps": lambda: (1e-3 * _randn((2, 6, 1023), 10), 2),
    "storage_offset_odd_v": lambda: (_randn((1 + 2 * 6 * 4099,), 12)[1:].view(2, 6, 4099), 2),
    "permuted": lambda: (_randn((2, 9, 11, 6), 13).permute(0, 3, 1, 2), 3),
    "ragged_chunks": lambda: (300 * _randn((1, 32, 70001), 11) + 7, 8),
    "unet_stage": lambda: (_randn((2, 64, 8, 8, 8), 16), 8),
}
SEAMS = [f"{k}_cg{c}" for c in (1, 8) for k in IC.SEAMS]
CASES = sorted(FIXED) + SEAMS


def make(name, dtype, affine, seam_sizes):
    """x (CPU, of `dtype`, possibly a view), G, weight, bias (fp32 or None), gy (of `dtype`)"""
    if name in FIXED:
        x, G = FIXED[name]()
    else:
        cg, V = seam_sizes[name]
        x, G = _randn((1, 2 * cg, V), 20 + SEAMS.index(name)), 2
    if dtype != torch.float32:
        if x.is_contiguous() and x.storage_offset():      # keep the one-element storage offset in the narrower type
            flat = torch.zeros(1 + x.numel(), dtype=dtype)
            flat[1:] = x.reshape(-1).to(dtype)
            x = flat[1:].view(x.shape)
        else:
            x = x.to(dtype)
    C = x.shape[1]
    g = torch.Generator().manual_seed(99)
    w = (1 + 0.5 * torch.randn(C, generator=g)) if affine else None
    b = torch.randn(C, generator=g) if affine else None
    gy = torch.randn(x.shape, generator=g).to(dtype)
    return x, G, w, b, gy


def activation(z, act, slope=SLOPE):
    return F.relu(z) if act == "relu" else F.leaky_relu(z, slope) if act == "leaky_relu" else z


def reference(x, G, w, b, gy, act, slope=SLOPE, eps=EPS, constant=False):
    """float64: y, gx, gw, gb and the Σ|terms| of gw, gb; asserts the condition on the inputs"""
    x64 = x.double().contiguous().requires_grad_(True)
    ps = [p.double().requires_grad_(True) for p in (w, b) if p is not None]
    z = F.group_norm(x64, G, ps[0] if ps else None, ps[1] if ps else None, eps)
    if not constant:
        zd = z.detach().abs()
        assert float(zd.min()) > 2.0 ** -30 * float(zd.max()), "a pre-activation within float64 rounding of a gate"
    y = activation(z, act, slope)
    g64 = gy.double()
    grads = torch.autograd.grad(y, [x64] + ps, g64)
    out = {"y": y.detach(), "gx": grads[0]}
    if ps:
        dims = [0] + list(range(2, x.dim()))
        zd = z.detach()
        gate = torch.ones_like(zd) if act is None else torch.where(zd > 0, 1.0, 0.0 if act == "relu" else slope).double()
        xhat = F.group_norm(x64.detach(), G, None, None, eps)
        gp = g64 * gate
        out.update(gw=grads[1], gb=grads[2], gw_terms=(gp * xhat).abs().sum(dims), gb_terms=gp.abs().sum(dims))
    return out


def check(got, ref, dtype, note=None):
    """got: dict y, gx[, gw, gb]; prints each achieved fraction of its bound before asserting"""
    return IC.check(got, ref, dtype, note)
