"""Native group norm with a fused activation: ft.GroupNorm, ft.group_norm, ft.convert_group_norm.

The reference's CNN blocks (factorizer/layers/conv.py; here cnn.py) norm with ``nn.GroupNorm(8, C)`` and activate with
``nn.LeakyReLU`` right behind it.  ``ft.GroupNorm`` subclasses the framework's class, with the same constructor, defaults and
``state_dict`` keys; on a device tensor of fp32 / bf16 with fp32 parameters it runs csrc/gnorm.hip: float64 sums about the group's
first element in a fixed order, one rounding per stored element, no atomics.  ``ft.group_norm(..., act=...)`` is the norm and the
activation behind it (None, "relu", "leaky_relu") as ONE autograd node and one launch each way for groups of up to
``fz_gnorm_one_pass_max()`` elements.

Everything outside the native gate runs ``F.group_norm`` and then the framework's activation: silently on the CPU (bit-identical
to the framework), with one ``composed.warn_once`` naming the reason on a device (`fallback_reason`)."""
from __future__ import annotations

import torch
import torch.nn.functional as F
from torch import nn

from . import _native, composed

_NATIVE_DTYPES = (torch.float32, torch.bfloat16)
ACTS = {None: 0, "relu": 1, "leaky_relu": 2}


def fallback_reason(dtype, param_dtypes=()):
    """why a DEVICE tensor of `dtype` does not take the native kernels (None: it does); `param_dtypes`: the types of the
    weight / bias that are present"""
    if dtype not in _NATIVE_DTYPES:
        return f"{str(dtype).replace('torch.', '')} input (the native kernels store float32 or bfloat16)"
    if any(d != torch.float32 for d in param_dtypes):
        return "weight / bias that are not float32"
    return None


def _geometry(x, num_groups):
    B, C = x.shape[0], x.shape[1]
    return B, C, num_groups, x.numel() // (B * C)


def _workspace(x, B, C, G, V):
    n = _native.lib().fz_gnorm_workspace_bytes(B, C, G, V)
    if n < 0:
        raise _native.NativeError(f"fz_gnorm_workspace_bytes({B}, {C}, {G}, {V}): shape out of range")
    return torch.empty(n // 8, dtype=torch.float64, device=x.device)


class GroupNormFn(torch.autograd.Function):
    """y = act((x − mean) rstd γ_c + β_c) per group of a contiguous channels-first device tensor.  Saves x, the float64
    (mean, rstd), γ and β — the backward recomputes the pre-activation; the parameter gradients are complete when backward
    returns (nothing is left in the deferred-finish queue)."""

    @staticmethod
    def forward(ctx, x, weight, bias, num_groups, eps, act, slope):
        x = x.contiguous()
        B, C, G, V = _geometry(x, num_groups)
        y = torch.empty_like(x)
        stats = torch.empty(B * G, 2, dtype=torch.float64, device=x.device)
        ws = _workspace(x, B, C, G, V)
        L = _native.lib()
        _native.check(L.fz_gnorm_fwd(_native.ptr(x), _native.ptr(weight), _native.ptr(bias), _native.ptr(y), _native.ptr(stats),
                                     B, C, G, V, float(eps), act, float(slope), _native.act_dtype(x), _native.ptr(ws),
                                     _native.stream_ptr(x)), "fz_gnorm_fwd")
        ctx.save_for_backward(x, stats, weight, bias)
        ctx.cfg = (G, act, float(slope))
        return y

    @staticmethod
    def backward(ctx, gy):
        x, stats, weight, bias = ctx.saved_tensors
        G, act, slope = ctx.cfg
        B, C, _, V = _geometry(x, G)
        gy = gy.to(x.dtype).contiguous()
        need_x, need_w, need_b = ctx.needs_input_grad[:3]
        gx = torch.empty_like(x)
        gw = torch.empty(C, dtype=torch.float32, device=x.device) if weight is not None and need_w else None
        gb = torch.empty(C, dtype=torch.float32, device=x.device) if bias is not None and need_b else None
        ws = _workspace(x, B, C, G, V)
        L = _native.lib()
        _native.check(L.fz_gnorm_bwd(_native.ptr(x), _native.ptr(gy), _native.ptr(weight), _native.ptr(bias), _native.ptr(stats),
                                     _native.ptr(gx), _native.ptr(gw), _native.ptr(gb), B, C, G, V, act, slope,
                                     _native.act_dtype(x), _native.ptr(ws), _native.stream_ptr(x)), "fz_gnorm_bwd")
        return (gx if need_x else None), gw, gb, None, None, None, None


def launches(channels_per_group: int, spatial: int, backward: bool = False, affine: bool = False) -> int:
    """native launches of one forward (or one backward) over groups of `channels_per_group` planes of `spatial` elements"""
    return _native.lib().fz_gnorm_launches(channels_per_group, spatial, int(backward), int(affine))


def _framework_act(y, act, negative_slope):
    if act == "relu":
        return F.relu(y)
    if act == "leaky_relu":
        return F.leaky_relu(y, negative_slope)
    return y


def group_norm(x, num_groups, weight=None, bias=None, eps=1e-5, act=None, negative_slope=0.01):
    """act(F.group_norm(x, num_groups, weight, bias, eps)) with act in (None, "relu", "leaky_relu"): one native autograd node
    on fp32 / bf16 device tensors of at least 3 dims with fp32 parameters (the output has the input's type; no autocast casting
    of its own), the framework's norm and activation elsewhere."""
    if act not in ACTS:
        raise ValueError(f"group_norm: act must be None, 'relu' or 'leaky_relu', not {act!r}")
    if x.is_cuda and x.dim() >= 3 and x.numel() and x.shape[1] % num_groups == 0:
        F._verify_batch_size([x.size(0) * x.size(1) // num_groups, num_groups] + list(x.size()[2:]))
        why = fallback_reason(x.dtype, [p.dtype for p in (weight, bias) if p is not None])
        if why is None:
            return GroupNormFn.apply(x, weight, bias, num_groups, eps, ACTS[act], negative_slope)
        composed.warn_once(f"group_norm:{why}", f"group norm with {why} is outside the native kernel set; using ATen on device")
    return _framework_act(F.group_norm(x, num_groups, weight, bias, eps), act, negative_slope)


class GroupNorm(nn.GroupNorm):
    """nn.GroupNorm on the native kernels; `forward_act(x, act, negative_slope)` is the norm with the activation behind it
    fused (cnn.py)."""

    def forward(self, input):
        return group_norm(input, self.num_groups, self.weight, self.bias, self.eps)

    def forward_act(self, input, act, negative_slope=0.01):
        return group_norm(input, self.num_groups, self.weight, self.bias, self.eps, act, negative_slope)


def convert_group_norm(module: nn.Module) -> nn.Module:
    """`module` with every nn.GroupNorm in it replaced by ft.GroupNorm (in the manner of ft.convert_instance_norm): parameters,
    eps, the flags and `training` are kept, the state_dict keys do not change, everything else is left alone.  Idempotent."""
    out = module
    if type(module) is nn.GroupNorm:
        out = GroupNorm(module.num_groups, module.num_channels, module.eps, module.affine)
        if module.affine:
            with torch.no_grad():
                out.weight = module.weight
                out.bias = module.bias
        out.training = module.training
    for name, child in module.named_children():
        new = convert_group_norm(child)
        if new is not child:
            out.add_module(name, new)
    return out
