"""Native instance norm: ft.InstanceNorm1d / 2d / 3d, ft.instance_norm, ft.convert_instance_norm.

The Deconver bundles build their networks with ``norm: nn.InstanceNorm3d`` / ``nn.InstanceNorm2d`` (deconver.py:50-66 norm1,
norm2; :129-138 Stem).  The classes here subclass the framework's, with the same constructor, defaults and ``state_dict`` keys;
on a device tensor of fp32 / bf16 whose statistics come from the input they run csrc/inorm.hip: float64 sums about the plane's
first element in a fixed order, one rounding per stored element, no atomics.  A framework ``nn.InstanceNorm*d`` given as
``norm=`` keeps running the framework's kernels; the native class is opted into by ``norm=ft.InstanceNorm3d`` or by
``ft.convert_instance_norm(model)``.

Everything outside the native gate runs ``F.instance_norm``: silently on the CPU (bit-identical to the framework), with one
``composed.warn_once`` naming the reason on a device (`fallback_reason`)."""
from __future__ import annotations

import torch
import torch.nn.functional as F
from torch import nn

from . import _native, composed

_NATIVE_DTYPES = (torch.float32, torch.bfloat16)


def fallback_reason(dtype, training: bool = True, track_running_stats: bool = False, param_dtypes=()):
    """why a DEVICE tensor of `dtype` does not take the native kernels in a module with these flags (None: it does);
    `param_dtypes`: the types of the weight / bias that are present.  (A plane of one element is no fallback: it raises the
    framework's ValueError whenever the statistics come from the input.)"""
    if dtype not in _NATIVE_DTYPES:
        return f"{str(dtype).replace('torch.', '')} input (the native kernels store float32 or bfloat16)"
    if track_running_stats:
        return "track_running_stats=True (the framework updates the running statistics)" if training else \
            "eval mode with running statistics"
    if any(d != torch.float32 for d in param_dtypes):
        return "weight / bias that are not float32"
    return None


def _planes(x):
    P = x.shape[0] * x.shape[1]
    return P, x.shape[1], (x.numel() // P if P else 0)


def _workspace(x, P, V):
    n = _native.lib().fz_inorm_workspace_bytes(P, V)
    if n < 0:
        raise _native.NativeError(f"fz_inorm_workspace_bytes({P}, {V}): shape out of range")
    return torch.empty(n // 8, dtype=torch.float64, device=x.device)


class InstanceNormFn(torch.autograd.Function):
    """y = (x − mean) rstd γ + β per plane of a contiguous channels-first device tensor.  Saves x, the float64 (mean, rstd) and γ;
    the parameter gradients are complete when backward returns (nothing is left in the deferred-finish queue)."""

    @staticmethod
    def forward(ctx, x, weight, bias, eps):
        x = x.contiguous()
        P, C, V = _planes(x)
        y = torch.empty_like(x)
        stats = torch.empty(P, 2, dtype=torch.float64, device=x.device)
        ws = _workspace(x, P, V)
        L = _native.lib()
        _native.check(L.fz_inorm_fwd(_native.ptr(x), _native.ptr(weight), _native.ptr(bias), _native.ptr(y), _native.ptr(stats),
                                     P, C, V, float(eps), _native.act_dtype(x), _native.ptr(ws), _native.stream_ptr(x)),
                      "fz_inorm_fwd")
        ctx.save_for_backward(x, stats, weight)
        ctx.has_bias = bias is not None
        return y

    @staticmethod
    def backward(ctx, gy):
        x, stats, weight = ctx.saved_tensors
        P, C, V = _planes(x)
        gy = gy.to(x.dtype).contiguous()
        need_x, need_w, need_b = ctx.needs_input_grad[:3]
        gx = torch.empty_like(x)
        gw = torch.empty(C, dtype=torch.float32, device=x.device) if weight is not None and need_w else None
        gb = torch.empty(C, dtype=torch.float32, device=x.device) if ctx.has_bias and need_b else None
        ws = _workspace(x, P, V)
        L = _native.lib()
        _native.check(L.fz_inorm_bwd(_native.ptr(x), _native.ptr(gy), _native.ptr(weight), _native.ptr(stats), _native.ptr(gx),
                                     _native.ptr(gw), _native.ptr(gb), P, C, V, _native.act_dtype(x), _native.ptr(ws),
                                     _native.stream_ptr(x)), "fz_inorm_bwd")
        return (gx if need_x else None), gw, gb, None


def launches(spatial: int, backward: bool = False, affine: bool = False) -> int:
    """native launches of one forward (or one backward) over planes of `spatial` elements"""
    n = 1 if spatial <= _native.lib().fz_inorm_one_pass_max() else 2
    return n + (1 if backward and affine else 0)


def _norm(x, running_mean, running_var, weight, bias, training, track_running_stats, momentum, eps):
    use_input_stats = training or not track_running_stats
    if x.is_cuda and x.dim() >= 3 and x.numel():
        if use_input_stats:
            F._verify_spatial_size(x.size())
        why = fallback_reason(x.dtype, training, track_running_stats, [p.dtype for p in (weight, bias) if p is not None])
        if why is None:
            return InstanceNormFn.apply(x, weight, bias, eps)
        composed.warn_once(f"instance_norm:{why}", f"instance norm with {why} is outside the native kernel set; using ATen on device")
    return F.instance_norm(x, running_mean, running_var, weight, bias, use_input_stats, momentum, eps)


def instance_norm(x, weight=None, bias=None, eps=1e-5):
    """F.instance_norm(x, weight=weight, bias=bias, eps=eps) with the statistics of the input: native on fp32 / bf16 device
    tensors (the output has the input's type; no autocast casting of its own), the framework's elsewhere."""
    return _norm(x, None, None, weight, bias, True, False, 0.0, eps)


class _Native:
    """`_apply_instance_norm` of nn.InstanceNorm{1,2,3}d on the native kernels; the rank check, the channel check and the
    unbatched-input handling stay the parent's forward."""

    def _apply_instance_norm(self, input):
        return _norm(input, self.running_mean, self.running_var, self.weight, self.bias, self.training,
                     self.track_running_stats, self.momentum if self.momentum is not None else 0.0, self.eps)


class InstanceNorm1d(_Native, nn.InstanceNorm1d):
    pass


class InstanceNorm2d(_Native, nn.InstanceNorm2d):
    pass


class InstanceNorm3d(_Native, nn.InstanceNorm3d):
    pass


_NATIVE_OF = {nn.InstanceNorm1d: InstanceNorm1d, nn.InstanceNorm2d: InstanceNorm2d, nn.InstanceNorm3d: InstanceNorm3d}


def convert_instance_norm(module: nn.Module) -> nn.Module:
    """`module` with every nn.InstanceNorm{1,2,3}d in it replaced by the native class (in the manner of
    nn.SyncBatchNorm.convert_sync_batchnorm): parameters, buffers, eps, momentum, the flags and `training` are kept, the
    state_dict keys do not change, everything else is left alone.  Idempotent."""
    out = module
    cls = _NATIVE_OF.get(type(module))
    if cls is not None:
        out = cls(module.num_features, module.eps, module.momentum, module.affine, module.track_running_stats)
        if module.affine:
            with torch.no_grad():
                out.weight = module.weight
                out.bias = module.bias
        if module.track_running_stats:
            out.running_mean = module.running_mean
            out.running_var = module.running_var
            out.num_batches_tracked = module.num_batches_tracked
        out.training = module.training
    for name, child in module.named_children():
        new = convert_instance_norm(child)
        if new is not child:
            out.add_module(name, new)
    return out
