"""The reference's CNN blocks — ``DoubleConv`` (the default block of ``UNet``), ``BasicBlock``, ``PreActivationBlock``, ``SepConv``
(factorizer/layers/conv.py:12-283) — on the package's native layers.

Same constructor arguments, sub-module names (``block1.0`` / ``block1.2`` / ``block2.0`` / ``block2.2``; ``conv1``, ``norm1``, ...,
``shortcut``; ``pwconv1.linear``, ``dwconv``, ``pwconv2.linear``) and parameter-creation order, so seeds and checkpoints line up.
The defaults are the reference's in the package's classes: ``ft.Conv3d`` (kernel 3, padding 1), ``ft.GroupNorm(8, C)``,
``nn.LeakyReLU``, ``nn.Dropout(p=0)``.

A norm directly followed by its activation runs as ONE ``ft.group_norm(..., act=...)`` call (`norm_act`) when the norm is exactly
``ft.GroupNorm``, the activation exactly ``nn.ReLU`` or ``nn.LeakyReLU`` and neither carries hooks (nor does the process carry global module hooks); otherwise
the two modules are called one after the other.  ``BasicBlock``'s tail (norm2, + shortcut, act) is the native norm without
activation, then the framework's add and activation; ``SepConv``'s depthwise convolution is the framework's."""
from __future__ import annotations

import math

from torch import nn

from . import convs
from .group_norm import GroupNorm
from .layers import Linear
from .utils import as_tuple, partialize


def _hooked(m):
    """does anything hang on a call of `m`: its own hooks, or the process-wide module hooks (the fused path calls no module)"""
    G = nn.modules.module
    return bool(m._forward_hooks or m._forward_pre_hooks or m._backward_hooks or m._backward_pre_hooks
                or G._global_forward_hooks or G._global_forward_pre_hooks or G._global_backward_hooks
                or G._global_backward_pre_hooks)


def fused_act(norm, act):
    """(act name, negative_slope) when `norm` followed by `act` can run as one ft.group_norm call, else None"""
    if type(norm) is not GroupNorm or _hooked(norm) or _hooked(act):
        return None
    if type(act) is nn.ReLU:
        return "relu", 0.0
    if type(act) is nn.LeakyReLU:
        return "leaky_relu", act.negative_slope
    return None


def norm_act(norm, act, x):
    """act(norm(x)), fused where `fused_act` allows"""
    f = fused_act(norm, act)
    if f is None:
        return act(norm(x))
    return norm.forward_act(x, *f)


_CONV = (convs.Conv3d, {"kernel_size": 3, "padding": 1})
_NORM = (GroupNorm, (8,))
_DROP = (nn.Dropout, {"p": 0.0})


class _ConvDropNormAct(nn.Sequential):
    """conv -- drop -- norm -- act with the last two fused; indices 0 .. 3 as in the reference's nn.Sequential"""

    def forward(self, x):
        if len(self) != 4:
            return super().forward(x)
        return norm_act(self[2], self[3], self[1](self[0](x)))


class DoubleConv(nn.Module):
    """(Conv -- Drop -- Norm -- Act) ** 2."""

    def __init__(self, in_channels, out_channels, mid_channels=None, conv=_CONV, norm=_NORM, act=nn.LeakyReLU, drop=_DROP,
                 stride=1, **kwargs):
        super().__init__()
        mid_channels = out_channels if mid_channels is None else mid_channels
        conv, drop, norm, act = partialize(conv), partialize(drop), partialize(norm), partialize(act)
        self.block1 = _ConvDropNormAct(conv(in_channels, mid_channels, stride=stride), drop(), norm(mid_channels), act())
        self.block2 = _ConvDropNormAct(conv(mid_channels, out_channels, stride=1), drop(), norm(out_channels), act())

    def forward(self, x):
        return self.block2(self.block1(x))


def _shortcut(conv1, in_channels, out_channels, stride):
    return conv1.__class__(in_channels, out_channels, kernel_size=1, stride=stride, bias=False)


class BasicBlock(nn.Module):
    """Basic ResNet block."""

    def __init__(self, in_channels, out_channels, mid_channels=None, conv=_CONV, norm=_NORM, act=nn.LeakyReLU, drop=_DROP,
                 stride=1, **kwargs):
        super().__init__()
        mid_channels = out_channels if mid_channels is None else mid_channels
        conv, drop, norm, act = partialize(conv), partialize(drop), partialize(norm), partialize(act)
        self.conv1 = conv(in_channels, mid_channels, stride=stride)
        self.drop1 = drop()
        self.norm1 = norm(mid_channels)
        self.conv2 = conv(mid_channels, out_channels)
        self.drop2 = drop()
        self.norm2 = norm(out_channels)
        self.act = act()
        if math.prod(as_tuple(stride)) != 1 or in_channels != out_channels:
            self.shortcut = _shortcut(self.conv1, in_channels, out_channels, stride)
        else:
            self.shortcut = nn.Identity()

    def forward(self, x):
        shortcut = self.shortcut(x)
        out = norm_act(self.norm1, self.act, self.drop1(self.conv1(x)))
        out = self.norm2(self.drop2(self.conv2(out)))
        return self.act(out + shortcut)


class PreActivationBlock(nn.Module):
    """Pre-activation version of BasicBlock."""

    def __init__(self, in_channels, out_channels, mid_channels=None, conv=_CONV, norm=_NORM, act=nn.LeakyReLU, drop=_DROP,
                 stride=1, **kwargs):
        super().__init__()
        mid_channels = out_channels if mid_channels is None else mid_channels
        conv, drop, norm, act = partialize(conv), partialize(drop), partialize(norm), partialize(act)
        self.norm1 = norm(in_channels)
        self.act = act()
        self.conv1 = conv(in_channels, mid_channels, stride=stride)
        self.drop1 = drop()
        self.norm2 = norm(mid_channels)
        self.conv2 = conv(mid_channels, out_channels)
        self.drop2 = drop()
        if math.prod(as_tuple(stride)) != 1 or in_channels != out_channels:
            self.shortcut = _shortcut(self.conv1, in_channels, out_channels, stride)

    def forward(self, x):
        out = norm_act(self.norm1, self.act, x)
        shortcut = self.shortcut(out) if hasattr(self, "shortcut") else x
        out = self.drop1(self.conv1(out))
        out = norm_act(self.norm2, self.act, out)
        out = self.drop2(self.conv2(out))
        return out + shortcut


class SepConv(nn.Module):
    """Inverted separable convolution from MobileNetV2 (https://arxiv.org/abs/1801.04381): channels-first Linear, activation,
    depthwise convolution (the framework's: groups != 1 is outside ft.Conv3d's native gate), Linear."""

    def __init__(self, in_channels, out_channels=None, hidden_channels=None, ratio=2, spatial_dims=3, act=nn.GELU, kernel_size=5,
                 stride=1, padding=2, dilation=1, bias=True, padding_mode="zeros", device=None, dtype=None, **kwargs):
        super().__init__()
        out_channels = in_channels if out_channels is None else out_channels
        hidden_channels = int(ratio * in_channels) if hidden_channels is None else hidden_channels
        conv = getattr(nn, f"Conv{spatial_dims}d")
        self.pwconv1 = Linear(in_channels, hidden_channels, bias=False)
        self.act = partialize(act)()
        self.dwconv = conv(hidden_channels, hidden_channels, kernel_size=kernel_size, groups=hidden_channels, stride=stride,
                           padding=padding, dilation=dilation, bias=bias, padding_mode=padding_mode, device=device, dtype=dtype)
        self.pwconv2 = Linear(hidden_channels, out_channels)

    def forward(self, x):
        return self.pwconv2(self.dwconv(self.act(self.pwconv1(x))))
