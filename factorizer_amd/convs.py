"""Conv3d / ConvTranspose3d (and Conv2d / ConvTranspose2d) parameter containers whose forward runs
the native GEMM-family kernels for the shapes the Factorizer U-shape uses (unet.py:53,123,231,253):
kernel 2 / stride 2 (space-to-depth GEMM), transposed kernel 2 / stride 2 (GEMM +
depth-to-space), kernel 3 / padding 1 (stem) and kernel 1 (head).  They subclass the torch
modules, so initialisation and state_dict keys are those of the reference's nn.Conv3d / nn.Conv2d."""
from __future__ import annotations

import torch
from torch import nn

from . import composed
from . import pointwise as PW


def _all(v, n):
    return tuple(v) == (n,) * len(v)


def _gate(m, x, nd) -> bool:
    """what every native convolution needs of its module and input (rank nd)"""
    return (x.is_cuda and x.numel() and x.dtype in (torch.float32, torch.bfloat16) and m.weight.dtype == torch.float32
            and x.dim() == nd + 2 and m.groups == 1 and _all(m.dilation, 1))


class _Conv:
    """forward of Conv2d / Conv3d (`_nd` = 2 / 3): k2s2 down-sampling on the space-to-depth loader, the k3p1 stem on the tap
    loader (3-D: the stem kernel), the k1 head on the plain GEMM."""

    _warn_dtype = False

    def _gate(self, x) -> bool:
        return _gate(self, x, self._nd) and self.padding_mode == "zeros"

    def _k2s2_native(self, x) -> bool:
        return (self._gate(x) and _all(self.kernel_size, 2) and _all(self.stride, 2) and _all(self.padding, 0)
                and all(s % 2 == 0 for s in x.shape[2:]) and x.shape[-1] % 4 == 0
                and (PW._vox(x) // 2 ** self._nd) % 4 == 0 and self.in_channels % 2 == 0)

    def forward_fork(self, x):
        """``(x, self(x))`` for an ``x`` that is also kept as a skip connection: on the native path both
        come out of one autograd node whose backward adds the skip gradient inside the input-gradient
        kernel (PW.SkipConvK2S2Fn) instead of leaving the sum to a separate accumulation pass."""
        if self._k2s2_native(x) and x.requires_grad and torch.is_grad_enabled():
            return PW.SkipConvK2S2Fn.apply(x, self.weight, self.bias)
        return x, self(x)

    def forward(self, x):
        nd = self._nd
        if self._gate(x):
            C = self.in_channels
            k3 = _all(self.kernel_size, 3) and _all(self.stride, 1) and _all(self.padding, 1) and x.shape[-1] % 4 == 0
            if k3 and C % 2:
                # odd C_in (1- or 3-modality stems: ISLES / BraTS variants, RGB): the kernels consume channel
                # pairs, so run them on one extra all-zero channel (input 1/C larger, weights padded to match)
                pad = (0, 0) * nd + (0, 1)
                return PW.ConvK3Fn.apply(torch.nn.functional.pad(x, pad), torch.nn.functional.pad(self.weight, pad), self.bias)
            if self._k2s2_native(x):
                return PW.ConvK2S2Fn.apply(x, self.weight, self.bias)
            if k3:
                return PW.ConvK3Fn.apply(x, self.weight, self.bias)
            if _all(self.kernel_size, 1) and _all(self.stride, 1) and _all(self.padding, 0) and C % 2 == 0 \
                    and PW._vox(x) % 4 == 0:
                return PW.LinearFn.apply(x, self.weight.reshape(self.out_channels, C, 1), self.bias)
            composed.warn_once(f"conv{nd}d{self.kernel_size}{self.stride}{tuple(x.shape[2:])}",
                               f"Conv{nd}d kernel={self.kernel_size} stride={self.stride} on {tuple(x.shape)} is "
                               "outside the native kernel set; using ATen on device")
        elif self._warn_dtype and x.is_cuda and x.numel():
            composed.warn_once(f"conv{nd}d{self.kernel_size}{self.stride}{tuple(x.shape[2:])}{x.dtype}",
                               f"Conv{nd}d kernel={self.kernel_size} stride={self.stride} on {tuple(x.shape)} ({x.dtype}) is "
                               "outside the native kernel set; using ATen on device")
        return super().forward(x)


class _ConvTranspose:
    """forward of ConvTranspose2d / ConvTranspose3d (`_nd` = 2 / 3): kernel 2 / stride 2 as GEMM + depth-to-space."""

    _even_width = False

    def native_ok(self, x, output_size=None):
        return bool(_gate(self, x, self._nd) and output_size is None
                    and _all(self.kernel_size, 2) and _all(self.stride, 2)
                    and _all(self.padding, 0) and _all(self.output_padding, 0) and self.in_channels % 2 == 0
                    and PW._vox(x) % 4 == 0 and not (self._even_width and x.shape[-1] % 2))

    def forward(self, x, output_size=None):
        if self.native_ok(x, output_size):
            return PW.TConvK2S2Fn.apply(x, self.weight, self.bias)
        if x.is_cuda and x.numel():
            nd = self._nd
            composed.warn_once(f"tconv{nd}d{self.kernel_size}{self.stride}{tuple(x.shape[2:])}",
                               f"ConvTranspose{nd}d kernel={self.kernel_size} stride={self.stride} on "
                               f"{tuple(x.shape)} is outside the native kernel set; using ATen on device")
        return super().forward(x, output_size)


class Conv3d(_Conv, nn.Conv3d):
    _nd = 3


class ConvTranspose3d(_ConvTranspose, nn.ConvTranspose3d):
    _nd = 3


class Conv2d(_Conv, nn.Conv2d):
    """Conv3d's container for a 2-D U-shape (factorizer.py:147,159 / deconver.py with spatial_dims=2)."""
    _nd = 2
    _warn_dtype = True   # kept as found: only the 2-D module also warns of a device tensor that fails the base gate (dtype, rank, groups)


class ConvTranspose2d(_ConvTranspose, nn.ConvTranspose2d):
    _nd = 2
    # kept as found: only the 2-D gate asks for an even width (the backward's s2d loaders take an even Wo).  The 3-D backward
    # hands Wo = W to the same kind of loader, so a 3-D odd width with voxels % 4 == 0 looks refused there, not here: a follow-up.
    _even_width = True
