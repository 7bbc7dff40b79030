"""Independent restatement of the grouped correlations and of the blind-deconvolution layer (deconvolution.py:60-166) with
the bf16 STORAGE roundings of the device path inserted — framework ops on CPU tensors only; this file shares no code with
factorizer_amd.  Shared by tests/test_deconv_bf16_cpu.py and tests/test_gpu_deconv_bf16.py.

Storage contract restated here: a tensor that the device keeps in HBM as bf16 is rounded to nearest-even ONCE, when it is
stored; everything between two stores is fp32 (or whatever type the caller computes in: the float64 checks pass doubles).
Stored by `Deconv` on a bf16 input: s0 = relu(linear(x)), num = Hᵀx + ε, r = H s, s' = s ∘ num / (Hᵀr + ε).  Never rounded:
the filters h, the lag correlations and the ratio of the filter update, any parameter gradient.  In the backward the rounding is
a straight-through op (its gradient is the identity): the additional roundings of stored GRADIENTS are not restated — the tests
count them in their bounds."""
from __future__ import annotations

import contextlib
import itertools

import torch
import torch.nn.functional as F

BF = torch.bfloat16
U = 2.0 ** -8     # bf16 unit roundoff: 8 significand bits, round to nearest even

_CONV = {2: F.conv2d, 3: F.conv3d}


def rb(t):
    """the value a bf16 tensor in memory holds, in the type of t"""
    return t.to(BF).to(t.dtype)


class _StoreBf16(torch.autograd.Function):
    @staticmethod
    def forward(ctx, t):
        return rb(t)

    @staticmethod
    def backward(ctx, g):
        return g


def store_bf16(t):
    """round to bf16 as a straight-through op"""
    return _StoreBf16.apply(t)


def store_none(t):
    return t


def corr(inp, w):
    """out[b, g·Co + o] = Σ_i inp[b, g·Ci + i] ⋆ w[b or 0, g, o, i]  ("same" zero padding, odd extents).
    inp (B, G·Ci, *S); w (Bw, G, Co, Ci, *k), Bw ∈ {1, B}."""
    B = inp.shape[0]
    Bw, G, Co, Ci = w.shape[:4]
    ks = tuple(w.shape[4:])
    conv, pad = _CONV[len(ks)], tuple(k // 2 for k in ks)
    if Bw == 1:
        return conv(inp, w.reshape(G * Co, Ci, *ks), padding=pad, groups=G)
    out = conv(inp.reshape(1, B * G * Ci, *inp.shape[2:]), w.reshape(B * G * Co, Ci, *ks), padding=pad, groups=B * G)
    return out.reshape(B, G * Co, *inp.shape[2:])


def adjoint(w):
    """filters of the adjoint operator: channels transposed, every spatial axis reversed"""
    return torch.flip(w.transpose(2, 3), dims=tuple(range(4, w.ndim)))


def lag_corr(s, x, G, ks):
    """L[b, g, c, k, τ] = Σ_v x[b, g·C + c, v] · s[b, g·K + k, v + τ − p], one shifted product sum per lag τ"""
    B = s.shape[0]
    K, C = s.shape[1] // G, x.shape[1] // G
    sp = tuple(s.shape[2:])
    pad = [k // 2 for k in ks]
    spad = F.pad(s, [p for q in reversed(pad) for p in (q, q)]).reshape(B, G, 1, K, *[n + 2 * p for n, p in zip(sp, pad)])
    xg = x.reshape(B, G, C, 1, *sp)
    L = torch.zeros(B, G, C, K, *ks, dtype=s.dtype)
    red = tuple(range(4, 4 + len(sp)))
    for tau in itertools.product(*[range(k) for k in ks]):
        win = spad[(Ellipsis, *[slice(t, t + n) for t, n in zip(tau, sp)])]
        L[(Ellipsis, *tau)] = (xg * win).sum(red)
    return L


def mu_update(s, num, r, wT, eps):
    """s ∘ num / (corr(r, wT) + ε), unrounded"""
    return s * num / (corr(r, wT) + eps)


def deconv_forward(x, lin_w, lin_b, h0, groups, ksize, num_iters, num_grad_iters=None, eps=1e-16, update_filter=False,
                   store=store_bf16):
    """sources after num_iters multiplicative updates (deconvolution.py:136-166; `store` marks what the device keeps in memory).
    x (B, C, *S); lin_w (G·K, C, 1), lin_b (G·K); h0 (C, K, *k)."""
    B, C = x.shape[:2]
    K = h0.shape[1]
    num_grad_iters = num_iters if num_grad_iters is None else num_grad_iters
    lin = F.conv1d(x.flatten(2), lin_w, lin_b).reshape(B, lin_w.shape[0], *x.shape[2:])
    s = torch.relu(store(lin))
    h = torch.relu(h0).reshape(1, groups, C // groups, K, *ksize)
    if update_filter:
        h = h.expand(B, *h.shape[1:])
    for it in range(1, num_iters + 1):
        ctx = torch.no_grad() if it < num_iters - num_grad_iters + 1 else contextlib.nullcontext()
        with ctx:
            num = store(corr(x, adjoint(h)) + eps)
            r = store(corr(s, h))
            s = store(mu_update(s, num, r, adjoint(h), eps))
            if update_filter:
                num_h = lag_corr(s, x, groups, ksize) + eps
                den_h = lag_corr(s, store(corr(s, h)), groups, ksize) + eps
                h = h * (num_h / den_h)
    return s
