"""Host side of the bf16 storage mode of the Deconver family: the composed fallback of `ft.Deconv` on bfloat16 CPU tensors
(fp32 arithmetic, rounded where the device stores) against the independent restatement tests/deconv_bf16_ref.py, the
unchanged float32 CPU path, and the argument checks of the new entry points (no device needed)."""
import ctypes

import pytest
import torch

import deconv_bf16_ref as R
import factorizer_amd as ft

BF = torch.bfloat16

CONFIGS = {
    "recipe_dw_k3": dict(channels=8, groups=-1, ratio=1, kernel_size=(3, 3, 3), num_iters=1),
    "g2_r2_grad1": dict(channels=8, groups=2, ratio=2, kernel_size=(3, 3, 3), num_iters=2, num_grad_iters=1),
    "2d_filter_update": dict(channels=6, groups=3, ratio=1, kernel_size=(3, 3), num_iters=2, update_filter=True),
}


def _layer(cfg, seed=0):
    torch.manual_seed(seed)
    m = ft.Deconv(**cfg)
    with torch.no_grad():
        m.init.linear.linear.bias.add_(0.5)      # most sources start positive
    return m


def _ref(m, x, store):
    lin = m.init.linear.linear
    return R.deconv_forward(x, lin.weight, lin.bias, m.init.h0, m.groups, m.kernel_size, m.num_iters, m.num_grad_iters,
                            m.eps, m.update_filter, store)


@pytest.mark.parametrize("tag", sorted(CONFIGS))
def test_bf16_composed_fallback_equals_the_restatement(tag):
    """bfloat16 CPU input: same values as the restatement with the device's storage roundings (both are fp32 ATen between
    the roundings: bit for bit), bfloat16 out, fp32 parameter gradients equal to autograd through the restatement."""
    m = _layer(CONFIGS[tag])
    nd = len(m.kernel_size)
    torch.manual_seed(1)
    x = R.rb(torch.rand(2, m.channels, *((5, 6, 7)[:nd])))
    xb = x.to(BF).requires_grad_(True)
    y = m(xb)
    assert y.dtype == BF and y.shape[1] == m.groups * m.source_channels
    xr = x.clone().requires_grad_(True)
    yr = _ref(m, xr, R.store_bf16)
    assert torch.equal(y.float(), yr.detach())
    assert float(yr.detach().max()) > 0
    gy = R.rb(torch.rand_like(yr))
    params = [m.init.h0, m.init.linear.linear.weight]
    got = torch.autograd.grad(y, [xb] + params, gy.to(BF), allow_unused=True)
    ref = torch.autograd.grad(yr, [xr] + params, gy, allow_unused=True)
    assert got[0].dtype == BF and got[1].dtype == torch.float32
    for k, a, b in zip(("x", "h0", "linear.weight"), got, ref):
        if b is None:        # the sources' start reaches the result only through iterations that carry no gradient
            assert a is None and m.num_grad_iters < m.num_iters, k
            continue
        assert k == "x" or a.dtype == torch.float32
        # the composed path rounds the gradients that cross a bf16 tensor (x, s0, num, r, s per iteration) once each
        n = 2 + 3 * m.num_grad_iters
        err, scale = (a.float() - b).abs().max().item(), b.abs().max().item()
        assert err <= n * R.U * scale + 1e-6, (k, err, scale)


def test_bf16_restatement_is_close_to_plain_fp32():
    """the roundings move the layer's output by a few u at most (non-negative operands: no cancellation)"""
    m = _layer(CONFIGS["g2_r2_grad1"])
    torch.manual_seed(2)
    x = R.rb(torch.rand(2, 8, 5, 6, 7))
    with torch.no_grad():
        a, b = _ref(m, x, R.store_bf16), _ref(m, x, R.store_none)
        assert (a - b).abs().max() <= 6 * R.U * b.abs().max()       # s0, num, and r, s of two iterations
        assert torch.allclose(m(x), b, rtol=1e-5, atol=1e-6)         # the float32 module is the plain restatement


@pytest.mark.parametrize("tag", sorted(CONFIGS))
def test_fp32_cpu_path_is_unchanged(tag):
    """float32 CPU tensors take the expressions they always took: bit-identical to the composed statement written out here
    with the module's own framework helpers (`_gcorr`, `_lag_corr`: not touched by the storage mode)."""
    from factorizer_amd.deconver import _adjoint_filters, _gcorr, _lag_corr
    m = _layer(CONFIGS[tag])
    nd = len(m.kernel_size)
    torch.manual_seed(3)
    x = torch.rand(2, m.channels, *((5, 6, 7)[:nd]))
    with torch.no_grad():
        y = m(x)
        s, h = m.init(x)
        if not m.update_filter:
            h = h[:1]
        for _ in range(m.num_iters):
            hg = m._filters(h)
            num = _gcorr(x, _adjoint_filters(hg), m.padding) + m.eps
            s = s * num / (_gcorr(_gcorr(s, hg, m.padding), _adjoint_filters(hg), m.padding) + m.eps)
            if m.update_filter:
                num_h = _lag_corr(s, x, m.groups, m.padding) + m.eps
                den_h = _lag_corr(s, _gcorr(s, hg, m.padding), m.groups, m.padding) + m.eps
                h = h * (num_h / den_h).reshape(x.shape[0], m.channels, m.source_channels, *m.kernel_size)
    assert y.dtype == torch.float32 and torch.equal(y, s)


def test_float16_is_refused_by_the_binding():
    from factorizer_amd import _native
    with pytest.raises(TypeError):
        _native.act_dtype(torch.zeros(1, dtype=torch.float16))


def test_new_entry_points_check_their_arguments():
    """fz_gcorr_act / fz_gcorr_wgrad_act / fz_gcorr_mu_bwd validate before anything touches the device"""
    from factorizer_amd import _native
    from factorizer_amd import build
    build.build(verbose=False)
    lib = _native.lib()
    p = ctypes.c_void_p(8)      # a non-null pointer value the host code never dereferences
    F32, B16 = _native.STORE_F32, _native.STORE_BF16
    shape = (1, 2, 1, 1, 4, 4, 8, 3, 3, 3, 0)     # B, G, Ci, Co, D, H, W, kd, kh, kw, w_batched
    err = lib.fz_last_error_string
    for dt in (F32, B16):
        assert lib.fz_gcorr_act(None, p, p, None, None, *shape, 0.0, dt, None) == -4 and b"null" in err()
        assert lib.fz_gcorr_act(p, p, p, p, None, *shape, 0.0, dt, None) == -4            # mul_a without mul_b
        assert lib.fz_gcorr_wgrad_act(p, None, p, p, *shape, dt, None) == -4 and b"null" in err()
        assert lib.fz_gcorr_mu_bwd(p, p, p, p, None, p, p, p, *shape, 1e-16, dt, None) == -4 and b"null" in err()
        assert lib.fz_gcorr_mu_bwd(p, p, p, p, p, None, None, None, *shape, 1e-16, dt, None) == -4   # no output at all
    even = (1, 2, 1, 1, 4, 4, 8, 3, 4, 3, 0)
    assert lib.fz_gcorr_act(p, p, p, None, None, *even, 0.0, B16, None) == -2 and b"odd" in err()
    assert lib.fz_gcorr_mu_bwd(p, p, p, p, p, p, None, None, *even, 1e-16, B16, None) == -2
    bad = (1, 0, 1, 1, 4, 4, 8, 3, 3, 3, 0)
    assert lib.fz_gcorr_act(p, p, p, None, None, *bad, 0.0, F32, None) == -1
    assert lib.fz_gcorr_wgrad_act(p, p, p, p, *bad, F32, None) == -1
    for dt in (2, 7, -1):
        assert lib.fz_gcorr_act(p, p, p, None, None, *shape, 0.0, dt, None) == -2 and b"act_dtype" in err()
        assert lib.fz_gcorr_wgrad_act(p, p, p, p, *shape, dt, None) == -2 and b"act_dtype" in err()
        assert lib.fz_gcorr_mu_bwd(p, p, p, p, p, p, p, p, *shape, 1e-16, dt, None) == -2 and b"act_dtype" in err()
    # an empty batch is no work, whatever the type
    empty = (0,) + shape[1:]
    assert lib.fz_gcorr_act(p, p, p, None, None, *empty, 0.0, B16, None) == 0
    # the fp32 entry points are the new ones with FZ_STORE_F32: same checks, same messages
    assert lib.fz_gcorr(None, p, p, None, None, *shape, 0.0, None) == -4 and b"fz_gcorr: null pointer" in err()
    assert lib.fz_gcorr_wgrad(p, p, None, p, *shape, None) == -4 and b"fz_gcorr_wgrad: null pointer" in err()
