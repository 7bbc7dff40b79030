"""Sliding-window inference on 1-D and 2-D images (composed CPU path) against the 3-D oracle of oracle/cpu_ref.py, lifted:
unit axes are put in front of the spatial ones, the roi is 1 along them and the predictor squeezes them away again.  A unit axis
has one window and a Gaussian factor of exactly 1, so the lifted oracle IS the 1-D / 2-D algorithm.  Also the FIVES window grid
and the host-side argument checks of the fz_sw_*2 entry points (no device call)."""
import ctypes
import warnings

import pytest
import torch
import torch.nn.functional as F

import factorizer_amd as ft
from factorizer_amd import inference as I
from oracle import cpu_ref as O


def lifted_oracle(x, roi, sw_batch, net, overlap=0.5, mode="gaussian"):
    """oracle/cpu_ref.py:sliding_window_oracle (3-D) on a 1-D or 2-D image"""
    k = 5 - x.dim()
    x3 = x.reshape(*x.shape[:2], *(1,) * k, *x.shape[2:])

    def net3(w):
        y = net(w.reshape(*w.shape[:2], *w.shape[2 + k:]))
        return y.reshape(*y.shape[:2], *(1,) * k, *y.shape[2:])

    y = O.sliding_window_oracle(x3, (1,) * k + tuple(roi), sw_batch, net3, overlap=overlap, mode=mode)
    return y.reshape(*y.shape[:2], *y.shape[2 + k:])


def toy_net(nd, cin=2, cout=3, seed=0):
    g = torch.Generator().manual_seed(seed)
    w = torch.randn(cout, cin, *(3,) * nd, generator=g) * 0.2
    conv = (F.conv1d, F.conv2d)[nd - 1]
    return lambda x: torch.tanh(conv(x, w.to(x.device, x.dtype), torch.full((cout,), 0.1, device=x.device, dtype=x.dtype),
                                      padding=1))


@pytest.mark.parametrize("size,roi,ov,mode", [((37, 50), (16, 24), 0.5, "gaussian"),     # last windows at (21, 26)
                                              ((37, 50), (16, 24), 0.5, "constant"),
                                              ((24, 40), (24, 16), 0.25, "gaussian"),    # one window along y
                                              ((100,), (32,), 0.25, "gaussian"),
                                              ((101,), (30,), 0.5, "constant")])
def test_composed_matches_lifted_oracle(size, roi, ov, mode):
    torch.manual_seed(0)
    net = toy_net(len(size))
    x = torch.randn(2, 2, *size)
    with torch.no_grad(), warnings.catch_warnings():
        warnings.simplefilter("error", RuntimeWarning)     # CPU tensors are the composed path's own domain: no warning
        y = ft.sliding_window_inference(x, roi, 3, net, overlap=ov, mode=mode)
        yo = lifted_oracle(x, roi, 3, net, overlap=ov, mode=mode)
    assert y.shape == (2, 3, *size) and y.dtype == torch.float32
    assert torch.allclose(y, yo, rtol=1e-5, atol=1e-6)


def test_2d_grid_pulls_the_last_window_back():
    st = I.window_starts((37, 50), (16, 24), I.scan_interval((37, 50), (16, 24), (0.5, 0.5)))
    assert [s[0] for s in st[::4]] == [0, 8, 16, 21] and [s[1] for s in st[:4]] == [0, 12, 24, 26]


def test_per_axis_overlap_and_sigma():
    """overlap and sigma_scale as per-axis tuples, against a dense restatement with the per-axis grid spelled out"""
    torch.manual_seed(1)
    net = toy_net(2)
    x = torch.randn(1, 2, 30, 45)
    roi, ov, sig = (16, 20), (0.5, 0.25), (0.125, 0.25)
    with torch.no_grad():
        y = ft.sliding_window_inference(x, roi, 2, net, overlap=ov, mode="gaussian", sigma_scale=sig)
        ys = [0, 8, 14]                     # interval 8, last window pulled back to 30 - 16
        xs = [0, 15, 25]                    # interval 15, last window pulled back to 45 - 20
        g = []
        for r, s in zip(roi, sig):
            t = torch.arange(r, dtype=torch.float64) - (r - 1) / 2.0
            g.append(torch.exp(-(t ** 2) / (2 * (s * r) ** 2)).float().double())
        w = (g[0][:, None] * g[1][None, :]).float()
        w = w.clamp_min(max(float(w.min()), 1e-3))
        out, cnt = torch.zeros(1, 3, 30, 45), torch.zeros(30, 45)
        for y0 in ys:
            for x0 in xs:
                out[0, :, y0:y0 + 16, x0:x0 + 20] += w * net(x[:, :, y0:y0 + 16, x0:x0 + 20])[0]
                cnt[y0:y0 + 16, x0:x0 + 20] += w
    assert torch.allclose(y, out / cnt, rtol=1e-5, atol=1e-6)


def test_2d_image_smaller_than_the_roi_is_padded_and_cropped():
    """10 x 40 under a 16 x 16 roi: 3 + 3 rows of padding, windows along x only, the padding cropped off again"""
    torch.manual_seed(2)
    net = toy_net(2)
    x = torch.randn(1, 2, 10, 40)
    with torch.no_grad():
        y = ft.SlidingWindowInfererAdapt(roi_size=(16, 16), sw_batch_size=2, overlap=0.5, mode="gaussian")(x, net)
        yo = lifted_oracle(F.pad(x, (0, 0, 3, 3)), (16, 16), 2, net)[:, :, 3:13]
    assert y.shape == (1, 3, 10, 40)
    assert torch.allclose(y, yo, rtol=1e-5, atol=1e-6)
    # roi entries None / <= 0 take the image extent: one window, the weights cancel
    with torch.no_grad():
        z = ft.sliding_window_inference(x, (None, -1), 1, net, mode="gaussian")
    assert torch.allclose(z, net(x), rtol=1e-5, atol=1e-6)


def test_fives_and_odd_width_grids():
    """FIVES inference (inference.yaml:27,77-83): 2048^2 under roi 512^2, overlap 0.5 -> 7 x 7 windows; 1000 x 1298 -> 3 x 5
    windows with the last one pulled back to x0 = 786 (a width, origin and image width that are not multiples of 4)"""
    st = I.window_starts((2048, 2048), (512, 512), I.scan_interval((2048, 2048), (512, 512), (0.5, 0.5)))
    assert len(st) == 49 and st[0] == (0, 0) and st[-1] == (1536, 1536)
    st = I.window_starts((1000, 1298), (512, 512), I.scan_interval((1000, 1298), (512, 512), (0.5, 0.5)))
    assert len(st) == 15 and st[-1] == (488, 786) and [s[1] for s in st[:5]] == [0, 256, 512, 768, 786]


def test_rank_is_checked():
    with pytest.raises(ValueError, match="spatial axes"):
        ft.sliding_window_inference(torch.zeros(1, 1, 4, 4, 4, 4), 4, 1, lambda w: w)


@pytest.fixture(scope="module")
def lib():
    from factorizer_amd import build, _native
    build.build(verbose=False)
    return _native.lib()


def test_nd_entry_points_are_declared_and_exported(lib):
    from factorizer_amd import _native
    new = {"fz_sw_gather2", "fz_sw_accumulate2", "fz_sw_finalize2"}
    assert new <= set(_native.declared_symbols())
    for n in new:
        assert hasattr(lib, n)


def test_nd_entry_points_check_arguments_on_the_host(lib):
    """Every call below is refused before anything touches the device (none of them may pass: the pointers are fake)."""
    from factorizer_amd import _native
    p, F32, BF16 = ctypes.c_void_p(64), _native.STORE_F32, _native.STORE_BF16
    # gather: (C, D, H, W) = (3, 1, 20, 30), window (1, 8, 8)
    assert lib.fz_sw_gather2(None, p, 3, 1, 20, 30, 1, 8, 8, 0, 0, 0, F32, None) == -4
    assert lib.fz_sw_gather2(p, p, 3, 1, 20, 30, 1, 8, 8, 0, 0, 0, 7, None) == -4
    assert b"act_dtype" in lib.fz_last_error_string()
    assert lib.fz_sw_gather2(p, p, 3, 1, 20, 30, 1, 8, 8, 0, 13, 0, BF16, None) == -1          # y0 + rh > H
    assert b"outside" in lib.fz_last_error_string()
    assert lib.fz_sw_gather2(p, p, 3, 1, 20, 30, 1, 8, 7, 0, 0, 24, F32, None) == -1           # x0 + rw > W
    assert lib.fz_sw_gather2(p, p, 0, 1, 20, 30, 1, 8, 8, 0, 0, 0, F32, None) == -1
    # accumulate
    assert lib.fz_sw_accumulate2(p, p, p, None, p, p, 1e-3, 3, 1, 1, 101, 1, 1, 30, 0, 0, 71, F32, None) == -4
    assert lib.fz_sw_accumulate2(p, p, p, p, p, p, 1e-3, 3, 1, 1, 101, 1, 1, 30, 0, 0, 71, -1, None) == -4
    assert lib.fz_sw_accumulate2(p, p, p, p, p, p, 1e-3, 3, 1, 1, 101, 1, 1, 30, 0, 0, 72, BF16, None) == -1
    assert lib.fz_sw_accumulate2(p, p, p, p, p, p, 1e-3, 3, 1, 1, 101, 1, 1, 30, 0, -1, 0, F32, None) == -1
    # finalize: a bf16 result needs a tensor of its own
    assert lib.fz_sw_finalize2(p, p, None, 3, 100, F32, None) == -4
    assert lib.fz_sw_finalize2(p, p, p, 3, 100, BF16, None) == -4
    assert lib.fz_sw_finalize2(p, p, ctypes.c_void_p(128), 3, 100, 2, None) == -4
    assert lib.fz_sw_finalize2(p, p, p, 0, 100, F32, None) == -1
    assert lib.fz_sw_finalize2(p, p, p, 3, 0, F32, None) == -1
    # the original 3-D fp32 entry points keep refusing widths that are not multiples of 4
    assert lib.fz_sw_accumulate(p, p, p, p, p, p, 1e-3, 3, 4, 4, 101, 4, 4, 30, 0, 0, 0, None) == -2
