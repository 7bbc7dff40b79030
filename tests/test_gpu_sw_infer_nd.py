"""-m gpu: native sliding-window stitching (csrc/sw_infer.hip, fz_sw_*2) on 1-D, 2-D and 3-D images, any window width and
origin, fp32 and bf16 network outputs — against the 3-D oracle of oracle/cpu_ref.py lifted to 1-D / 2-D, against the
original fz_sw_* kernels bit for bit in 3-D fp32, and through the FIVES bundle's Deconver end to end.  Every native case
asserts that native kernels ran."""
import warnings

import pytest
import torch
from torch import nn

import factorizer_amd as ft
from factorizer_amd import _native, composed
from factorizer_amd import inference as I
from oracle import cpu_ref as O
from test_sw_infer_nd_cpu import lifted_oracle

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BF = torch.bfloat16


class Launches:
    """Asserts that the native library launched kernels inside the block."""

    def __enter__(self):
        self.n0 = _native.launch_count()
        return self

    def __exit__(self, *a):
        torch.cuda.synchronize()
        assert _native.launch_count() > self.n0, "native kernels were not launched"


def conv_tanh(nd, cin=2, cout=3, seed=0, out_dtype=None):
    torch.manual_seed(seed)
    conv = (nn.Conv1d, nn.Conv2d, nn.Conv3d)[nd - 1](cin, cout, 3, padding=1)

    def net(x):
        conv.to(x.device)
        y = torch.tanh(conv(x.float()))
        return y if out_dtype is None else y.to(out_dtype)
    return net


def oracle(x, roi, sw, net, ov, mode="gaussian"):
    return (O.sliding_window_oracle(x, roi, sw, net, overlap=ov, mode=mode) if x.dim() == 5
            else lifted_oracle(x, roi, sw, net, overlap=ov, mode=mode))


class Recorder:
    """Wraps a device network: keeps every window it saw and its output, so that the CPU oracle can stitch the SAME window
    outputs (upcast to fp32) — and checks on replay that the oracle's windows are the gathered ones, bit for bit."""

    def __init__(self, net):
        self.net, self.seen = net, []

    def __call__(self, w):
        y = self.net(w)
        self.seen.append((w.cpu(), y.float().cpu()))
        return y

    def replay(self):
        it = iter(self.seen)

        def f(w):
            wi, yi = next(it)
            assert torch.equal(w, wi)
            return yi
        return f


# 2-D / 1-D / 3-D geometries; W, x0 or rw not multiples of 4 take the element-wise bodies
GEOMS = [((1000, 1298), (512, 512), 0.5, 1),     # 3 x 5 windows, the last at x0 = 786 (FIVES roi on an odd-width image)
         ((37, 50), (16, 24), 0.5, 2),           # W = 50: element-wise; pulled-back windows at (21, 26)
         ((40, 64), (16, 32), 0.5, 2),           # everything a multiple of 4: 16-byte bodies
         ((100,), (32,), 0.25, 2),               # 1-D, x0 = 0, 24, 48, 68
         ((101,), (30,), 0.5, 2),                # 1-D, rw = 30
         ((12, 14, 27), (8, 8, 10), 0.5, 2),     # 3-D, rw = 10 (the original entry points refuse it)
         ((10, 12, 23), (8, 6, 7), 0.25, 1)]


@pytest.mark.parametrize("size,roi,ov,B", GEOMS)
@pytest.mark.parametrize("mode", ["gaussian", "constant"])
def test_native_stitching_matches_lifted_oracle(size, roi, ov, B, mode):
    net = conv_tanh(len(size))
    x = torch.randn(B, 2, *size)
    with torch.no_grad():
        with Launches(), warnings.catch_warnings():
            warnings.simplefilter("error", RuntimeWarning)
            y = ft.sliding_window_inference(x.to(DEV), roi, 3, net, overlap=ov, mode=mode)
        yo = oracle(x, roi, 3, net, ov, mode)
    assert y.shape == (B, 3, *size) and y.dtype == torch.float32
    assert torch.allclose(y.cpu(), yo, rtol=1e-5, atol=1e-5)


def _stitch_with_original_entry_points(x, roi, sw, net, ov):
    """the parent revision's native path: fz_sw_gather / fz_sw_accumulate / fz_sw_finalize (3-D fp32, rw % 4 == 0)"""
    L, st = _native.lib(), _native.stream_ptr(x)
    B, C, size = x.shape[0], x.shape[1], tuple(x.shape[2:])
    starts = I.window_starts(size, roi, I.scan_interval(size, roi, (ov,) * 3))
    fac, floor = I.gaussian_factors(roi, 0.125, torch.float32, x.device)
    jobs = [(b, s) for b in range(B) for s in starts]
    out = cnt = None
    for j0 in range(0, len(jobs), sw):
        chunk = jobs[j0:j0 + sw]
        win = torch.empty((len(chunk), C, *roi), device=x.device)
        for i, (b, s) in enumerate(chunk):
            _native.check(L.fz_sw_gather(x[b].data_ptr(), win[i].data_ptr(), C, *size, *roi, *s, st), "fz_sw_gather")
        prob = net(win).contiguous()
        if out is None:
            out = torch.zeros((B, prob.shape[1], *size), device=x.device)
            cnt = torch.zeros((B, *size), device=x.device)
        for i, (b, s) in enumerate(chunk):
            _native.check(L.fz_sw_accumulate(prob[i].data_ptr(), out[b].data_ptr(), cnt[b].data_ptr(), fac[0].data_ptr(),
                                             fac[1].data_ptr(), fac[2].data_ptr(), float(floor), prob.shape[1], *size,
                                             *roi, *s, st), "fz_sw_accumulate")
    for b in range(B):
        _native.check(L.fz_sw_finalize(out[b].data_ptr(), cnt[b].data_ptr(), out.shape[1], out[b, 0].numel(), st),
                      "fz_sw_finalize")
    return out


@pytest.mark.parametrize("size,roi,ov", [((20, 24, 27), (16, 16, 16), 0.5), ((32, 16, 40), (16, 16, 8), 0.25),
                                         ((16, 16, 16), (16, 16, 16), 0.5)])
def test_3d_fp32_bit_identical_to_the_original_kernels(size, roi, ov):
    """the geometries of test_gpu_parity.py::test_sliding_window_inference_native: W = 27 with x0 = 11 (unaligned), W = 40
    (16-byte bodies), one window"""
    net = conv_tanh(3)
    x = torch.randn(2, 2, *size, device=DEV)
    with torch.no_grad(), Launches():
        y_new = ft.sliding_window_inference(x, roi, 2, net, overlap=ov, mode="gaussian")
        y_old = _stitch_with_original_entry_points(x, roi, 2, net, ov)
    assert torch.equal(y_new, y_old)


def fives_deconver():
    """model_zoo/deconver_fives/configs/inference.yaml:31-47"""
    torch.manual_seed(0)
    return ft.Deconver(in_channels=3, out_channels=1, spatial_dims=2, encoder_depth=(1, 1, 1, 1, 1),
                       encoder_width=(32, 64, 128, 256, 512), strides=(1, 2, 2, 2, 2), decoder_depth=(1, 1, 1, 1),
                       norm=nn.InstanceNorm2d, act=nn.ReLU, groups=-1, ratio=1, kernel_size=(7, 7), num_iters=1,
                       mlp_ratio=4).to(DEV).eval()


@pytest.mark.parametrize("size,nwin", [((2048, 2048), 49), ((1000, 1298), 15)])
def test_fives_bundle_inference_end_to_end(size, nwin):
    """SlidingWindowInfererAdapt(roi 512^2, sw_batch 4, overlap 0.5, gaussian) (inference.yaml:77-83) around the bundle's
    2-D Deconver: native stitching against framework stitching of the same (deterministic) network outputs"""
    model = fives_deconver()
    x = torch.rand(1, 3, *size, device=DEV)
    inf = ft.SlidingWindowInfererAdapt(roi_size=(512, 512), sw_batch_size=4, overlap=0.5, mode="gaussian")
    calls = []

    def net(w):
        calls.append(w.shape[0])
        return model(w)
    with torch.no_grad():
        with Launches():
            y = inf(x, net)
        assert sum(calls) == nwin
        y2 = I.sliding_window_inference(x, (512, 512), 4, model, overlap=0.5, mode="gaussian", _composed=True)
    assert y.shape == (1, 1, *size) and y.dtype == torch.float32 and torch.isfinite(y).all()
    assert torch.allclose(y, y2, rtol=1e-5, atol=1e-5)
    # partition of unity: a constant network comes back exactly constant
    ones = inf(x, lambda w: torch.ones(w.shape[0], 1, *w.shape[2:], device=w.device))
    assert torch.allclose(ones, torch.ones_like(ones), rtol=0, atol=1e-6)


@pytest.mark.parametrize("size,roi,ov,in_dtype", [((37, 50), (16, 24), 0.5, torch.float32),
                                                  ((40, 64), (16, 32), 0.5, BF),
                                                  ((20, 24, 27), (16, 16, 16), 0.5, torch.float32),
                                                  ((12, 14, 27), (8, 8, 10), 0.5, BF)])
def test_bf16_network_outputs(size, roi, ov, in_dtype):
    """bf16 window outputs are summed in fp32 and rounded once: the result is bf16 and within one bf16 rounding (2^-8
    relative) of the oracle's fp32 stitch of the same window outputs; bf16 inputs are gathered byte-exactly (Recorder)"""
    rec = Recorder(conv_tanh(len(size), out_dtype=BF))
    x = torch.randn(2, 2, *size).to(in_dtype)
    with torch.no_grad():
        with Launches(), warnings.catch_warnings():
            warnings.simplefilter("error", RuntimeWarning)
            y = ft.sliding_window_inference(x.to(DEV), roi, 3, rec, overlap=ov, mode="gaussian")
            y2 = ft.sliding_window_inference(x.to(DEV), roi, 3, rec.net, overlap=ov, mode="gaussian")
        yo = oracle(x, roi, 3, rec.replay(), ov)
    assert y.dtype == BF and y.shape == (2, 3, *size)
    assert torch.equal(y, y2)                                   # run to run: bitwise
    err = (y.float().cpu() - yo).abs()
    assert (err <= 2.0 ** -8 * yo.abs() + 1e-6).all(), err.max()


def test_factorizer_under_bf16_autocast():
    """the README's small Factorizer under torch.autocast(bfloat16): bf16 logits, native stitching, pulled-back windows"""
    torch.manual_seed(0)
    model = ft.Factorizer(in_channels=4, out_channels=3, spatial_size=(32, 32, 32), encoder_depth=(1, 1, 1),
                          encoder_width=(32, 64, 128), strides=(1, 2, 2), decoder_depth=(1, 1), norm=ft.LayerNorm,
                          reshape=(ft.SWMatricize, {"head_dim": 8, "patch_size": 8}), act=nn.ReLU, factorize=ft.NMF,
                          rank=1, num_iters=5, init="uniform", solver="hals", mlp_ratio=2, dropout=0.0).to(DEV).eval()
    x = torch.rand(1, 4, 40, 32, 45, device=DEV)
    with torch.no_grad(), torch.autocast("cuda", dtype=BF), Launches():
        y = ft.SlidingWindowInfererAdapt(roi_size=(32, 32, 32), sw_batch_size=2, overlap=0.5, mode="gaussian")(x, model)
    assert y.shape == (1, 3, 40, 32, 45) and y.dtype == BF and torch.isfinite(y.float()).all()


def test_fp16_outputs_warn_once_and_stay_correct():
    """fp16 network outputs are outside the native set: one RuntimeWarning, framework stitching, values still right"""
    composed._warned.discard(f"sw_stitch:{torch.float16}")
    net = conv_tanh(2, out_dtype=torch.float16)
    x = torch.randn(1, 2, 37, 50)
    with torch.no_grad():
        with pytest.warns(RuntimeWarning, match="float16"), Launches():     # the fp32 windows are still gathered natively
            y = ft.sliding_window_inference(x.to(DEV), (16, 24), 2, net, overlap=0.5, mode="gaussian")
        with warnings.catch_warnings():
            warnings.simplefilter("error", RuntimeWarning)                   # once
            ft.sliding_window_inference(x.to(DEV), (16, 24), 2, net, overlap=0.5, mode="gaussian")
            # the test hook stays silent
            I.sliding_window_inference(x.to(DEV), (16, 24), 2, net, overlap=0.5, mode="gaussian", _composed=True)
        yo = lifted_oracle(x, (16, 24), 2, lambda w: net(w).float())
    assert y.dtype == torch.float16
    assert torch.allclose(y.float().cpu(), yo, rtol=1e-2, atol=1e-2)
