"""-m gpu: fz_seg_argmax (csrc/segmetric.hip) behind ft.discretize(argmax=True) / ft.one_hot_mask / ft.multiclass_counts /
ft.DiceMetric(argmax=True) / ft.HausdorffDistanceMetric(argmax=True) against the composed form on the CPU.  Everything here
is an integer or a decision: equality, no tolerance.  V covers one voxel, the scalar tail alone (7), one group of 4 with and
without a tail, and the SEG_CHUNK = 16384 seams; an unaligned view takes the one-voxel-per-lane kernel."""
import warnings

import pytest
import torch

import factorizer_amd as ft
from factorizer_amd import _native

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAN = float("nan")
VS = [1, 7, 8, 16384, 16385, 3 * 16384 + 5]


class Native:
    """the body must launch native kernels and may not take a composed device branch (those warn) — tests/test_gpu_loss.py"""

    def __enter__(self):
        self.n0 = _native.launch_count()
        self.w = warnings.catch_warnings()
        self.w.__enter__()
        warnings.simplefilter("error", RuntimeWarning)
        return self

    def __exit__(self, *exc):
        self.w.__exit__(*exc)
        if exc[0] is None:
            torch.cuda.synchronize()
            assert _native.launch_count() > self.n0, "native kernels were not launched"


def make(C, V, dtype, seed=0):
    """logits (2, C, V) with deliberate ties and NaNs at the first, a middle and the last voxel, labels (2, 1, V) with one
    value that names no class"""
    g = torch.Generator().manual_seed(seed)
    x = (torch.randn(2, C, V, generator=g) * 3).to(dtype)
    y = torch.randint(0, C, (2, 1, V), generator=g)
    for b, v in ((0, 0), (1, V // 2), (1, V - 1)):
        x[b, :, v] = 1.25                                   # all channels equal: class 0
    x[0, C - 1, V - 1] = x[0, 0, V - 1] = 40.0              # two equal maxima: class 0
    x[1, 0, 0] = NAN                                        # a NaN never wins
    x[0, :, V // 2] = NAN                                   # all NaN: class 0
    y[1, 0, V - 1] = C
    return x, y


def check_all(x, y, xd, yd, C):
    """label map, one-hot mask and counts of device tensors xd, yd against the CPU composed form of x, y"""
    want_map = ft.discretize(x, argmax=True)
    want_hot = ft.discretize(x, argmax=True, to_onehot=True)
    want_cnt = ft.multiclass_counts(x, y)
    with Native():
        got_map = ft.discretize(xd, argmax=True)
        got_hot = ft.discretize(xd, argmax=True, to_onehot=True)
        got_cnt = ft.multiclass_counts(xd, yd)
        got_cnt2 = ft.multiclass_counts(got_map, yd, num_classes=C)      # a uint8 label map as the prediction
        got_hot2 = ft.one_hot_mask(got_map, C)
    assert got_map.dtype == torch.uint8 and got_map.shape == want_map.shape and torch.equal(got_map.cpu(), want_map)
    assert got_hot.dtype == torch.uint8 and torch.equal(got_hot.cpu(), want_hot)
    assert got_cnt.dtype == torch.int64 and torch.equal(got_cnt.cpu(), want_cnt)
    assert torch.equal(got_cnt2, got_cnt) and torch.equal(got_hot2, got_hot)
    assert want_cnt[..., 1].sum() == x.shape[0] * x[0, 0].numel()        # every voxel is predicted as exactly one class


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("V", VS)
@pytest.mark.parametrize("C", [2, 3, 16])
def test_map_mask_and_counts_equal_the_cpu_composed_form(C, V, dtype):
    x, y = make(C, V, dtype, seed=C)
    check_all(x, y.to(torch.uint8), x.to(DEV), y.to(torch.uint8).to(DEV), C)


@pytest.mark.parametrize("ydt", [torch.int64, torch.float32])
@pytest.mark.parametrize("V", [8, 16385])
def test_label_kinds(V, ydt):
    x, y = make(5, V, torch.float32, seed=1)
    want = ft.multiclass_counts(x, y)
    yy = y.to(ydt)
    if ydt == torch.float32:
        yy = yy + 0.5                                        # truncates toward zero
    with Native():
        got = ft.multiclass_counts(x.to(DEV), yy.to(DEV))
    assert torch.equal(got.cpu(), want)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("V", [8, 16384])
def test_unaligned_view_one_element_into_its_storage(V, dtype):
    C = 3
    x, y = make(C, V, dtype, seed=2)
    xs = torch.zeros(2 * C * V + 1, dtype=dtype, device=DEV)
    xs[1:] = x.to(DEV).reshape(-1)
    ys = torch.zeros(2 * V + 1, dtype=torch.uint8, device=DEV)
    ys[1:] = y.to(torch.uint8).to(DEV).reshape(-1)
    xd, yd = xs[1:].view(2, C, V), ys[1:].view(2, 1, V)
    assert xd.data_ptr() % 16 and xd.is_contiguous()
    check_all(x, y.to(torch.uint8), xd, yd, C)


def test_spatial_ranks_and_dice_metric():
    x, y = make(4, 16 * 16 * 16, torch.float32, seed=3)
    want = ft.dice_metric(x, y, argmax=True, include_background=False, ignore_empty=True)
    for s in ((4096,), (64, 64), (16, 16, 16)):
        with Native():
            got = ft.DiceMetric(argmax=True, include_background=False, ignore_empty=True)(
                x.reshape(2, 4, *s).to(DEV), y.reshape(2, 1, *s).to(DEV))
        assert torch.equal(torch.nan_to_num(got.cpu(), nan=-1.0), torch.nan_to_num(want, nan=-1.0))


def test_hausdorff_metric_argmax_equals_hausdorff_distance_on_the_composed_masks():
    g = torch.Generator().manual_seed(4)
    x = torch.randn(2, 3, 16, 16, 16, generator=g)
    y = torch.randint(0, 3, (2, 1, 16, 16, 16), generator=g).to(torch.uint8)
    P, Y = ft.discretize(x, argmax=True, to_onehot=True), ft.one_hot_mask(y, 3)            # CPU: composed
    with Native():
        got = ft.HausdorffDistanceMetric(argmax=True, include_background=True, percentile=95)(x.to(DEV), y.to(DEV))
        want = ft.hausdorff_distance(P.to(DEV), Y.to(DEV), percentile=95)
    assert torch.equal(got, want)


@pytest.mark.parametrize("why,C,xdt,ydt", [("float16 logits", 3, torch.float16, torch.uint8), ("C = 17", 17, torch.float32, torch.uint8),
                                           ("int32 labels", 3, torch.float32, torch.int32)])
def test_composed_device_branch_warns_once_and_is_equal(why, C, xdt, ydt):
    from factorizer_amd import composed as CO
    x, y = make(C, 1000, torch.float32, seed=5)
    x = x.to(xdt)
    want = ft.multiclass_counts(x, y)
    for k in [k for k in CO._warned if k.startswith("metrics:multiclass_counts:")]:
        CO._warned.discard(k)
    n0 = _native.launch_count()
    with pytest.warns(RuntimeWarning, match="composed framework ops"):
        got = ft.multiclass_counts(x.to(DEV), y.to(ydt).to(DEV))
    with warnings.catch_warnings():
        warnings.simplefilter("error", RuntimeWarning)
        ft.multiclass_counts(x.to(DEV), y.to(ydt).to(DEV))
    torch.cuda.synchronize()
    assert _native.launch_count() == n0 and torch.equal(got.cpu(), want)
