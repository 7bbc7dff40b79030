"""CPU side of the mutually-exclusive-class metrics (factorizer_amd/metrics.py): argmax with ties to the lowest index and NaNs
that never win, the one-hot mask, the three integer counts per (sample, class) against brute force, and the Dice values they
give through the unchanged `_dice_from_counts`."""
import math

import pytest
import torch
import torch.nn.functional as F

import factorizer_amd as ft
from factorizer_amd import metrics as M

NAN = float("nan")


def brute_argmax(x):
    """lowest index of the largest non-NaN value, 0 when there is none — a python loop over voxels"""
    B, C = x.shape[:2]
    flat = x.double().reshape(B, C, -1)
    out = torch.zeros(B, flat.shape[2], dtype=torch.int64)
    for b in range(B):
        for v in range(flat.shape[2]):
            best, k = -math.inf, 0
            for c in range(C):
                val = flat[b, c, v].item()
                if val > best:
                    best, k = val, c
            out[b, v] = k
    return out.reshape(B, 1, *x.shape[2:])


def brute_counts(p, y, C):
    """(B, C, 3) from two int64 class maps (B, 1, *S); a class outside [0, C) matches nothing"""
    B = p.shape[0]
    out = torch.zeros(B, C, 3, dtype=torch.int64)
    for b in range(B):
        for c in range(C):
            P, Y = p[b] == c, y[b] == c
            out[b, c] = torch.tensor([(P & Y).sum(), P.sum(), Y.sum()])
    return out


def tie_case(dtype=torch.float32):
    x = torch.randn(2, 4, 3, 5, generator=torch.Generator().manual_seed(0)).to(dtype)
    x[0, :, 0, 0] = 1.5                      # all channels equal: class 0
    x[0, 1, 0, 1] = x[0, 3, 0, 1] = 9.0      # two equal maxima: the lower index, 1
    x[0, 2, 0, 2] = x[0, 3, 0, 2] = 9.0      # ... 2
    x[1, 0, 1, 1] = NAN                      # a NaN never wins, here against three numbers
    x[1, 3, 1, 2] = NAN
    x[1, :, 2, 2] = NAN                      # all NaN: class 0
    x[1, :, 2, 3] = -math.inf                # all −inf: class 0
    x[1, 0, 2, 4], x[1, 1:, 2, 4] = NAN, -math.inf   # NaN, then −inf everywhere: nothing exceeds −inf, class 0
    return x


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float64])
def test_argmax_ties_and_nans(dtype):
    x = tie_case(dtype)
    m = ft.discretize(x, argmax=True)
    assert m.dtype == torch.uint8 and m.shape == (2, 1, 3, 5)
    assert torch.equal(m.long(), brute_argmax(x))
    assert m[0, 0, 0, 0] == 0 and m[0, 0, 0, 1] == 1 and m[0, 0, 0, 2] == 2 and m[1, 0, 2, 2] == 0 and m[1, 0, 1, 1] != 0
    oh = ft.discretize(x, argmax=True, to_onehot=True)
    assert oh.dtype == torch.uint8 and torch.equal(oh, F.one_hot(m[:, 0].long(), 4).movedim(-1, 1).to(torch.uint8))


def test_bf16_ties_are_decided_on_the_stored_values():
    """two fp32 values that differ only below bf16 resolution tie once stored as bf16: the lower index wins there"""
    x = torch.zeros(1, 3, 4)
    x[0, 2] = 1.0 + 2.0 ** -10
    x[0, 1] = 1.0
    assert ft.discretize(x, argmax=True).unique().tolist() == [2]
    assert ft.discretize(x.to(torch.bfloat16), argmax=True).unique().tolist() == [1]


def test_argmax_argument_checks():
    x = torch.zeros(1, 3, 4)
    for kw in (dict(threshold=0.3), dict(sigmoid=False)):
        with pytest.raises(ValueError):
            ft.discretize(x, argmax=True, **kw)
        with pytest.raises(ValueError):
            ft.dice_metric(x, torch.zeros(1, 1, 4), argmax=True, **kw)
        with pytest.raises(ValueError):
            ft.DiceMetric(argmax=True, **kw)
    with pytest.raises(ValueError):
        ft.discretize(torch.zeros(1, 1, 4), argmax=True)
    with pytest.raises(ValueError):
        ft.discretize(x, to_onehot=True)
    with pytest.raises(ValueError):
        ft.multiclass_counts(torch.zeros(1, 1, 4, dtype=torch.uint8), torch.zeros(1, 1, 4, dtype=torch.uint8))   # num_classes
    with pytest.raises(ValueError):
        ft.multiclass_counts(x, torch.zeros(1, 3, 4))
    assert torch.equal(ft.discretize(x), (x >= 0).to(torch.uint8))       # the thresholded form is as it was


@pytest.mark.parametrize("dt", [torch.uint8, torch.int64, torch.float32, torch.int32])
def test_one_hot_mask(dt):
    y = torch.randint(0, 5, (2, 1, 4, 6), generator=torch.Generator().manual_seed(1))
    got = ft.one_hot_mask(y.to(dt), 5)
    assert got.dtype == torch.uint8 and torch.equal(got, F.one_hot(y[:, 0], 5).movedim(-1, 1).to(torch.uint8))
    y[0, 0, 0, 0], y[1, 0, 1, 1] = 5, 200                            # out of range: an all-zero row
    got = ft.one_hot_mask(y.to(dt), 5)
    assert got[0, :, 0, 0].sum() == 0 and got[1, :, 1, 1].sum() == 0 and got.sum() == y.numel() - 2


@pytest.mark.parametrize("C,shape", [(2, (9,)), (3, (4, 5)), (16, (3, 4, 5))])
@pytest.mark.parametrize("ydt", [torch.uint8, torch.int64, torch.float32])
def test_multiclass_counts_against_brute_force(C, shape, ydt):
    g = torch.Generator().manual_seed(2)
    x = torch.randn(2, C, *shape, generator=g)
    y = torch.randint(0, C, (2, 1, *shape), generator=g)
    y[0][y[0] == C - 1] = 0                    # class C − 1 is absent from sample 0's labels
    x[1, 1] = -50.0                            # class 1 is never predicted in sample 1
    y.view(2, -1)[1, 0] = C                    # one label names no class
    got = ft.multiclass_counts(x, y.to(ydt))
    p = brute_argmax(x)
    assert got.dtype == torch.int64 and torch.equal(got, brute_counts(p, y, C))
    assert got[0, C - 1, 2] == 0 and got[1, 1, 1] == 0
    assert torch.equal(ft.multiclass_counts(p.to(torch.uint8), y.to(ydt), num_classes=C), got)   # a label map as prediction
    assert torch.equal(ft.multiclass_counts(x, y.to(ydt), num_classes=C), got)


@pytest.mark.parametrize("ib", [True, False])
@pytest.mark.parametrize("ie", [True, False])
def test_dice_metric_argmax(ib, ie):
    g = torch.Generator().manual_seed(3)
    C = 4
    x = torch.randn(3, C, 6, 6, generator=g)
    y = torch.randint(0, C, (3, 1, 6, 6), generator=g)
    y[0][y[0] == 3] = 0                        # class 3 absent from sample 0, predicted there
    y[1][y[1] == 2] = 0
    x[1, 2] = -50.0                            # class 2 absent and not predicted in sample 1
    counts = brute_counts(brute_argmax(x), y, C).double()
    want = 2 * counts[..., 0] / (counts[..., 1] + counts[..., 2])
    empty = counts[..., 2] == 0
    fill = torch.full_like(want, NAN) if ie else (counts[..., 1] == 0).double()
    want = torch.where(empty, fill, want).float()
    want = want if ib else want[:, 1:]
    got = ft.dice_metric(x, y, argmax=True, include_background=ib, ignore_empty=ie)
    assert got.shape == want.shape and torch.equal(torch.nan_to_num(got, nan=-1.0), torch.nan_to_num(want, nan=-1.0))
    m = ft.DiceMetric(argmax=True, include_background=ib, ignore_empty=ie)
    m(x[:2], y[:2])
    m(x[2:], y[2:])
    assert torch.equal(torch.nan_to_num(m.get_buffer(), nan=-1.0), torch.nan_to_num(want, nan=-1.0))
    assert torch.equal(m.aggregate(), M.reduce_metric(want, "mean"))
    if ie:
        assert torch.isnan(got[0, -1]) and torch.isnan(got[1, 2 - (0 if ib else 1)])
    else:
        assert got[0, -1] == 0.0 and got[1, 2 - (0 if ib else 1)] == 1.0


def test_hausdorff_metric_argmax_is_hausdorff_distance_on_the_one_hot_masks():
    g = torch.Generator().manual_seed(4)
    x = torch.randn(1, 3, 8, 8, 8, generator=g)
    y = torch.randint(0, 3, (1, 1, 8, 8, 8), generator=g)
    got = ft.HausdorffDistanceMetric(argmax=True, include_background=True, percentile=95)(x, y)
    P = F.one_hot(brute_argmax(x)[:, 0], 3).movedim(-1, 1).to(torch.uint8)
    Y = F.one_hot(y[:, 0], 3).movedim(-1, 1).to(torch.uint8)
    assert torch.equal(got, ft.hausdorff_distance(P, Y, percentile=95))
