"""-m gpu: the segmentation-metric kernels (csrc/segmetric.hip) against the independent CPU reference
tests/seg_metric_ref.py — integer counts equal, masks and edges bit for bit, unit-spacing minimum squared distances exact."""
import math
import warnings

import pytest
import torch
from torch import nn

import factorizer_amd as ft
from factorizer_amd import _native
from factorizer_amd import functional as Fn
import parity as P
import seg_metric_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F32, BF16, U8 = torch.float32, torch.bfloat16, torch.uint8


class Launches:
    """Asserts that the native library actually launched kernels inside the block."""

    def __enter__(self):
        self.n0 = _native.launch_count()
        return self

    def __exit__(self, *a):
        torch.cuda.synchronize()
        assert _native.launch_count() > self.n0, "native kernels were not launched"


def _logits(shape, seed, threshold, dtype, offset=0):
    """logits none of which lies within 1e-3 of the decision bound: a sign and a magnitude >= 0.05, moved by the bound.
    (bf16 rounding moves a value by at most |x| 2^-9 < 0.02 here, so the margin survives it — asserted.)  `offset`: the
    tensor starts that many elements into its buffer (an unaligned base)."""
    g = torch.Generator().manual_seed(seed)
    n = math.prod(shape)
    mag = 0.05 + torch.randn(n, generator=g).abs() * 1.5
    sign = torch.where(torch.rand(n, generator=g) < 0.45, 1.0, -1.0)
    b = R.bound64(True, threshold)
    buf = torch.zeros(n + offset, dtype=dtype)
    buf[offset:] = (sign * mag + b).to(dtype)
    z = buf[offset:].view(shape)
    assert ((z.double() - b).abs() > 1e-3).all()
    return buf, z


def _labels(shape, seed, dtype, offset=0):
    g = torch.Generator().manual_seed(seed + 1000)
    n = math.prod(shape)
    buf = torch.zeros(n + offset, dtype=dtype)
    buf[offset:] = (torch.rand(n, generator=g) > 0.55).to(dtype)
    return buf, buf[offset:].view(shape)


def _dev(buf, shape, offset):
    return buf.to(DEV)[offset:].view(shape)


COUNT_CASES = [((2, 3, 128, 128, 128), p, l, 0.5, 0) for p in (F32, BF16) for l in (U8, F32, BF16)] + [
    ((2, 3, 128, 128, 128), F32, U8, 0.3, 0), ((2, 3, 128, 128, 128), BF16, U8, 0.7, 0),
    ((1, 1, 37, 50, 23), F32, U8, 0.5, 1), ((1, 1, 37, 50, 23), BF16, BF16, 0.7, 3), ((1, 1, 37, 50, 23), F32, F32, 0.3, 0),
    ((1, 3, 240, 240, 155), F32, U8, 0.5, 0), ((1, 3, 240, 240, 155), BF16, F32, 0.3, 0),
    ((1, 1, 2048, 2048), F32, U8, 0.5, 0), ((1, 1, 2048, 2048), BF16, BF16, 0.7, 0),
    ((2, 2, 1001), F32, U8, 0.5, 0), ((2, 2, 1001), BF16, F32, 0.3, 0), ((2, 2, 1001), F32, BF16, 0.7, 5),
]


@pytest.mark.parametrize("shape,pdt,ldt,threshold,offset", COUNT_CASES)
def test_counts_masks_and_dice_equal_the_reference(shape, pdt, ldt, threshold, offset):
    """Every voxel takes part: the logits keep 1e-3 from the bound, so the float64 decision of the reference is the fp32
    decision of the kernel.  Counts equal as integers, the mask of the same pass bit for bit, Dice within 2^-22."""
    zb, z = _logits(shape, 7, threshold, pdt, offset)
    yb, y = _labels(shape, 7, ldt, offset)
    zd, yd = _dev(zb, shape, offset), _dev(yb, shape, offset)
    with Launches(), warnings.catch_warnings():
        warnings.simplefilter("error")                       # inside the native gate: nothing composed
        got = ft.segmentation_counts(zd, yd, threshold=threshold)
        mask = ft.discretize(zd, threshold=threshold)
        dice = ft.dice_metric(zd, yd, threshold=threshold, ignore_empty=True)
    ref = R.counts(z, y, threshold=threshold)
    assert got.dtype == torch.int64 and torch.equal(got.cpu(), ref), (got.cpu() - ref).tolist()
    assert mask.dtype == torch.uint8 and torch.equal(mask.cpu().bool(), R.decide(z, True, threshold))
    rd = R.dice(ref, ignore_empty=True)
    assert torch.equal(torch.isnan(dice.cpu()), torch.isnan(rd))
    err = (dice.cpu().double() - rd).abs().nan_to_num(0.0).max().item()
    P.note("dice abs err", shape=list(shape), pred=str(pdt), label=str(ldt), threshold=threshold, max_abs_err=err)
    assert err <= 2.0 ** -22, err


def test_counts_zero_logits_and_empty_planes():
    """A block of logits exactly at 0.0 is foreground at threshold 0.5 (−0.0 as well); empty label / prediction planes give
    the NaN / 1 / 0 entries of the Dice table at the reference's positions."""
    shape = (2, 3, 64, 64, 48)
    _, z = _logits(shape, 3, 0.5, F32)
    _, y = _labels(shape, 3, U8)
    z, y = z.clone(), y.clone()
    z[0, 0, 10:30, 7:40, 5:29] = 0.0
    z[0, 0, 31, 7:40, 5:29] = -0.0
    y[0, 1] = 0                    # empty label, non-empty prediction
    y[1, 2] = 0; z[1, 2] = -1.0    # both empty
    z[1, 0] = -2.0                 # empty prediction only
    zd, yd = z.to(DEV), y.to(DEV)
    with Launches():
        got = ft.segmentation_counts(zd, yd)
        mask = ft.discretize(zd)
    ref = R.counts(z, y)
    assert torch.equal(got.cpu(), ref)
    assert mask[0, 0, 10:30, 7:40, 5:29].all() and mask[0, 0, 31, 7:40, 5:29].all()
    assert torch.equal(mask.cpu().bool(), R.decide(z))
    for ie in (False, True):
        d, rd = ft.dice_metric(zd, yd, ignore_empty=ie).cpu(), R.dice(ref, ignore_empty=ie)
        assert torch.equal(torch.isnan(d), torch.isnan(rd))
        assert (d.double() - rd).abs().nan_to_num(0.0).max().item() <= 2.0 ** -22
    assert ft.dice_metric(zd, yd)[0, 1] == 0.0 and ft.dice_metric(zd, yd)[1, 2] == 1.0
    # discrete inputs: the mask of the pass above, as uint8 and as bool, and probabilities with sigmoid=False
    assert torch.equal(ft.segmentation_counts(mask, yd).cpu(), ref)
    assert torch.equal(ft.segmentation_counts(mask.bool(), yd.bool()).cpu(), ref)
    pr = torch.sigmoid(zd)
    assert torch.equal(ft.segmentation_counts(pr, yd, sigmoid=False, threshold=0.5).cpu(), R.counts(pr.cpu(), y, sigmoid=False))
    # accumulating form
    m = ft.DiceMetric(ignore_empty=True)
    m(zd, yd); m(zd[:1], yd[:1])
    assert m.get_buffer().shape == (3, 3) and torch.isfinite(m.aggregate())


def test_composed_device_branch_warns_once():
    z = torch.randn(1, 2, 16, 16, 16, device=DEV)
    y = (torch.rand(1, 2, 16, 16, 16, device=DEV) > 0.5).to(U8)
    with pytest.warns(RuntimeWarning, match="composed") as rec:
        a = ft.segmentation_counts(z.half(), y)
        ft.segmentation_counts(z.half(), y)
    assert len([w for w in rec if "segmentation_counts" in str(w.message)]) == 1
    assert torch.equal(a.cpu(), R.counts(z.half().cpu(), y.cpu()))
    assert torch.equal(ft.segmentation_counts(z.double(), y).cpu(), R.counts(z.cpu(), y.cpu()))


def test_counts_and_hausdorff_replay_bitwise():
    shape = (2, 3, 96, 96, 96)
    _, z = _logits(shape, 5, 0.5, F32)
    zd = z.to(DEV)
    yd = R.blobs(shape, 21, 0.5, 4).to(U8).to(DEV)
    a, b = ft.segmentation_counts(zd, yd), ft.segmentation_counts(zd, yd)
    assert torch.equal(a, b)
    pm = R.blobs((1, 2, 64, 64, 64), 22, 0.5, 4).to(U8).to(DEV)
    lm = R.blobs((1, 2, 64, 64, 64), 23, 0.5, 4).to(U8).to(DEV)
    h1 = ft.hausdorff_distance(pm, lm, percentile=95, spacing=(1.0, 1.5, 0.7))
    h2 = ft.hausdorff_distance(pm, lm, percentile=95, spacing=(1.0, 1.5, 0.7))
    assert torch.isfinite(h1).all() and torch.equal(h1.view(torch.int32), h2.view(torch.int32))


# ---- edges -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(2, 3, 5000), (2, 3, 301, 207), (1, 4, 61, 50, 47), (1, 2, 128, 128, 128)])
def test_edges_equal_the_reference(shape):
    """Random blobs (thresholded smoothed noise); plane (0, 0) emptied, plane (0, 1) filled, the last plane made to touch
    every face of the image."""
    m = R.blobs(shape, 31, 0.3, 3)
    m[0, 0] = False
    m[0, 1] = True
    last = m[-1, -1]
    for ax in range(last.dim()):
        last.select(ax, 0).fill_(True)
        last.select(ax, last.shape[ax] - 1).fill_(True)
    ref = R.edges(m)
    for md in (m.to(U8).to(DEV), m.to(DEV)):
        with Launches():
            e, n = Fn.mask_edges(md)
        assert e.dtype == torch.uint8 and torch.equal(e.cpu().bool(), ref)
        assert torch.equal(n.cpu(), ref.flatten(2).sum(-1))
        assert torch.equal(ft.mask_edges(md), e)
    assert n[0, 0] == 0


# ---- minimum squared distances ---------------------------------------------------------------------------------------------
def _edge_lists(shape, seed, level, smooth):
    e = R.edges(R.blobs(shape, seed, level, smooth))
    return torch.nonzero(e[0, 0]), torch.nonzero(e[0, 1])


def _coords4(idx):
    c = torch.zeros((idx.shape[0], 4), dtype=torch.float32)
    c[:, :idx.shape[1]] = idx.float()
    return c.to(DEV)


# (image, seed, level, smooth): edge voxels per plane — 96^3: about 2.9e4 x 2.7e4 = 8e8 pairs, the largest the brute-force
# reference takes in seconds; the others are far smaller
DIST_CASES = [((1, 2, 96, 96, 96), 41, 1.15, 6), ((1, 2, 40, 70, 33), 42, 0.2, 2), ((1, 2, 512, 640), 43, 0.8, 5),
              ((1, 2, 4000), 44, 0.0, 3)]


@pytest.mark.parametrize("shape,seed,level,smooth", DIST_CASES)
def test_min_dist2_unit_spacing_exact(shape, seed, level, smooth):
    """Every difference, square and sum is an integer below 2^24: the fp32 kernel must return the int64 brute-force minimum
    exactly, in both directions, whatever the order of the lists."""
    q, t = _edge_lists(shape, seed, level, smooth)
    assert q.shape[0] > 0 and t.shape[0] > 0 and q.shape[0] * t.shape[0] < 1.05e9, (q.shape, t.shape)
    P.note("edge counts", shape=list(shape), nq=q.shape[0], nt=t.shape[0])
    for a, b in ((q, t), (t, q)):
        with Launches():
            got = Fn.edge_min_dist2(_coords4(a), _coords4(b), (1.0, 1.0, 1.0))
        ref = R.min_dist2_int(a, b)
        assert got.dtype == torch.float32 and torch.equal(got.cpu().to(torch.int64), ref)
        assert torch.equal(got.cpu(), ref.float())
    # list order: permute both lists, un-permute the result
    g = torch.Generator().manual_seed(seed)
    pq, pt = torch.randperm(q.shape[0], generator=g), torch.randperm(t.shape[0], generator=g)
    got = Fn.edge_min_dist2(_coords4(q), _coords4(t), (1.0, 1.0, 1.0))
    got_p = Fn.edge_min_dist2(_coords4(q[pq]), _coords4(t[pt]), (1.0, 1.0, 1.0))
    assert torch.equal(got_p.cpu(), got.cpu()[pq])


def test_min_dist2_anisotropic_spacing():
    """d = fl(fl(w0 dx²) + w1 dy²) + w2 dz² with w = fl(s²): dx², dy², dz² are exact integers; each weight carries one rounding
    (u = 2^-24), each of the three products one more (the two FMAs round product and sum together, which only helps), the
    two additions of non-negative terms one each, and the minimum over candidates amplifies nothing: |err| <= (1 + 1 + 2) u
    = 2.4e-7 relative to first order — inside the 1e-6 asserted."""
    sp = (1.0, 1.5, 0.7)
    w = [s * s for s in sp]
    worst = 0.0
    for shape, seed, level, smooth in (((1, 2, 96, 96, 96), 41, 1.15, 6), ((1, 2, 40, 70, 33), 42, 0.2, 2)):
        q, t = _edge_lists(shape, seed, level, smooth)
        for a, b in ((q, t), (t, q)):
            got = Fn.edge_min_dist2(_coords4(a), _coords4(b), w).cpu().double()
            ref = R.min_dist2(a, b, sp)
            rel = ((got - ref).abs() / ref.clamp_min(1e-300)).masked_fill(ref == 0, 0.0)
            assert (got[ref == 0] == 0).all()
            worst = max(worst, rel.max().item())
    P.note("min dist2 spacing (1, 1.5, 0.7) rel err", max_rel_err=worst)
    assert worst <= 1e-6, worst


# ---- Hausdorff values ------------------------------------------------------------------------------------------------------
def _rel_err(got, ref):
    """largest elementwise relative error over the finite entries; NaN / inf must sit at the same places, zeros be zeros"""
    got, ref = got.cpu().double(), ref.double()
    assert got.shape == ref.shape
    assert torch.equal(torch.isnan(got), torch.isnan(ref)) and torch.equal(got == math.inf, ref == math.inf), (got, ref)
    fin = torch.isfinite(ref)
    g, r = got[fin], ref[fin]
    assert (g[r == 0] == 0).all()
    rel = ((g - r).abs() / r.clamp_min(1e-300)).masked_fill(r == 0, 0.0)
    return rel.max().item() if rel.numel() else 0.0


def _hd_check(pm, lm, spacing, what):
    """hausdorff_distance for percentiles 95, 50, None and both `directed` settings against the reference, 1e-6 relative
    per value; NaN and inf at the same places"""
    pd_, ld_ = pm.to(U8).to(DEV), lm.to(U8).to(DEV)
    table = R.hausdorff_table(pm, lm, [95, 50, None], spacing)
    worst = 0.0
    for pct in (95, 50, None):
        for directed in (False, True):
            with Launches():
                got = ft.hausdorff_distance(pd_, ld_, percentile=pct, spacing=spacing, directed=directed)
            worst = max(worst, _rel_err(got, table[pct][0 if directed else 1]))
    P.note(f"hausdorff rel err: {what}", max_rel_err=worst)
    assert worst <= 1e-6, worst


def test_hausdorff_values_3d_with_empty_planes():
    shape = (2, 3, 32, 40, 28)
    pm, lm = R.blobs(shape, 51, 0.4, 2), R.blobs(shape, 52, 0.4, 2)
    pm[0, 1] = False                 # NaN: no prediction edge
    lm[1, 0] = False                 # inf when directed, NaN undirected
    pm[1, 2] = False; lm[1, 2] = False
    _hd_check(pm, lm, None, "3-D unit")
    _hd_check(pm, lm, (1.0, 1.5, 0.7), "3-D spacing (1, 1.5, 0.7)")
    got = ft.hausdorff_distance(pm.to(U8).to(DEV), lm.to(U8).to(DEV), percentile=95, include_background=False)
    assert got.shape == (2, 2)
    m = ft.HausdorffDistanceMetric(include_background=True, percentile=95)
    v = m(pm.to(U8).to(DEV), lm.to(U8).to(DEV))
    assert v.shape == (2, 3) and torch.isfinite(m.aggregate())


def _vessels(shape, seed, width=0.06, smooth=6):
    """vessel-like 2-D masks: thin bands around the zero level set of smooth noise"""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(shape, generator=g)
    k = 2 * smooth + 1
    B, C = shape[:2]
    x = x.reshape(B * C, 1, *shape[2:])
    for _ in range(2):
        x = nn.functional.avg_pool2d(x, k, stride=1, padding=smooth)
    x = x.reshape(shape)
    return (x / x.std()).abs() < width


def test_hausdorff_values_2d_vessels_and_1d():
    pm, lm = _vessels((1, 2, 512, 512), 61), _vessels((1, 2, 512, 512), 62)
    n = R.edges(pm).flatten(2).sum(-1)
    P.note("vessel edge counts", pred=n.tolist(), label=R.edges(lm).flatten(2).sum(-1).tolist())
    assert (n > 1000).all()
    _hd_check(pm, lm, (0.5, 2.0), "2-D vessels 512^2")
    _hd_check(R.blobs((2, 2, 3000), 63, 0.0, 4), R.blobs((2, 2, 3000), 64, 0.0, 4), 0.25, "1-D")


def test_hausdorff_axis_beyond_the_exact_range_is_composed_and_warns_once():
    from factorizer_amd import composed
    composed._warned.discard("metrics:hausdorff_distance:axis")
    pm, lm = R.blobs((1, 2, 6, 2049), 71, 0.0, 2), R.blobs((1, 2, 6, 2049), 72, 0.0, 2)
    pd_, ld_ = pm.to(U8).to(DEV), lm.to(U8).to(DEV)
    with pytest.warns(RuntimeWarning) as rec:
        a = ft.hausdorff_distance(pd_, ld_, percentile=95)
        b = ft.hausdorff_distance(pd_, ld_, percentile=None)
    assert len([w for w in rec if "2049" in str(w.message)]) == 1
    table = R.hausdorff_table(pm, lm, [95, None])
    assert _rel_err(a, table[95][1]) <= 1e-6 and _rel_err(b, table[None][1]) <= 1e-6


# ---- end to end ------------------------------------------------------------------------------------------------------------
def test_validation_pass_end_to_end():
    """A small Factorizer through ft.sliding_window_inference on a 96 x 96 x 80 volume, its stitched logits into ft.DiceMetric
    and ft.HausdorffDistanceMetric, against the reference applied to the same logits.  Logits within 1e-3 of the bound are
    left out of the count comparison; that may concern at most 0.1 % of the voxels (a condition of the test)."""
    torch.manual_seed(0)
    model = ft.Factorizer(in_channels=4, out_channels=3, spatial_size=(32, 32, 32), encoder_depth=(1, 1, 1),
                          encoder_width=(32, 64, 128), strides=(1, 2, 2), decoder_depth=(1, 1), norm=ft.LayerNorm,
                          reshape=(ft.SWMatricize, {"head_dim": 8, "patch_size": 8}), act=nn.ReLU, factorize=ft.NMF,
                          rank=1, num_iters=5, init="uniform", solver="hals", mlp_ratio=2, dropout=0.0).to(DEV).eval()
    g = torch.Generator().manual_seed(1)
    x = torch.rand((1, 4, 96, 96, 80), generator=g).to(DEV)
    label = R.blobs((1, 3, 96, 96, 80), 81, 1.3, 6).to(U8)
    with torch.no_grad(), Launches():
        logits = ft.sliding_window_inference(x, (32, 32, 32), 4, model, overlap=0.5, mode="gaussian")
        # an untrained head: move each channel so that its top 3 % is foreground (both classes occur, and the edge lists stay
        # short enough for the brute-force reference) and give it unit spread (a monotone map of the stitched logits)
        V = logits[0, 0].numel()
        logits = (logits - logits.flatten(2).kthvalue(int(0.97 * V), dim=-1).values[:, :, None, None, None]) \
            / logits.std(dim=(2, 3, 4), keepdim=True)
        dm, hm = ft.DiceMetric(), ft.HausdorffDistanceMetric(include_background=True, percentile=95)
        dice = dm(logits, label.to(DEV))
        mask = ft.discretize(logits)
        hd = hm(mask, label.to(DEV))
    z = logits.cpu()
    near = z.abs() < 1e-3
    share = near.float().mean().item()
    P.note("end to end: share of logits within 1e-3 of the bound", share=share)
    assert share <= 1e-3, share
    far = ~near
    got_mask = mask.cpu().bool()
    assert torch.equal(got_mask[far], R.decide(z)[far])
    y = label.bool()
    ref_far = torch.stack([((R.decide(z) & y) & far).flatten(2).sum(-1), (R.decide(z) & far).flatten(2).sum(-1),
                           (y & far).flatten(2).sum(-1)], dim=-1)
    got_far = torch.stack([((got_mask & y) & far).flatten(2).sum(-1), (got_mask & far).flatten(2).sum(-1),
                           (y & far).flatten(2).sum(-1)], dim=-1)
    assert torch.equal(got_far, ref_far)
    # the counts of the kernel are those of its own mask, every voxel included
    cnt = ft.segmentation_counts(logits, label.to(DEV)).cpu()
    assert torch.equal(cnt, R.counts(got_mask.to(U8), label))
    assert (dice.cpu().double() - R.dice(cnt)).abs().max().item() <= 2.0 ** -22
    # Hausdorff on the mask the kernel wrote (the reference sees the same voxels)
    ref_hd = R.hausdorff(got_mask, label, 95)
    err = _rel_err(hd, ref_hd)
    P.note("end to end HD95 rel err", max_rel_err=err)
    assert err <= 1e-6, err
    assert math.isfinite(float(dm.aggregate())) and hm.get_buffer().shape == (1, 3)
