"""ft.dice_metric / ft.hausdorff_distance and their pieces on CPU tensors (the composed path and the host logic), against
the independent reference tests/seg_metric_ref.py, plus the host-side argument checks of the new entry points."""
import ctypes
import math
import warnings

import pytest
import torch

import factorizer_amd as ft
import seg_metric_ref as R

SHAPES = [(2, 3, 257), (2, 2, 33, 29), (1, 3, 12, 11, 9)]


def _case(shape, seed, pdtype=torch.float32, ldtype=torch.uint8):
    g = torch.Generator().manual_seed(seed)
    z = (torch.randn(shape, generator=g) * 2).to(pdtype)
    y = (torch.rand(shape, generator=g) > 0.6).to(ldtype)
    return z, y


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("pdtype,ldtype", [(torch.float32, torch.uint8), (torch.bfloat16, torch.float32),
                                           (torch.float32, torch.bool), (torch.float32, torch.bfloat16)])
@pytest.mark.parametrize("threshold", [0.5, 0.3])
def test_counts_and_dice_equal_the_reference(shape, pdtype, ldtype, threshold):
    z, y = _case(shape, 1, pdtype, ldtype)
    with warnings.catch_warnings():
        warnings.simplefilter("error")          # CPU tensors: composed ops, silently
        got = ft.segmentation_counts(z, y, threshold=threshold)
        d = ft.dice_metric(z, y, threshold=threshold)
        m = ft.discretize(z, threshold=threshold)
    ref = R.counts(z, y, threshold=threshold)
    assert got.dtype == torch.int64 and got.shape == (*shape[:2], 3)
    assert torch.equal(got, ref)
    assert d.dtype == torch.float32 and torch.equal(d, R.dice(ref).to(torch.float32))
    assert m.dtype == torch.uint8 and torch.equal(m.bool(), R.decide(z, threshold=threshold))


def test_discrete_predictions_and_non_binary_labels():
    z, y = _case((2, 2, 16, 16), 2)
    p = ft.discretize(z)
    assert torch.equal(ft.segmentation_counts(p, y), R.counts(z, y))            # a mask is taken as it is
    assert torch.equal(ft.segmentation_counts(p.bool(), y), R.counts(z, y))
    prob = torch.sigmoid(z)
    assert torch.equal(ft.segmentation_counts(prob, y, sigmoid=False, threshold=0.5), R.counts(prob, y, sigmoid=False))
    assert torch.equal(ft.segmentation_counts(z, y.float() * 3.5), R.counts(z, y))   # a non-zero label counts as 1


def test_empty_plane_cases_of_the_dice_table():
    z = torch.full((1, 4, 8, 8), -1.0)
    y = torch.zeros((1, 4, 8, 8), dtype=torch.uint8)
    z[0, 0, :4] = 1.0; y[0, 0, 2:6] = 1          # |Y| > 0: 2 · 16 / (32 + 32)
    z[0, 1, :2] = 1.0                            # |Y| = 0, |P| > 0
    y[0, 3, 0, 0] = 1                            # |Y| > 0, |P| = 0
    d = ft.dice_metric(z, y)
    assert d.tolist() == [[0.5, 0.0, 1.0, 0.0]]
    d = ft.dice_metric(z, y, ignore_empty=True)
    assert d[0, 0] == 0.5 and math.isnan(d[0, 1]) and math.isnan(d[0, 2]) and d[0, 3] == 0.0
    d = ft.dice_metric(z, y, include_background=False)
    assert d.shape == (1, 3) and d.tolist() == [[0.0, 1.0, 0.0]]


def test_zero_logit_is_foreground_at_threshold_half():
    z = torch.zeros((1, 1, 4, 4))
    z[0, 0, 0] = -1e-30
    z[0, 0, 1, 0] = -0.0                          # −0.0 >= 0.0
    m = ft.discretize(z)
    assert m[0, 0, 1:].all() and not m[0, 0, 0].any()
    y = torch.ones((1, 1, 4, 4), dtype=torch.uint8)
    assert ft.segmentation_counts(z, y)[0, 0].tolist() == [12, 12, 16]
    assert ft.discretize(z.bfloat16())[0, 0, 1:].all()


def test_reductions_handle_nan():
    nan = math.nan
    f = torch.tensor([[1.0, nan, 0.5], [nan, nan, nan], [0.0, 1.0, nan]])
    from factorizer_amd.metrics import reduce_metric
    assert reduce_metric(f, "none") is f
    assert torch.allclose(reduce_metric(f, "mean_channel"), torch.tensor([0.75, 0.0, 0.5]))
    assert torch.allclose(reduce_metric(f, "mean_batch"), torch.tensor([0.5, 1.0, 0.5]))
    assert float(reduce_metric(f, "mean")) == pytest.approx((0.75 + 0.5) / 2)      # the all-NaN sample is left out
    assert float(reduce_metric(torch.full((2, 2), nan), "mean")) == 0.0
    with pytest.raises(ValueError):
        reduce_metric(f, "sum")


def test_dice_metric_class_buffer_aggregate_reset():
    m = ft.DiceMetric(ignore_empty=True)
    with pytest.raises(ValueError):
        m.aggregate()
    assert m.get_buffer() is None
    z1, y1 = _case((2, 3, 9, 9), 3)
    z2, y2 = _case((1, 3, 9, 9), 4)
    y2[0, 1] = 0                                  # a NaN entry
    v1, v2 = m(z1, y1), m(z2, y2)
    assert v1.shape == (2, 3) and v2.shape == (1, 3) and math.isnan(v2[0, 1])
    buf = m.get_buffer()
    ref = torch.cat([R.dice(R.counts(z1, y1), ignore_empty=True), R.dice(R.counts(z2, y2), ignore_empty=True)]).float()
    assert buf.shape == (3, 3) and torch.equal(torch.isnan(buf), torch.isnan(ref))
    assert torch.equal(buf.nan_to_num(7.0), ref.nan_to_num(7.0))
    per_sample = torch.stack([ref[0].mean(), ref[1].mean(), (ref[2, 0] + ref[2, 2]) / 2])
    assert float(m.aggregate()) == pytest.approx(float(per_sample.mean()), rel=1e-6)
    assert m.aggregate("mean_batch").shape == (3,) and m.aggregate("mean_channel").shape == (3,)
    assert m.aggregate("none").shape == (3, 3)
    m.reset()
    assert m.get_buffer() is None
    m2 = ft.DiceMetric(include_background=False, reduction="mean_batch", threshold=0.3)
    m2(z1, y1)
    assert torch.allclose(m2.aggregate(), R.dice(R.counts(z1, y1, threshold=0.3))[:, 1:].mean(0).float())
    with pytest.raises(ValueError):
        ft.DiceMetric(reduction="median")


# ---- edges -------------------------------------------------------------------------------------------------------------------
def test_edges_single_voxel_full_image_box_border():
    m = torch.zeros((1, 1, 7, 7, 7), dtype=torch.uint8)
    m[0, 0, 3, 3, 3] = 1
    assert torch.equal(ft.mask_edges(m), m)                                     # a single voxel is its own edge
    full = torch.ones((1, 1, 6, 5, 4), dtype=torch.uint8)
    e = ft.mask_edges(full)
    assert e.dtype == torch.uint8 and e[0, 0, 1:-1, 1:-1, 1:-1].sum() == 0      # only the border shell
    assert int(e.sum()) == 6 * 5 * 4 - 4 * 3 * 2
    box = torch.zeros((1, 1, 10, 10), dtype=torch.uint8)
    box[0, 0, 2:8, 3:9] = 1
    e = ft.mask_edges(box)
    assert int(e.sum()) == 6 * 6 - 4 * 4 and e[0, 0, 3:7, 4:8].sum() == 0 and e[0, 0, 2, 3:9].all()
    touch = torch.zeros((1, 1, 8, 8), dtype=torch.uint8)
    touch[0, 0, :3, :] = 1                                                      # touches three image borders
    e = ft.mask_edges(touch)
    want = torch.zeros_like(touch)
    want[0, 0, 0, :] = 1; want[0, 0, 2, :] = 1; want[0, 0, 1, 0] = 1; want[0, 0, 1, 7] = 1
    assert torch.equal(e, want)
    line = torch.tensor([0, 1, 1, 1, 1, 0, 1, 1], dtype=torch.uint8).reshape(1, 1, 8)
    assert ft.mask_edges(line).flatten().tolist() == [0, 1, 0, 0, 1, 0, 1, 1]


@pytest.mark.parametrize("shape", [(2, 2, 200), (1, 2, 40, 37), (1, 2, 18, 17, 16)])
def test_edges_equal_the_reference_on_blobs(shape):
    m = R.blobs(shape, 5)
    assert torch.equal(ft.mask_edges(m.to(torch.uint8)).bool(), R.edges(m))
    assert torch.equal(ft.mask_edges(m).bool(), R.edges(m))                     # bool masks as well


# ---- Hausdorff ---------------------------------------------------------------------------------------------------------------
def _boxes(shift=(0, 4, 0)):
    """two 6 x 6 x 6 boxes in a 20^3 image, the second moved by `shift`"""
    p = torch.zeros((1, 1, 20, 20, 20), dtype=torch.uint8)
    y = torch.zeros_like(p)
    p[0, 0, 4:10, 4:10, 4:10] = 1
    y[0, 0, 4 + shift[0]:10 + shift[0], 4 + shift[1]:10 + shift[1], 4 + shift[2]:10 + shift[2]] = 1
    return p, y


def test_hausdorff_offset_boxes_closed_form():
    # a box moved by 4 voxels along one axis: the far face of each box is 4 from the other box's far-side face, and no
    # surface voxel is farther than that
    p, y = _boxes((0, 4, 0))
    assert float(ft.hausdorff_distance(p, y, percentile=None)) == 4.0
    assert float(ft.hausdorff_distance(p, y, percentile=None, spacing=(1.0, 1.5, 0.7))) == pytest.approx(6.0, rel=1e-6)
    assert float(ft.hausdorff_distance(p, y, percentile=None, spacing=2.0)) == pytest.approx(8.0, rel=1e-6)
    p, y = _boxes((4, 0, 0))
    assert float(ft.hausdorff_distance(p, y, percentile=None, spacing=(1.0, 1.5, 0.7))) == pytest.approx(4.0, rel=1e-6)
    # identical masks: 0 at every percentile
    assert float(ft.hausdorff_distance(p, p, percentile=95)) == 0.0


@pytest.mark.parametrize("percentile", [None, 95, 50])
@pytest.mark.parametrize("spacing", [None, (1.0, 1.5, 0.7)])
@pytest.mark.parametrize("directed", [False, True])
def test_hausdorff_equals_the_reference(percentile, spacing, directed):
    p, y = _boxes((1, 4, 2))
    y[0, 0, 15:18, 15:18, 2:4] = 1                # a second component only the label has: directed ≠ undirected
    got = ft.hausdorff_distance(p, y, percentile=percentile, spacing=spacing, directed=directed)
    ref = R.hausdorff(p, y, percentile, spacing, directed_only=directed)
    assert got.dtype == torch.float32 and got.shape == (1, 1)
    assert float(got) == pytest.approx(float(ref), rel=1e-6)
    if not directed and percentile != 50:         # the label-only component is the far tenth of d(Y→P)
        assert float(got) > float(ft.hausdorff_distance(p, y, percentile=percentile, spacing=spacing, directed=True))


def test_hausdorff_lower_dimensions_and_background():
    p = R.blobs((2, 3, 48, 40), 6).to(torch.uint8)
    y = R.blobs((2, 3, 48, 40), 7).to(torch.uint8)
    got = ft.hausdorff_distance(p, y, percentile=95, spacing=(0.5, 2.0))
    ref = R.hausdorff(p, y, 95, (0.5, 2.0))
    assert torch.allclose(got.double(), ref, rtol=1e-6, atol=0)
    got = ft.hausdorff_distance(p, y, percentile=95, include_background=False)
    assert got.shape == (2, 2) and torch.allclose(got.double(), R.hausdorff(p, y, 95)[:, 1:], rtol=1e-6, atol=0)
    p1, y1 = R.blobs((1, 2, 300), 8).to(torch.uint8), R.blobs((1, 2, 300), 9).to(torch.uint8)
    assert torch.allclose(ft.hausdorff_distance(p1, y1, percentile=50).double(), R.hausdorff(p1, y1, 50), rtol=1e-6, atol=0)
    with pytest.raises(ValueError):
        ft.hausdorff_distance(p, y, spacing=(1.0, 1.0, 1.0))
    with pytest.raises(ValueError):
        ft.hausdorff_distance(p, y, percentile=101)


def test_hausdorff_empty_edge_sets():
    p, y = _boxes()
    z = torch.zeros_like(p)
    assert math.isnan(float(ft.hausdorff_distance(z, y, directed=True)))         # no edge in P
    assert math.isinf(float(ft.hausdorff_distance(p, z, directed=True)))         # none in Y only
    assert math.isnan(float(ft.hausdorff_distance(z, z, directed=True)))
    for a, b in ((z, y), (p, z), (z, z)):                                       # the maximum propagates the NaN direction
        assert math.isnan(float(ft.hausdorff_distance(a, b)))
        assert math.isnan(float(R.hausdorff(a, b)))


def test_hausdorff_metric_class_aggregates():
    m = ft.HausdorffDistanceMetric(include_background=True, percentile=95)
    p, y = _boxes((0, 4, 0))
    p2 = torch.cat([p, torch.zeros_like(p)], dim=1)        # channel 1 empty: NaN
    y2 = torch.cat([y, y], dim=1)
    v = m(p2, y2)
    assert v.shape == (1, 2) and math.isnan(v[0, 1])
    m(torch.cat([y, y], dim=1), y2)                        # identical: 0, 0
    assert m.get_buffer().shape == (2, 2)
    assert float(m.aggregate()) == pytest.approx(float(v[0, 0]) / 2)
    assert m.aggregate("mean_batch").tolist() == pytest.approx([float(v[0, 0]) / 2, 0.0])
    m.reset()
    assert m.get_buffer() is None
    assert ft.HausdorffDistanceMetric()(p2, y2).shape == (1, 1)    # MONAI's default leaves the background channel out


# ---- host-side argument checks of the entry points (no device call) -----------------------------------------------------------
def test_host_side_argument_checks():
    from factorizer_amd import _native, build
    build.build(verbose=False)
    lib = _native.lib()
    p8 = ctypes.c_void_p(64)      # a non-null, 16-byte aligned pointer value the host code never dereferences
    err = lib.fz_last_error_string
    assert lib.fz_seg_counts(None, 0, p8, 2, 0.0, None, p8, p8, 6, 4096, None) == -4 and b"null pred" in err()
    assert lib.fz_seg_counts(p8, 0, p8, 2, 0.0, None, None, p8, 6, 4096, None) == -4 and b"workspace" in err()
    assert lib.fz_seg_counts(p8, 0, p8, 2, 0.0, None, p8, None, 6, 4096, None) == -4 and b"neither" in err()
    assert lib.fz_seg_counts(p8, 5, p8, 2, 0.0, None, p8, p8, 6, 4096, None) == -4 and b"kind" in err()
    assert lib.fz_seg_counts(p8, 0, p8, 9, 0.0, None, p8, p8, 6, 4096, None) == -4 and b"kind" in err()
    assert lib.fz_seg_counts(p8, 0, p8, 2, math.nan, None, p8, p8, 6, 4096, None) == -4 and b"NaN" in err()
    assert lib.fz_seg_counts(p8, 0, p8, 2, 0.0, None, p8, p8, 0, 4096, None) == -1
    assert lib.fz_seg_counts(p8, 0, p8, 2, 0.0, None, p8, p8, 6, 0, None) == -1
    assert lib.fz_seg_counts(ctypes.c_void_p(66), 0, p8, 2, 0.0, None, p8, p8, 6, 4096, None) == -4 and b"aligned" in err()
    # workspace helpers: 3 uint32 per plane and chunk; never more than 4096 chunks per plane
    assert lib.fz_seg_counts_chunks(1) == 1 and lib.fz_seg_counts_chunks(16384) == 1 and lib.fz_seg_counts_chunks(16385) == 2
    assert lib.fz_seg_counts_chunks(128 ** 3) == 128 and lib.fz_seg_counts_chunks(1 << 34) <= 4096
    assert lib.fz_seg_counts_workspace_bytes(6, 128 ** 3) == 6 * 128 * 12 and lib.fz_seg_counts_workspace_bytes(0, 8) == -1

    assert lib.fz_mask_edges(None, p8, p8, 1, 3, 4, 4, 4, None) == -4 and b"null" in err()
    assert lib.fz_mask_edges(p8, p8, p8, 1, 3, 4, 4, 4, None) == -4 and b"alias" in err()
    q8 = ctypes.c_void_p(128)
    assert lib.fz_mask_edges(p8, q8, p8, 1, 4, 4, 4, 4, None) == -4 and b"nd" in err()
    assert lib.fz_mask_edges(p8, q8, p8, 1, 2, 4, 4, 4, None) == -1 and b"lifted" in err()
    assert lib.fz_mask_edges(p8, q8, p8, 1, 3, 0, 4, 4, None) == -1
    assert lib.fz_mask_edges(p8, q8, p8, 0, 3, 4, 4, 4, None) == -1

    assert lib.fz_edge_min_dist2(None, 4, p8, 4, 1.0, 1.0, 1.0, p8, None, None) == -4 and b"null" in err()
    assert lib.fz_edge_min_dist2(p8, 0, p8, 4, 1.0, 1.0, 1.0, p8, None, None) == -1
    assert lib.fz_edge_min_dist2(p8, 4, p8, 0, 1.0, 1.0, 1.0, p8, None, None) == -1
    assert lib.fz_edge_min_dist2(p8, 4, p8, 4, -1.0, 1.0, 1.0, p8, None, None) == -4 and b"weights" in err()
    assert lib.fz_edge_min_dist2(p8, 4, p8, 4, math.inf, 1.0, 1.0, p8, None, None) == -4
    assert lib.fz_edge_min_dist2(ctypes.c_void_p(72), 4, p8, 4, 1.0, 1.0, 1.0, p8, None, None) == -4 and b"aligned" in err()
    assert lib.fz_edge_min_dist2(p8, 4, p8, 100000, 1.0, 1.0, 1.0, p8, None, None) == -4 and b"workspace" in err()
    # splits: one for a short target list, several (and a workspace of splits x nq floats) for a long one, at most 64
    assert lib.fz_edge_min_dist2_splits(100, 100) == 1 and lib.fz_edge_min_dist2_workspace_bytes(100, 100) == 0
    ns = lib.fz_edge_min_dist2_splits(50000, 50000)
    assert 1 < ns <= 64 and lib.fz_edge_min_dist2_workspace_bytes(50000, 50000) == ns * 50000 * 4
    assert lib.fz_edge_min_dist2_splits(10, 10 ** 8) <= 64 and lib.fz_edge_min_dist2_splits(0, 5) == 0
