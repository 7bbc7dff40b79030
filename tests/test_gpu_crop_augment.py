"""-m gpu: the crop cut inside the augmentation gather (csrc/aug_crop.hip).  The defining identity against the existing kernels
(ft.crop_augment_batch == ft.augment_batch on the device-stacked boxes, bit for bit), the independent float64 reference
tests/aug_ref.py on host-cut crops, proof that nothing outside a box is read, the paths around the native gate, replay, and
the module.  The roi shapes, matrices and flips are those of tests/aug_cases.py."""
import warnings

import numpy as np
import pytest
import torch

import factorizer_amd as ft
from factorizer_amd import _native, composed
from factorizer_amd import augment as AG
import aug_cases as K
import aug_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F32, BF16 = torch.float32, torch.bfloat16

# name: (roi, C, L, source shapes, origin sets).  Every set has one origin per source; over the sets every free axis sees 0 and
# N - roi.  "3d": source W 33 makes rows unaligned, source W 40 takes the vector source path at origin x 0 / 4 / 12 and the
# scalar one at 3 (labels and bf16; fp32 rows are dword-aligned wherever they start), D and H equal to the roi pin those origins at 0; the third source is the first tensor again.  "2d": roi W 47
# runs the masked tail, W equal to the roi pins origin x at 0.  "2dv": the 2-D output-side vector path.
GEOM = {
    "3d": ((20, 24, 28), 3, 2, [(23, 31, 33), (20, 24, 40), (23, 31, 33)],
           [[(0, 0, 0), (0, 0, 0), (3, 7, 5)], [(3, 7, 5), (0, 0, 4), (0, 0, 0)], [(1, 2, 3), (0, 0, 12), (3, 0, 4)],
            [(0, 7, 0), (0, 0, 3), (2, 4, 5)]]),
    "2d": ((33, 47), 2, 1, [(40, 47), (33, 64), (37, 50)],
           [[(0, 0), (0, 0), (0, 0)], [(7, 0), (0, 17), (4, 3)], [(3, 0), (0, 8), (2, 1)]]),
    "2dv": ((16, 20), 2, 1, [(21, 32), (17, 23)],
            [[(0, 0), (0, 0)], [(5, 12), (1, 3)], [(2, 4), (0, 1)], [(1, 3), (1, 0)]]),
}


class Launches:
    """Asserts that the native library launched exactly `n` kernels inside the block."""

    def __init__(self, n):
        self.n = n

    def __enter__(self):
        self.n0 = _native.launch_count()
        return self

    def __exit__(self, *a):
        torch.cuda.synchronize()
        got = _native.launch_count() - self.n0
        assert got == self.n, f"{got} native launches"


def _np(t):
    return t.detach().cpu().double().numpy()


def _bf16_steps(a, b):
    """distance of two bf16 tensors in representable values (0 = equal, 1 = neighbours)"""
    def key(t):
        i = t.cpu().contiguous().view(torch.int16).to(torch.int32)
        return torch.where(i >= 0, i, -(i & 0x7FFF))
    return (key(a) - key(b)).abs().max().item()


def _sources(name, seed, dtype=F32, device=DEV):
    roi, C, L, shapes, _ = GEOM[name]
    xs = [K.image((1, C) + s, seed + i, dtype)[0].to(device) for i, s in enumerate(shapes)]
    ls = [K.label((1, L) + s, seed + i, L)[0].to(device) for i, s in enumerate(shapes)]
    for i in range(1, len(shapes)):
        if shapes[i] == shapes[0]:
            xs[i], ls[i] = xs[0], ls[0]                                     # one source used twice in the batch
    return xs, ls


def _cut(ts, org, roi):
    return torch.stack([t[(slice(None),) + tuple(slice(o, o + r) for o, r in zip(g, roi))] for t, g in zip(ts, org)])


def _all_steps(B, nd, seed=0x7EA5EED0BADC0DE):
    """records with affine, flips, noise, smoothing and gain / offset drawn on every sample"""
    p = ft.draw_augment_params(B, nd, generator=torch.Generator().manual_seed(21 + B + nd), affine_prob=1, noise_prob=1,
                               smooth_prob=1, scale_intensity_prob=1, shift_intensity_prob=1)
    p.seed = seed
    assert all(not torch.equal(p.affine[b], torch.eye(nd)) for b in range(B)) and (p.sigma > 0).all() and p.flip.any()
    return p


def _flips_only(B, nd):
    p = ft.AugmentParams.identity(B, nd)
    p.flip = torch.tensor([[(b + k) % 2 == 0 for k in range(nd)] for b in range(B)])
    p.flip[B - 1] = True
    return p


# ---- 1. the identity, native against native ----------------------------------------------------------------------------------
@pytest.mark.parametrize("label_dtype", [torch.uint8, torch.bool])
@pytest.mark.parametrize("dtype", [F32, BF16])
@pytest.mark.parametrize("name", list(GEOM))
def test_crop_in_the_gather_equals_augment_batch_on_stacked_crops(name, dtype, label_dtype):
    roi, C, L, shapes, origin_sets = GEOM[name]
    B, nd = len(shapes), len(roi)
    xs, ls = _sources(name, 1, dtype)
    if label_dtype == torch.bool:
        ls = [l > 1 for l in ls]
    drawn, ident, flips = _all_steps(B, nd), ft.AugmentParams.identity(B, nd), _flips_only(B, nd)
    for org in origin_sets:
        x, l = _cut(xs, org, roi), _cut(ls, org, roi)                       # device slices + stack: what the fused path saves
        with Launches(2):                                                   # the crop gather + ONE smoothing launch
            gi, gl = ft.crop_augment_batch(xs, ls, org, roi, drawn)
        ci, cl = ft.augment_batch(x, l, drawn)
        assert gi.dtype == dtype and gl.dtype == label_dtype and gi.shape == (B, C) + roi and gl.shape == (B, L) + roi
        assert torch.equal(gi, ci) and torch.equal(gl, cl), (org, "all steps")
        with Launches(1):                                                   # identity records: a pure batched crop
            gi, gl = ft.crop_augment_batch(xs, ls, org, roi, ident)
        assert torch.equal(gi, x) and torch.equal(gl, l), (org, "identity")
        with Launches(1):
            gi, gl = ft.crop_augment_batch(xs, ls, org, roi)                # params=None means the same
        assert torch.equal(gi, x) and torch.equal(gl, l)
        with Launches(1):
            gi, gl = ft.crop_augment_batch(xs, ls, org, roi, flips)
        ci, cl = ft.augment_batch(x, l, flips)
        assert torch.equal(gi, ci) and torch.equal(gl, cl), (org, "flips")
        dims = [1 + k for k in range(nd)]
        assert torch.equal(gi[B - 1], x[B - 1].flip(dims)) and torch.equal(gl[B - 1], l[B - 1].flip(dims))


def test_the_vector_and_the_scalar_source_paths_are_both_taken():
    """the origin sets above reach both: what the kernel decides per sample is restated by augment.source_vector_loads"""
    seen = set()
    for name in ("3d", "2dv"):
        roi, C, L, shapes, origin_sets = GEOM[name]
        xs, ls = _sources(name, 1)
        for org in origin_sets:
            imgs, labs, g, r = AG._crop_sources(xs, ls, org, roi)
            v = AG.source_vector_loads(AG._crop_table(imgs, labs, g, r), roi, 4)
            seen |= {(name, bool(a), bool(b)) for a, b in v.tolist()}
            for b, s in enumerate(shapes):                                   # torch's device allocations are aligned
                assert bool(v[b, 0]) and bool(v[b, 1]) == (s[-1] % 4 == 0 and org[b][-1] % 4 == 0)
            vb = AG.source_vector_loads(AG._crop_table(imgs, labs, g, r), roi, 2)            # the same boxes read as bf16
            seen |= {(name, "bf16", bool(a)) for a in vb[:, 0].tolist()}
    assert {("3d", True, True), ("3d", True, False), ("2dv", True, True), ("2dv", True, False)} <= seen
    assert {(n, "bf16", a) for n in ("3d", "2dv") for a in (True, False)} <= seen


# ---- 2. against the float64 reference ------------------------------------------------------------------------------------------
CASES = [(3, i) for i in range(6)] + [(2, i) for i in range(3)]
_REF = {}


def _case(nd, i, dtype):
    """sources, origins, records and the float64 reference of resample case i on host-cut crops, computed once and shared"""
    k = (nd, i, dtype)
    if k not in _REF:
        name = "3d" if nd == 3 else "2d"
        roi, C, L, shapes, origin_sets = GEOM[name]
        shape, A, F = K.resample_cases(nd)[i]
        assert tuple(shape[2:]) == roi
        B = A.shape[0]
        xs, ls = _sources(name, 10 + i, dtype, "cpu")
        pick = [(i + b) % len(shapes) for b in range(B)]                    # which sources the batch is cut from moves with i
        org = [origin_sets[(i + 1) % len(origin_sets)][j] for j in pick]
        xs, ls = [xs[j] for j in pick], [ls[j] for j in pick]
        p = ft.AugmentParams.identity(B, nd)
        p.affine, p.flip = A, F
        ri, rl = R.augment(_cut(xs, org, roi).double().numpy(), _cut(ls, org, roi).numpy(), A.double().numpy(), F.numpy(),
                           p.noise_std.numpy(), p.sigma.numpy(), p.gain.numpy(), p.offset.numpy())
        ri.setflags(write=False)
        rl.setflags(write=False)
        _REF[k] = (xs, ls, org, roi, p, ri, rl)
    return _REF[k]


@pytest.mark.parametrize("nd,i", CASES)
def test_cropped_linear_resample_fp32(nd, i):
    xs, ls, org, roi, p, ri, rl = _case(nd, i, F32)
    B = len(xs)
    for b in range(B):
        if not torch.equal(p.affine[b], torch.eye(nd)):
            assert R.clamp_share(_np(p.affine[b]), p.flip[b].tolist(), roi) > 0.01     # the crop's border padding is exercised
    with Launches(1):
        gi, gl = ft.crop_augment_batch([x.to(DEV) for x in xs], [l.to(DEV) for l in ls], org, roi, p)
    err = np.abs(_np(gi) - ri).max()
    print(f"cropped resample nd={nd} case {i} origins {org}: max abs err {err:.3e}")
    assert err <= 2e-5
    for b in range(B):      # labels: exact outside the voxels whose float64 position is within 1e-3 of a half-integer
        exempt = R.near_half(_np(p.affine[b]), p.flip[b].tolist(), roi)
        print(f"  sample {b}: exempt share {exempt.mean():.4f}")
        assert exempt.mean() <= 0.02
        assert np.array_equal(gl[b].cpu().numpy()[:, ~exempt], rl[b][:, ~exempt])


@pytest.mark.parametrize("nd,i", [(3, 0), (3, 4), (2, 1)])
def test_cropped_linear_resample_bf16_within_one_ulp(nd, i):
    xs, ls, org, roi, p, ri, _ = _case(nd, i, BF16)
    gi, _ = ft.crop_augment_batch([x.to(DEV) for x in xs], None, org, roi, p)
    assert gi.dtype == BF16
    steps = _bf16_steps(gi, torch.tensor(ri).to(BF16))
    print(f"bf16 cropped resample nd={nd} case {i}: {steps} bf16 steps")
    assert steps <= 1


# ---- 3. nothing outside the box is read --------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(GEOM))
def test_voxels_outside_every_box_never_reach_the_output(name):
    """the same batch twice — outside every box NaN (images) and 255 (labels), then 0: bitwise equal outputs.  An origin added
    before the clamp, or a +1 corner taken from the source instead of the box, reads the poison."""
    roi, C, L, shapes, origin_sets = GEOM[name]
    B, nd = len(shapes), len(roi)
    xs, ls = _sources(name, 3)
    p = _all_steps(B, nd)
    p.sigma.zero_()                                                          # the smoothing pass reads the workspace only
    p.affine[0] = torch.eye(nd)                                              # one sample on the identity path
    for org in origin_sets[1:3]:
        outs = []
        for fill_x, fill_l in ((float("nan"), 255), (0.0, 0)):
            px, pl = {}, {}
            for t, l in zip(xs, ls):                                         # one poisoned copy per distinct source tensor
                if id(t) not in px:
                    px[id(t)], pl[id(t)] = torch.full_like(t, fill_x), torch.full_like(l, fill_l)
            for b in range(B):
                box = (slice(None),) + tuple(slice(o, o + r) for o, r in zip(org[b], roi))
                px[id(xs[b])][box] = xs[b][box]
                pl[id(xs[b])][box] = ls[b][box]
            with Launches(1):
                outs.append(ft.crop_augment_batch([px[id(t)] for t in xs], [pl[id(t)] for t in xs], org, roi, p))
        (ai, al), (bi, bl) = outs
        assert not torch.isnan(ai).any() and int(al.max()) <= 3
        assert torch.equal(ai, bi) and torch.equal(al, bl), org


# ---- 4. paths ------------------------------------------------------------------------------------------------------------------
def test_either_tensor_alone_a_source_twice_and_lifted_sources():
    roi, C, L, shapes, origin_sets = GEOM["3d"]
    xs, ls = _sources("3d", 4)
    assert xs[2] is xs[0]
    org = origin_sets[2]
    p = _all_steps(3, 3)
    both = ft.crop_augment_batch(xs, ls, org, roi, p)
    with Launches(2):
        gi, none = ft.crop_augment_batch(xs, None, org, roi, p)
    assert none is None and torch.equal(gi, both[0])
    with Launches(1):                                                       # labels do not smooth
        none, gl = ft.crop_augment_batch(None, ls, org, roi, p)
    assert none is None and torch.equal(gl, both[1])
    gi, gl = ft.crop_augment_batch([x[None] for x in xs], [l[None] for l in ls], org, roi, p)     # PreparedVolume's shape
    assert torch.equal(gi, both[0]) and torch.equal(gl, both[1])
    same = ft.crop_augment_batch([xs[1]] * 3, [ls[1]] * 3, [(0, 0, 0), (0, 0, 4), (0, 0, 3)], roi)
    assert torch.equal(same[0][1], xs[1][:, :, :, 4:32]) and torch.equal(same[1][2], ls[1][:, :, :, 3:31])


def test_a_non_contiguous_source_warns_once_and_gives_the_same_result():
    roi, C, L, shapes, origin_sets = GEOM["2d"]
    xs, ls = _sources("2d", 5)
    org = origin_sets[1]
    p = _all_steps(3, 2)
    want = ft.crop_augment_batch(xs, ls, org, roi, p)
    strided = list(xs)
    strided[1] = xs[1].transpose(1, 2).contiguous().transpose(1, 2)          # the same values, other strides
    assert not strided[1].is_contiguous()
    composed._warned.discard("augment:crop_augment_batch:contiguous")
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        with Launches(2):
            got = ft.crop_augment_batch(strided, ls, org, roi, p)
        ft.crop_augment_batch(strided, ls, org, roi, p)
    assert len([m for m in w if "not contiguous" in str(m.message)]) == 1
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])


def _gate_params(B, nd):
    p = ft.AugmentParams.identity(B, nd, seed=99)
    p.affine[0] = ft.augment.affine_matrix((0.2,) * {1: 0, 2: 1, 3: 3}[nd], (1.1,) * nd, nd)
    p.flip[1, nd - 1] = True
    p.noise_std[0] = 0.05
    p.sigma[1] = 0.8
    p.gain[0], p.offset[1] = 1.2, 0.05
    return p


@pytest.mark.parametrize("shapes,roi,org,dtype,tol", [
    ([(2, 13, 12, 17), (2, 10, 15, 14)], (10, 12, 14), [(3, 0, 3), (0, 3, 0)], torch.float16, 1e-3),
    ([(3, 64), (3, 57)], (57,), [(7,), (0,)], F32, 1e-5)])
def test_outside_the_gate_runs_composed_with_one_warning_and_matches_the_cpu(shapes, roi, org, dtype, tol):
    nd = len(roi)
    xs = [K.image((1,) + s, 40 + i, dtype)[0] for i, s in enumerate(shapes)]
    ls = [K.label((1,) + s, 40 + i, 1)[0] for i, s in enumerate(shapes)]
    p = _gate_params(2, nd)
    for k in [k for k in composed._warned if k.startswith("augment:")]:
        composed._warned.discard(k)
    n0 = _native.launch_count()
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        gi, gl = ft.crop_augment_batch([x.to(DEV) for x in xs], [l.to(DEV) for l in ls], org, roi, p)
        ft.crop_augment_batch([x.to(DEV) for x in xs], [l.to(DEV) for l in ls], org, roi, p)
    assert len([m for m in w if "composed framework ops" in str(m.message)]) == 1
    assert "crop_augment_batch" in str([m for m in w if "composed framework ops" in str(m.message)][0].message)
    assert _native.launch_count() == n0
    ci, cl = ft.crop_augment_batch(xs, ls, org, roi, p)
    assert gi.dtype == dtype and gi.is_cuda and gi.shape == (2, shapes[0][0]) + roi
    assert (gi.cpu().double() - ci.double()).abs().max().item() <= tol
    assert torch.equal(gl.cpu(), cl)


# ---- 5. replay -----------------------------------------------------------------------------------------------------------------
def test_two_calls_with_equal_inputs_and_seed_are_bitwise_equal():
    roi, C, L, shapes, origin_sets = GEOM["3d"]
    xs, ls = _sources("3d", 6, BF16)
    p = _all_steps(3, 3)
    a = ft.crop_augment_batch(xs, ls, origin_sets[3], roi, p)
    b = ft.crop_augment_batch(xs, ls, origin_sets[3], roi, p)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    p.seed += 1
    c = ft.crop_augment_batch(xs, ls, origin_sets[3], roi, p)
    assert not torch.equal(a[0], c[0]) and torch.equal(a[1], c[1])


# ---- 6. the module -------------------------------------------------------------------------------------------------------------
def test_rand_crop_augment_module_on_device():
    roi, C, L, shapes, _ = GEOM["3d"]
    xs, ls = _sources("3d", 7)
    aug = ft.RandCropAugment(3, roi, affine_prob=0.6, noise_prob=0.6, smooth_prob=0.6)
    g = torch.Generator().manual_seed(11)
    a, b = aug(xs, ls, generator=g)
    g.manual_seed(11)
    org = ft.draw_crop_origins(xs, roi, g)
    params = ft.draw_augment_params(3, 3, generator=g, **aug.kwargs)
    c, d = ft.crop_augment_batch(xs, ls, org, roi, params)
    assert torch.equal(a, c) and torch.equal(b, d) and not a.requires_grad and a.shape == (3, C) + roi and a.is_cuda
    aug.eval()
    with Launches(1):
        a, b = aug(xs, ls)
    centre = [tuple((n - r) // 2 for n, r in zip(s, roi)) for s in shapes]
    assert torch.equal(a, _cut(xs, centre, roi)) and torch.equal(b, _cut(ls, centre, roi))
