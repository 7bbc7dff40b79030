"""ft.crop_augment_batch, ft.draw_crop_origins and ft.RandCropAugment on CPU tensors: the defining identity (a crop cut inside
the gather == augment_batch on the stacked boxes, bit for bit), the independent float64 reference tests/aug_ref.py on host-cut
crops, the origin draws, the host source table, the errors, and the host-side argument checks of fz_aug_crop_resample (called
through ctypes; nothing touches a device)."""
import ctypes
import warnings

import numpy as np
import pytest
import torch

import factorizer_amd as ft
from factorizer_amd import augment as AG
import aug_cases as K
import aug_ref as R

ROI3, ROI2 = K.SHAPE3[2:], K.SHAPE2[2:]                       # (20, 24, 28), (33, 47)
SRC3 = [(23, 31, 33), (20, 24, 40), (23, 31, 33)]             # ragged; sample 2 is sample 0's tensor again
SRC2 = [(40, 47), (33, 64), (37, 50), (40, 47)]               # sample 3 is sample 0's tensor again
ORG3 = [(0, 0, 0), (0, 0, 12), (3, 7, 5)]                     # 0 and N - roi on every axis
ORG2 = [(0, 0), (0, 17), (4, 3), (7, 0)]


def _sources(shapes, C, L, seed, dtype=torch.float32):
    xs = [K.image((1, C) + s, seed + i, dtype)[0] for i, s in enumerate(shapes)]
    ls = [K.label((1, L) + s, seed + i, L)[0] for i, s in enumerate(shapes)]
    for i in range(1, len(shapes)):
        if shapes[i] == shapes[0]:
            xs[i], ls[i] = xs[0], ls[0]                           # one source used twice
    return xs, ls


def _cut(ts, org, roi):
    return torch.stack([t[(slice(None),) + tuple(slice(o, o + r) for o, r in zip(g, roi))] for t, g in zip(ts, org)])


def _all_steps(B, nd, seed=0x1234567890ABCDE):
    """records with every step drawn on every sample"""
    g = torch.Generator().manual_seed(5)
    p = ft.draw_augment_params(B, nd, generator=g, affine_prob=1, noise_prob=1, smooth_prob=1, scale_intensity_prob=1,
                               shift_intensity_prob=1)
    p.seed = seed
    return p


# ---- draw_crop_origins ---------------------------------------------------------------------------------------------------------
def test_origins_stay_in_range_and_cover_it():
    g = torch.Generator().manual_seed(3)
    shapes = [(22, 24, 30), (20, 26, 28)] * 150                # N - roi = (2, 0, 2) and (0, 2, 0)
    o = ft.draw_crop_origins(shapes, ROI3, g)
    assert o.dtype == torch.int64 and o.shape == (300, 3) and o.device.type == "cpu"
    free = torch.tensor(shapes) - torch.tensor(ROI3)
    assert (o >= 0).all() and (o <= free).all()
    assert sorted(set(o[0::2, 0].tolist())) == [0, 1, 2] and sorted(set(o[1::2, 1].tolist())) == [0, 1, 2]
    assert (o[0::2, 1] == 0).all() and (o[1::2, 0] == 0).all()          # roi == N gives 0
    assert torch.equal(ft.draw_crop_origins([ROI3] * 4, ROI3, g), torch.zeros(4, 3, dtype=torch.int64))


def test_origins_repeat_with_the_generator_state_and_take_tensors():
    g = torch.Generator().manual_seed(4)
    state = g.get_state()
    shapes = [(40, 50, 60), (21, 25, 29)]
    a = ft.draw_crop_origins(shapes, ROI3, g)
    b = ft.draw_crop_origins(shapes, ROI3, g)
    g.set_state(state)
    c = ft.draw_crop_origins([torch.empty((2,) + shapes[0]), torch.empty((1, 2) + shapes[1])], ROI3, g)
    assert torch.equal(a, c) and not torch.equal(a, b)
    g.set_state(state)
    u = torch.rand(2, 3, generator=g, dtype=torch.float64)               # ONE rand call: g = floor(u (N - roi + 1))
    assert torch.equal(a, torch.floor(u * (torch.tensor(shapes) - torch.tensor(ROI3) + 1)).long())
    assert torch.equal(ft.draw_crop_origins([(9, 9)], 4, torch.Generator().manual_seed(1)),
                       ft.draw_crop_origins([(9, 9)], (4, 4), torch.Generator().manual_seed(1)))


def test_a_roi_above_the_extent_raises_with_sample_and_axis():
    with pytest.raises(ValueError, match="sample 1, axis 2"):
        ft.draw_crop_origins([(20, 24, 28), (20, 24, 27)], ROI3)


# ---- the defining identity -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nd", [3, 2])
def test_crop_inside_the_gather_equals_augment_on_the_stacked_boxes(nd):
    shapes, org, roi, C, L = (SRC3, ORG3, ROI3, 3, 2) if nd == 3 else (SRC2, ORG2, ROI2, 2, 1)
    xs, ls = _sources(shapes, C, L, 50)
    B = len(shapes)
    p = _all_steps(B, nd)
    with warnings.catch_warnings():
        warnings.simplefilter("error")                                   # CPU tensors: silently
        gi, gl = ft.crop_augment_batch(xs, ls, torch.tensor(org), roi, p)
    ci, cl = ft.augment_batch(_cut(xs, org, roi), _cut(ls, org, roi), p)
    assert gi.shape == (B, C) + roi and gl.shape == (B, L) + roi and gl.dtype == torch.uint8
    assert torch.equal(gi, ci) and torch.equal(gl, cl)
    assert xs[B - 1] is xs[0] and not torch.equal(gi[0], gi[B - 1])       # the same source, another box and record
    # pure crop: no records
    gi, gl = ft.crop_augment_batch(xs, ls, org, roi)
    assert torch.equal(gi, _cut(xs, org, roi)) and torch.equal(gl, _cut(ls, org, roi))


def test_identity_holds_for_one_axis_either_tensor_alone_lifted_sources_and_bool_labels():
    xs = [K.image((1, 2, n), 60 + i)[0] for i, n in enumerate((57, 64, 70))]
    p = _all_steps(3, 1)
    org = [(0,), (7,), (13,)]
    gi, none = ft.crop_augment_batch(xs, None, org, (57,), p)            # 1-D: composed everywhere
    assert none is None and torch.equal(gi, ft.augment_batch(_cut(xs, org, (57,)), None, p)[0])
    xs, ls = _sources(SRC3, 3, 2, 70, torch.bfloat16)
    p = _all_steps(3, 3)
    ci, cl = ft.augment_batch(_cut(xs, ORG3, ROI3), _cut(ls, ORG3, ROI3), p)
    gi, none = ft.crop_augment_batch(xs, None, ORG3, ROI3, p)
    assert none is None and gi.dtype == torch.bfloat16 and torch.equal(gi, ci)
    none, gl = ft.crop_augment_batch(None, ls, ORG3, ROI3, p)
    assert none is None and torch.equal(gl, cl)
    gi, gl = ft.crop_augment_batch([x[None] for x in xs], [l[None] for l in ls], ORG3, ROI3, p)   # (1, C, *S) sources
    assert torch.equal(gi, ci) and torch.equal(gl, cl)
    bl = [l > 1 for l in ls]
    gl = ft.crop_augment_batch(None, bl, ORG3, ROI3, p)[1]
    assert gl.dtype == torch.bool and torch.equal(gl, cl > 1)


@pytest.mark.parametrize("nd", [3, 2])
def test_crops_match_the_float64_reference(nd):
    """aug_ref.augment on host-cut crops; the bounds are those of tests/test_augment_cpu.py for the composed path: 3e-5 on
    the image, labels exact outside the voxels near a half-integer position (at least 98 % of them)"""
    shapes, org, roi, C, L = (SRC3, ORG3, ROI3, 3, 2) if nd == 3 else (SRC2, ORG2, ROI2, 2, 1)
    xs, ls = _sources(shapes, C, L, 80)
    _, A, F = K.resample_cases(nd)[0]
    B = A.shape[0]
    xs, ls, org = xs[:B], ls[:B], org[:B]
    p = ft.AugmentParams.identity(B, nd, seed=0x1234567890ABCDE)
    p.affine, p.flip = A, F
    p.noise_std = torch.tensor([0.1, 0.05, 0.0][:B])
    p.sigma = torch.tensor([[0.5, 0.75, 1.0], [1.0, 0.0, 0.6], [0.0, 0.0, 0.0]])[:B, :nd].clone()
    p.gain = torch.tensor([1.3, 0.7, 1.0][:B])
    p.offset = torch.tensor([-0.1, 0.05, 0.0][:B])
    gi, gl = ft.crop_augment_batch(xs, ls, org, roi, p)
    shape = (B, C) + roi
    ri, rl = R.augment(_cut(xs, org, roi).double().numpy(), _cut(ls, org, roi).numpy(), p.affine.double().numpy(),
                       p.flip.numpy(), p.noise_std.double().numpy(), p.sigma.double().numpy(), p.gain.double().numpy(),
                       p.offset.double().numpy(), R.noise_field(shape, p.seed))
    err = np.abs(gi.double().numpy() - ri).max()
    print("crop + composed pipeline max abs err", err)
    assert err <= 3e-5
    for b in range(B):
        ok = ~R.near_half(p.affine[b].double().numpy(), p.flip[b].tolist(), roi)
        assert ok.mean() >= 0.98
        assert np.array_equal(gl[b].numpy()[:, ok], rl[b][:, ok])


# ---- the host table ------------------------------------------------------------------------------------------------------------
def test_source_table_holds_pointers_extents_and_origins():
    xs, ls = _sources(SRC3, 3, 2, 90)
    imgs, labs, g, roi = AG._crop_sources(xs, ls, ORG3, ROI3)
    t = AG._crop_table(imgs, labs, g, roi)
    assert t.dtype == torch.int64 and t.shape == (3, AG.SRC) and AG.SRC == 8
    for b in range(3):
        assert t[b].tolist() == [xs[b].data_ptr(), ls[b].data_ptr(), *SRC3[b], *ORG3[b]]
    assert t[0, 0] == t[2, 0] and t[0, 5:].tolist() != t[2, 5:].tolist()     # one source, two boxes
    xs2, _ = _sources(SRC2, 2, 1, 91)
    imgs, labs, g, roi = AG._crop_sources(xs2, None, ORG2, ROI2)
    t2 = AG._crop_table(imgs, labs, g, roi)                                   # 2-D: lifted with extent 1, origin 0; no label
    assert t2[1].tolist() == [xs2[1].data_ptr(), 0, 1, 33, 64, 0, 0, 17]


def test_vector_eligibility_follows_origin_x_source_width_and_base_alignment():
    """every lane's first element on a 4-byte boundary: always for fp32, even origin x / source W for bf16, multiples of 4 for
    the one-byte label"""
    base = 1 << 20
    rows = [[base, base, 20, 24, 40, 0, 0, 0],          # aligned in everything
            [base, base, 20, 24, 40, 0, 0, 4],
            [base, base, 20, 24, 40, 0, 0, 12],
            [base, base, 20, 24, 40, 0, 0, 3],          # odd origin x
            [base, base, 20, 24, 40, 0, 0, 2],          # even origin x, not a multiple of 4
            [base, base, 23, 31, 33, 3, 7, 4],          # odd source W: rows start anywhere
            [base, base, 23, 31, 34, 3, 7, 4],          # even source W, not a multiple of 4
            [base + 2, base + 2, 20, 24, 40, 0, 0, 4],  # bases off by two bytes (a bf16 element)
            [base, 0, 20, 24, 40, 0, 0, 4]]             # no label
    t = torch.tensor(rows, dtype=torch.int64)
    f32 = AG.source_vector_loads(t[[0, 1, 2, 3, 4, 5, 6, 8]], (20, 24, 28), 4).tolist()
    assert f32 == [[True, True], [True, True], [True, True], [True, False], [True, False], [True, False], [True, False],
                   [True, False]]
    bf16 = AG.source_vector_loads(t, (20, 24, 28), 2).tolist()
    assert bf16 == [[True, True], [True, True], [True, True], [False, False], [True, False], [False, False], [True, False],
                    [False, False], [True, False]]
    assert not AG.source_vector_loads(t, (20, 24, 27), 4).any()               # the output side decides first


# ---- RandCropAugment -----------------------------------------------------------------------------------------------------------
def test_module_eval_is_the_centred_identity_crop():
    xs, ls = _sources(SRC3, 3, 2, 100)
    aug = ft.RandCropAugment(3, ROI3)
    aug.eval()
    gi, gl = aug(xs, ls)
    org = [tuple((n - r) // 2 for n, r in zip(s, ROI3)) for s in SRC3]
    assert org[0] == (1, 3, 2) and org[1] == (0, 0, 6)
    assert torch.equal(gi, _cut(xs, org, ROI3)) and torch.equal(gl, _cut(ls, org, ROI3))
    gi, none = aug(xs)
    assert none is None and torch.equal(gi, _cut(xs, org, ROI3))


def test_module_training_repeats_and_draws_origins_before_records():
    xs, ls = _sources(SRC3, 3, 2, 101)
    kw = dict(affine_prob=0.7, noise_prob=0.7, smooth_prob=0.7)
    aug = ft.RandCropAugment(3, ROI3, **kw)
    g = torch.Generator().manual_seed(12)
    a, b = aug(xs, ls, generator=g)
    g.manual_seed(12)
    c, d = aug(xs, ls, generator=g)
    assert torch.equal(a, c) and torch.equal(b, d) and a.shape == (3, 3) + ROI3 and not a.requires_grad
    g.manual_seed(12)
    org = ft.draw_crop_origins(SRC3, ROI3, g)                               # the origin draw comes first ...
    x, l = _cut(xs, org.tolist(), ROI3), _cut(ls, org.tolist(), ROI3)
    e, f = ft.BatchAugment(3, **kw)(x, l, generator=g)                     # ... and leaves the generator where BatchAugment
    assert torch.equal(a, e) and torch.equal(b, f)                          # draws the same records
    assert aug.kwargs == ft.BatchAugment(3, **kw).kwargs
    with pytest.raises(ValueError):
        ft.RandCropAugment(3, (20, 24))
    with pytest.raises(ValueError):
        ft.RandCropAugment(3, ROI3, sigma_range=((0.5, 1.0),))


# ---- errors --------------------------------------------------------------------------------------------------------------------
def test_argument_errors():
    xs, ls = _sources(SRC3, 3, 2, 110)
    with pytest.raises(ValueError, match="channels"):
        ft.crop_augment_batch([xs[0], xs[1][:2], xs[2]], None, ORG3, ROI3)
    with pytest.raises(ValueError, match="float64"):
        ft.crop_augment_batch([xs[0], xs[1].double(), xs[2]], None, ORG3, ROI3)
    with pytest.raises(ValueError, match="meta"):
        ft.crop_augment_batch([xs[0], xs[1].to("meta"), xs[2]], None, ORG3, ROI3)
    with pytest.raises(ValueError, match="sample 1, axis 2"):
        ft.crop_augment_batch(xs, ls, [(0, 0, 0), (0, 0, 13), (0, 0, 0)], ROI3)
    with pytest.raises(ValueError, match="sample 2, axis 0"):
        ft.crop_augment_batch(xs, ls, [(0, 0, 0), (0, 0, 0), (-1, 0, 0)], ROI3)
    with pytest.raises(ValueError, match="sample 1"):
        ft.crop_augment_batch(xs, [ls[0], ls[1][:, :, :, :39], ls[2]], ORG3, ROI3)
    with pytest.raises(ValueError):
        ft.crop_augment_batch(xs[:2], None, ORG3, ROI3)                     # two sources, three origins
    with pytest.raises(ValueError):
        ft.crop_augment_batch(xs, None, ORG3, ROI3, ft.AugmentParams.identity(2, 3))
    with pytest.raises(ValueError):
        ft.crop_augment_batch(None, None, ORG3, ROI3)
    with pytest.raises(TypeError):
        ft.crop_augment_batch(ls, None, ORG3, ROI3)                         # an integer image


# ---- host-side argument checks (ctypes, no device work) -------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    from factorizer_amd import _native, build
    build.build(verbose=False)
    return _native.lib()


P8 = ctypes.c_void_p(4096)   # a non-null, aligned pointer value the host code never dereferences
P9 = ctypes.c_void_p(8192)


def test_crop_resample_argument_checks(lib):
    assert lib.fz_aug_source_words() == AG.SRC
    ok = dict(src=P8, out=P9, dt=0, C=2, lab_out=None, L=0, table=P8, seed=None, ws=None, ns=0, B=2, nd=3, D=8, H=8, W=8)

    def call(**kw):
        a = {**ok, **kw}
        return lib.fz_aug_crop_resample(a["src"], a["out"], a["dt"], a["C"], a["lab_out"], a["L"], a["table"], a["seed"],
                                        a["ws"], a["ns"], a["B"], a["nd"], a["D"], a["H"], a["W"], None)
    assert call(src=None) == -4 and b"source table" in lib.fz_last_error_string()
    assert call(table=None) == -4 and b"table" in lib.fz_last_error_string()
    assert call(out=None) == -4 and call(L=1) == -4                                   # planes without an output
    assert call(dt=7) == -4 and b"act_dtype" in lib.fz_last_error_string()
    assert call(nd=1) == -4 and call(nd=4) == -4 and b"nd" in lib.fz_last_error_string()
    assert call(W=2049) == -1 and b"2048" in lib.fz_last_error_string()               # the ROI is limited, sources are not
    assert call(D=2049) == -1 and call(H=2049) == -1
    assert call(nd=2) == -1                                                           # D must be 1 for a 2-D roi
    assert call(C=0) == -1 and call(B=0) == -1 and call(W=0) == -1
    assert call(ns=1) == -4 and call(ns=3, ws=P8) == -4                               # slots need a workspace, ns <= B
    assert call(src=ctypes.c_void_p(4100)) == -4 and b"aligned" in lib.fz_last_error_string()   # int64 words
    assert call(out=ctypes.c_void_p(8194)) == -4
    n0 = lib.fz_launch_count()
    assert call(src=None) == -4 and lib.fz_launch_count() == n0
