"""ft.prepare_volume / ft.restore_prediction on CPU tensors (the composed path) against the independent float64 reference
tests/vol_prep_ref.py, the semantics table row by row, the round trip, and the host-side argument checks of the new entry
points (no GPU needed)."""
import ctypes

import pytest
import torch

import factorizer_amd as ft
import vol_prep_ref as R

U8, I16, F32, BF16 = torch.uint8, torch.int16, torch.float32, torch.bfloat16


check_prepared, check_label = R.check_prepared, R.check_label


@pytest.mark.parametrize("name", sorted(R.CASES))
def test_composed_path_equals_the_reference(name):
    x, kw = R.make_case(name)
    lab = R.class_map(x.shape[1:], 1)
    got = ft.prepare_volume(x, lab, classes=R.BRATS_CLASSES, **kw)
    ref = R.prepare(x, lab, classes=R.BRATS_CLASSES, **kw)
    check_prepared(got, ref)
    check_label(got, ref)
    s, e = ft.foreground_bbox(x, kw["margin"], kw.get("allow_smaller", True))
    assert (s, e) == (ref["start"], ref["end"]) and all(isinstance(v, int) for v in s + e)


def test_semantics_rows_say_what_they_claim():
    """the properties each table row is named after, read off the results (not only equality with the reference)"""
    x, kw = R.make_case("margin_clipped")
    p = ft.prepare_volume(x, **kw)
    assert p.box_start == (0, 5, 2) and p.box_end == (16, 26, 16)            # clipped at 0 and at 26, free elsewhere
    x, kw = R.make_case("margin_outside")
    p = ft.prepare_volume(x, **kw)
    assert p.box_start == (-2, 5, 2) and p.box_end == (16, 28, 16)
    assert (p.image[0, :, :2] == 0).all() and (p.image[0, :, :, 21:] == 0).all()   # the crop zero-fills outside the image
    x, kw = R.make_case("margin_outside_all")
    p = ft.prepare_volume(x, **kw)                                            # nonzero=False rewrites those zeros too
    assert p.pad_before == (0, 0, 1)                                          # [0, 0, 1] is a box voxel outside the image
    assert torch.equal(p.image[0, :, 0, 0, 1], (0 - p.mean) / p.std) and (p.image[0, :, 0, 0, 1] != 0).all()
    x, kw = R.make_case("no_foreground")
    p = ft.prepare_volume(x, **kw)
    assert p.box_start == (0, 0, 0) and p.box_end == tuple(x.shape[1:]) and (x <= 0).all()
    x, kw = R.make_case("constant_channel")
    p = ft.prepare_volume(x, **kw)
    assert p.std[1] == 1.0 and p.mean[1] == x[1].max() and (p.image[0, 1] == 0).all()
    x, kw = R.make_case("zero_channel")
    p = ft.prepare_volume(x, **kw)
    assert p.std[2] == 1.0 and p.mean[2] == 0.0 and (p.image[0, 2] == 0).all()
    x, kw = R.make_case("negatives_outside_box")
    p = ft.prepare_volume(x, **kw)
    inside = x[:, 7:14, 9:17, 6:13]
    assert (x < 0).any() and (inside >= 0).all()                              # ... and none of them is in the box
    q = ft.prepare_volume(torch.where(x < 0, torch.zeros_like(x), x), **kw)
    assert torch.equal(p.mean, q.mean) and torch.equal(p.std, q.std) and torch.equal(p.image, q.image)
    x, kw = R.make_case("negatives_inside_box")
    p = ft.prepare_volume(x, **kw)
    q = ft.prepare_volume(torch.where(x < 0, torch.zeros_like(x), x), **kw)
    assert p.box_start == q.box_start and not torch.equal(p.mean, q.mean)     # the negatives of the box enter the statistics
    x, kw = R.make_case("odd_pads")
    p = ft.prepare_volume(x, **kw)
    widths = [r - (e - s) for r, s, e in zip((20, 24, 17), p.box_start, p.box_end)]
    assert widths == [7, 9, 9] and p.pad_before == (3, 4, 4)                  # w // 2 in front, the larger half behind
    x, kw = R.make_case("no_roi")
    p = ft.prepare_volume(x, **kw)
    assert p.pad_before == (0, 0, 0) and tuple(p.image.shape[2:]) == tuple(e - s for s, e in zip(p.box_start, p.box_end))
    x, kw = R.make_case("whole_tensor")
    p = ft.prepare_volume(x, **kw)
    assert (p.mean == p.mean[0]).all() and (p.std == p.std[0]).all()


@pytest.mark.parametrize("dtype", [F32, I16])
def test_normalize_intensity_alone(dtype):
    x = R.volume((3, 9, 12, 10), ((1, 8), (2, 11), (0, 9)), 21, dtype=dtype, neg_inside=True)
    for nonzero in (True, False):
        for cw in (True, False):
            got = ft.normalize_intensity(x, nonzero, cw)
            mean, std, sel = R.stats(x, nonzero, cw)
            view = (-1, 1, 1, 1)
            m64, s64 = torch.tensor(mean, dtype=torch.float64).view(view), torch.tensor(std, dtype=torch.float64).view(view)
            want = torch.where(sel, (x.double() - m64) / s64, x.double())
            bound = 2.0 ** -22 * (x.double().abs() + m64.abs()) / s64       # the bound of check_prepared
            assert got.dtype == F32 and ((got.double() - want).abs() <= bound).all()
            assert torch.equal(got == 0, x == 0) or not nonzero               # zeros stay zeros
    b = torch.stack([x, x.flip(1)])
    assert torch.equal(ft.normalize_intensity(b)[1], ft.normalize_intensity(x.flip(1)))


def test_native_gate_names_its_reason():
    """device calls the kernels do not take are composed with a warning that says why; CPU calls silently"""
    import warnings
    from factorizer_amd import composed, volume as V
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        assert V._native_gate("t", False, True, [F32], 1, [8]) is False
        assert V._native_gate("t", True, True, [F32], V.MAX_CHANNELS, [V.MAX_PLANE - 1]) is True
    for key, args, word in (("torch.float16", (False, [torch.float16], 1, [8]), "outside the native kernel set"),
                            ("channels", (True, [F32], V.MAX_CHANNELS + 1, [8]), "channels"),
                            ("plane", (True, [F32], 1, [8, V.MAX_PLANE]), "voxels"),
                            ("other", (True, [F32], 1, [8], "a reason in words"), "a reason in words")):
        composed._warned.discard("volume:t:" + key)
        with pytest.warns(RuntimeWarning, match=word) as rec:
            assert V._native_gate("t", True, *args) is False
            assert V._native_gate("t", True, *args) is False
        assert len(rec) == 1


def test_label_forms():
    x, kw = R.make_case("odd_pads")
    lab = R.class_map(x.shape[1:], 3, dtype=I16, top=6)
    two = ((1, 4), (0, 2, 5))
    for classes in (R.BRATS_CLASSES, two):
        for l in (lab, lab[None], lab.to(U8)):
            got = ft.prepare_volume(x, l, classes=classes, **kw)
            check_label(got, R.prepare(x, lab, classes=classes, **kw))
    assert ft.BRATS_CLASSES == R.BRATS_CLASSES and ft.BRATS_LABEL_VALUES == R.BRATS_LABEL_VALUES
    ready = R.encode(lab, two)                                               # already channel-first: cropped and padded as it is
    check_label(ft.prepare_volume(x, ready, **kw), R.prepare(x, ready, **kw))
    with pytest.raises(ValueError):
        ft.prepare_volume(x, lab, classes=((32,),), **kw)
    with pytest.raises(ValueError):
        ft.prepare_volume(x, lab, classes=((1,),) * 9, **kw)
    with pytest.raises(ValueError):
        ft.prepare_volume(torch.zeros(1, 2, 2, 2, 2, 2))


@pytest.mark.parametrize("name", ["margin_clipped", "margin_outside", "odd_pads", "no_roi", "2d", "1d_padded"])
@pytest.mark.parametrize("K", [1, 3])
def test_restore_equals_the_reference(name, K):
    x, kw = R.make_case(name)
    p = ft.prepare_volume(x, **kw)
    shape = (3,) + tuple(p.image.shape[2:])
    ls = R.logits_for(shape, K, 31, F32, threshold=0.3)
    assert ((R.ensemble64(ls) - R.bound64(0.3)).abs() > 1e-3).all()
    geo = dict(box_start=p.box_start, box_end=p.box_end, pad_before=p.pad_before, orig_size=p.orig_size)
    args = (p.box_start, p.box_end, p.pad_before, p.orig_size)
    mask = ft.restore_prediction(ls if K > 1 else ls[0], p, threshold=0.3)
    assert mask.dtype == U8 and torch.equal(mask, R.restore(ls, *args, threshold=0.3))
    lm = ft.restore_prediction(ls, geo, threshold=0.3, label_values=(7, 200, 9))
    assert lm.dtype == U8 and torch.equal(lm, R.restore(ls, *args, threshold=0.3, label_values=(7, 200, 9)))


def test_label_values_priority():
    """where several channels fire the first in channel order writes; where none does the voxel is 0"""
    geo = dict(box_start=(0, 0), box_end=(2, 4), pad_before=(0, 0), orig_size=(2, 4))
    z = torch.tensor([[[-1., 1, -1, 1], [-1, -1, 1, 1]],      # channel 0
                      [[-1., 1, 1, -1], [1, -1, 1, 1]],       # channel 1
                      [[-1., 1, 1, 1], [1, 1, -1, 1]]])[None]
    lm = ft.restore_prediction(z, geo, label_values=ft.BRATS_LABEL_VALUES)
    assert lm.tolist() == [[0, 3, 1, 3], [1, 2, 3, 3]]
    assert torch.equal(lm, R.restore([z], (0, 0), (2, 4), (0, 0), (2, 4), label_values=R.BRATS_LABEL_VALUES))
    with pytest.raises(ValueError):
        ft.restore_prediction([z] * 9, geo)


def test_round_trip_reproduces_the_class_map_inside_the_box():
    x, kw = R.make_case("3d_mixed_pad")
    g = torch.Generator().manual_seed(5)
    # nested BraTS regions, so that the three channels determine the class: 0 outside, 2 (ED) ⊃ 1 (NCR) ⊃ 3 (ET)
    lab = torch.zeros(x.shape[1:], dtype=U8)
    r = torch.rand(x.shape[1:], generator=g)
    lab[r < 0.6] = 2
    lab[r < 0.4] = 1
    lab[r < 0.2] = 3
    p = ft.prepare_volume(x, lab, classes=ft.BRATS_CLASSES, **kw)
    ls = R.logits_for(tuple(p.label.shape[1:]), 3, 41, F32, target=p.label[0] != 0)
    out = ft.restore_prediction(ls, p, label_values=ft.BRATS_LABEL_VALUES)
    box = tuple(slice(max(s, 0), min(e, n)) for s, e, n in zip(p.box_start, p.box_end, p.orig_size))
    inside = torch.zeros_like(lab, dtype=torch.bool)
    inside[box] = True
    assert torch.equal(out[box], lab[box]) and (out[~inside] == 0).all() and (lab[~inside] != 0).any()


def test_host_side_argument_checks_of_the_volume_entry_points():
    """the new entry points refuse bad arguments with FZ_E_ARG and a message before touching the device"""
    from factorizer_amd import _native
    from factorizer_amd import functional as Fn
    lib = _native.lib()
    assert lib.fz_abi_version() == 7
    E_ARG = -4
    p8 = ctypes.c_void_p(8)   # a non-null pointer value the host code never dereferences
    ok = Fn.vol_geom((8, 8, 8), (1, 1, 1), (7, 7, 7), (1, 1, 1), (8, 8, 8))
    assert lib.fz_vol_workspace_bytes(2, ctypes.byref(ok)) == 2 * 3 * 8
    # more than three spatial axes
    assert lib.fz_vol_bbox(p8, _native.VOL_F32, 1, 4, 8, 8, 8, p8, None) == E_ARG and b"nd" in lib.fz_last_error_string()
    g4 = Fn.vol_geom((8, 8, 8), (1, 1, 1), (7, 7, 7), (1, 1, 1), (8, 8, 8))
    g4.nd = 4
    assert lib.fz_vol_stats(p8, _native.VOL_F32, 1, ctypes.byref(g4), 1, 1, p8, None) == E_ARG
    assert b"nd" in lib.fz_last_error_string()
    # K > 8: logit tensors and class sets
    table = (ctypes.c_void_p * 9)(*[8] * 9)
    assert lib.fz_vol_restore(table, 9, _native.VOL_F32, 3, ctypes.byref(ok), 0.0, None, p8, None) == E_ARG
    assert b"K" in lib.fz_last_error_string()
    ids, cnt = (ctypes.c_int * 9)(*range(9)), (ctypes.c_int * 9)(*[1] * 9)

    def write(geom, ids, cnt, n):
        return lib.fz_vol_write(p8, _native.VOL_F32, p8, _native.VOL_F32, 1, p8, _native.VOL_U8, 0, ids, cnt, n, p8,
                                ctypes.byref(geom), 1, 1, p8, p8, p8, None)

    assert write(ok, ids, cnt, 9) == E_ARG and b"class sets" in lib.fz_last_error_string()
    # class id >= 32
    ids[2] = 32
    assert write(ok, ids, cnt, 3) == E_ARG and b"class id" in lib.fz_last_error_string()
    # a box inconsistent with the sizes: pad + box beyond the prepared extent, empty, outside the image, a lifted axis in use
    for bad, word in ((Fn.vol_geom((8, 8, 8), (1, 1, 1), (7, 7, 7), (3, 1, 1), (8, 8, 8)), b"exceeds"),
                      (Fn.vol_geom((8, 8, 8), (1, 4, 1), (7, 4, 7), (0, 0, 0), (8, 8, 8)), b"empty"),
                      (Fn.vol_geom((8, 8, 8), (1, 1, 9), (7, 7, 12), (0, 0, 0), (8, 8, 8)), b"no voxel"),
                      (Fn.vol_geom((8, 8), (1, 1), (7, 7), (0, 0), (8, 8)), b"lifted")):
        if word == b"lifted":
            bad.size[0] = 2
        assert lib.fz_vol_workspace_bytes(1, ctypes.byref(bad)) == -1
        for rc in (lib.fz_vol_stats(p8, _native.VOL_F32, 1, ctypes.byref(bad), 1, 1, p8, None), write(bad, ids, cnt, 0),
                   lib.fz_vol_restore(table, 2, _native.VOL_F32, 3, ctypes.byref(bad), 0.0, None, p8, None)):
            assert rc == E_ARG and word in lib.fz_last_error_string(), lib.fz_last_error_string()
    # element kinds per role
    assert [lib.fz_vol_kind_ok(_native.VOL_IMAGE_IN, k) for k in range(5)] == [1, 0, 0, 1, 0]
    assert [lib.fz_vol_kind_ok(_native.VOL_IMAGE_OUT, k) for k in range(5)] == [1, 1, 0, 0, 0]
    assert [lib.fz_vol_kind_ok(_native.VOL_LABEL_IN, k) for k in range(5)] == [0, 0, 1, 1, 0]
    assert [lib.fz_vol_kind_ok(_native.VOL_LOGITS, k) for k in range(5)] == [1, 1, 0, 0, 0]
    assert lib.fz_vol_stats(p8, _native.VOL_BF16, 1, ctypes.byref(ok), 1, 1, p8, None) == E_ARG
    assert lib.fz_vol_restore(table, 2, _native.VOL_U8, 3, ctypes.byref(ok), 0.0, None, p8, None) == E_ARG
