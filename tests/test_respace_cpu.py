"""ft.spacing_geometry / ft.resample_volume / ft.restore_spaced_prediction on CPU tensors (the composed path): the geometry
invariants, the shape rule, the values against the independent float64 reference tests/respace_ref.py and against
scipy.ndimage.map_coordinates, the round trip, and the argument checks (no GPU needed).

Value bounds (derived, shared with tests/test_gpu_respace.py): positions are float64 on every path, so a bilinear value
differs from the float64 reference by three nested fp32 lerps of three roundings each plus the fp32 rounding of the weight
against a neighbour difference of at most 2·max|v| per axis — about 15 · 2^-24 ≈ 9e-7, doubled: 2e-6 · max|v| absolute.  The
probability path adds the fp32 sigmoid: 4e-6."""
import ctypes

import numpy as np
import pytest
import torch

import factorizer_amd as ft
import respace_ref as R

F32, BF16, U8 = torch.float32, torch.bfloat16, torch.uint8
IMG_BOUND, PROB_BOUND = 2e-6, 4e-6


def geometry_of(name):
    x, lab, A, kw = R.make_case(name)
    g = ft.spacing_geometry(x.shape[1:], A, kw["pixdim"], roi_size=kw["roi"], box_start=kw.get("box_start"),
                            orig_size=kw.get("orig_size"))
    return x, lab, A, kw, g, R.geometry(x.shape[1:], A, **kw)


def source_position(g, o):
    """the position, on the file's grid, that unpadded output index o reads"""
    p = [0.0] * len(o)
    for w, a in enumerate(g.src_axis):
        p[a] = g.scale[w] * o[w] + g.offset[w] + g.box_start[a]
    return p


# ---- geometry invariants -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("box", [None, (2, 0, 3)])
def test_every_signed_permutation_keeps_the_world_point(box):
    """dst_affine·[o; 1] is the world point of the source position each output voxel reads, through crop → orient → space"""
    size = (7, 5, 6)
    for k, code in enumerate(R.all_codes()):
        A = R.make_affine(code, (0.9, 1.2, 5.0), deg=20.0 * ((k % 5) - 2) / 2)
        assert ft.orientation_of(A) == code == R.code_of(A)
        g = ft.spacing_geometry(size, A, (2.0, 1.5, 2.5), box_start=box)
        assert sorted(g.src_axis) == [0, 1, 2] and g.dst_affine.dtype == torch.float64
        D = g.dst_affine.numpy()
        for o in ((0, 0, 0), (1, 0, 0), (0, 2, 0), (0, 0, 3), tuple(n - 1 for n in g.res_size)):
            world = D @ np.array(list(o) + [1.0])
            want = A @ np.array(source_position(g, o) + [1.0])
            assert np.abs(world - want).max() <= 1e-9, (code, o)
        M = D[:3, :3]
        assert all(M[w, w] > 0 and abs(M[w, w]) == np.abs(M[:, w]).max() for w in range(3))    # "RAS": positive dominant diagonal
        assert ft.orientation_of(D) == "RAS"
        ref = R.geometry(size, A, (2.0, 1.5, 2.5), box_start=box)
        assert list(g.src_axis) == ref["perm"] and list(g.flip) == ref["flip"] and list(g.res_size) == ref["res"]
        assert np.abs(D - ref["affine"]).max() <= 1e-12


def test_other_axis_codes_and_lower_dimensions():
    A = R.make_affine("RAS", (1.0, 2.0, 3.0), deg=10)
    g = ft.spacing_geometry((4, 5, 6), A, None, axcodes="LPS")
    assert g.src_axis == (0, 1, 2) and g.flip == (True, True, False) and g.res_size == (4, 5, 6)
    assert ft.orientation_of(g.dst_affine) == "LPS"
    g = ft.spacing_geometry((4, 5, 6), A, None, axcodes="SRA")
    assert g.src_axis == (2, 0, 1) and g.flip == (False,) * 3 and ft.orientation_of(g.dst_affine) == "SRA"
    g = ft.spacing_geometry((4, 5, 6), R.make_affine("PIR", (1, 1, 1)), 2.0, axcodes=None)      # no reorientation
    assert g.src_axis == (0, 1, 2) and g.flip == (False,) * 3 and ft.orientation_of(g.dst_affine) == "PIR"
    A2 = R.make_affine("AL", (3.0, 0.9), deg=5)
    assert ft.orientation_of(A2) == "AL" and ft.orientation_of(A2, 2) == "AL"
    g = ft.spacing_geometry((13, 18), A2, 2.0)                                                 # "RAS" names the first two axes
    assert g.src_axis == (1, 0) and g.flip == (True, False)
    assert ft.spacing_geometry((13, 18), A2, 2.0, axcodes="RA").res_size == g.res_size
    g = ft.spacing_geometry((17,), R.make_affine("L", (3.0,)), 2.0, axcodes="R")
    assert g.src_axis == (0,) and g.flip == (True,) and g.res_size == (25,)


# ---- shapes ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,zoom,pix,want", [(10, 1.0, 2.0, 6), (1, 1.0, 2.0, 1), (1, 3.0, 2.0, 1), (14, 3.0, 2.0, 20),
                                             (12, 3.0, 2.0, 18), (4, 1.0, 2.0, 2), (6, 1.0, 2.0, 4), (17, 3.0, 2.0, 25),
                                             (9, 1.0, 1.0, 9)])
def test_output_extent_rounds_half_to_even(n, zoom, pix, want):
    """n_out = round_half_even((n − 1)·zoom / pixdim + 1): 14 → 20.5 → 20, 12 → 17.5 → 18, 4 → 2.5 → 2, 6 → 3.5 → 4"""
    g = ft.spacing_geometry((n,), [[zoom, 0.0], [0.0, 1.0]], pix, axcodes=None)
    assert g.res_size == (want,) == (R.half_even((n - 1) * zoom / pix + 1),)
    assert want == max(1, round((n - 1) * zoom / pix + 1))
    if n == 10:                                             # the last voxel reads position 10 and clamps to 9
        x = torch.arange(10, dtype=F32)[None]
        out, _ = ft.resample_volume(x, g)
        assert g.scale[0] * (want - 1) == 10.0 and out[0].tolist() == [0.0, 2.0, 4.0, 6.0, 8.0, 9.0]
        lab, _ = ft.resample_volume(x, g, mode="nearest")
        assert lab[0].tolist() == [0.0, 2.0, 4.0, 6.0, 8.0, 9.0]


def test_pad_is_symmetric_with_the_smaller_half_in_front():
    _, _, _, _, g, ref = geometry_of("grow_transposed_mirror")
    assert g.res_size == (20, 13, 16) and g.out_size == (20, 18, 16) and g.pad_before == (0, 2, 0)   # one axis, odd pad 5
    assert list(g.pad_before) == ref["pad"] and list(g.out_size) == ref["out"]


# ---- values ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(R.CASES))
def test_composed_path_equals_the_reference_and_scipy(name):
    from scipy.ndimage import map_coordinates
    x, lab, A, kw, g, ref = geometry_of(name)
    assert list(g.res_size) == ref["res"] and list(g.out_size) == ref["out"] and list(g.pad_before) == ref["pad"]
    img, lout = ft.resample_volume(torch.from_numpy(x), g, label=torch.from_numpy(lab))
    want = R.forward(x, ref)
    assert img.dtype == F32 and tuple(img.shape) == want.shape
    err = np.abs(img.numpy().astype(np.float64) - want).max()
    print(name, "bilinear max abs err", err, "bound", IMG_BOUND * np.abs(x).max())
    assert err <= IMG_BOUND * np.abs(x).max()
    # scipy: order 1 with mode "nearest" is bilinear with border clamping
    xo = R._oriented(x, ref).astype(np.float64)
    pos = np.meshgrid(*[np.arange(n) * (p / z) for n, p, z in zip(ref["res"], ref["pix"], ref["zoom"])], indexing="ij")
    inner = (slice(None),) + tuple(slice(b, b + n) for b, n in zip(ref["pad"], ref["res"]))
    for c in range(x.shape[0]):
        sp = map_coordinates(xo[c], pos, order=1, mode="nearest")
        assert np.abs(sp - want[inner][c]).max() <= 1e-9 * np.abs(x).max()
    # nearest label: exact, and these inputs have no position within 1e-9 of a tie on a non-dyadic scale
    assert not R.near_ties(ref).any()
    assert lout.dtype == U8 and np.array_equal(lout.numpy(), R.forward(lab, ref, "nearest"))
    near, _ = ft.resample_volume(torch.from_numpy(x), g, mode="nearest")
    assert np.array_equal(near.numpy(), R.forward(x, ref, "nearest"))
    # bf16: the fp32 value rounded to nearest even
    half, _ = ft.resample_volume(torch.from_numpy(x), g, out_dtype=BF16)
    assert half.dtype == BF16 and torch.equal(half, img.to(BF16))


def test_half_ties_round_to_even():
    x, lab, A, kw, g, ref = geometry_of("half_ties")
    assert abs(g.scale[0]) == 0.5 and abs(g.scale[1]) == 0.5
    p = R.forward_positions(ref)[0]
    assert (p[1::2] % 1 == 0.5).sum() >= 4                                   # exact ties are there
    assert R.table(ref["res"][0], 0.5, 9)[4][:6].tolist() == [0, 0, 1, 2, 2, 2]   # 0.5 → 0, 1.5 → 2, 2.5 → 2


@pytest.mark.parametrize("size,roi", [((2, 5, 6, 8), None), ((2, 5, 6, 7), (5, 8, 10))])
def test_the_identity_map_is_bit_identical_to_indexing(size, roi):
    g0 = torch.Generator().manual_seed(1)
    x = torch.randn(size, generator=g0)
    x[0, 1, 2, 3] = float("inf")                             # an interpolation would turn its neighbours into NaN
    lab = torch.randint(0, 255, size, generator=g0).to(U8)
    g = ft.spacing_geometry(size[1:], np.eye(4), 1.0, roi_size=roi)
    assert all(s == 1.0 for s in g.scale) and g.offset == (0.0,) * 3
    img, lout = ft.resample_volume(x, g, label=lab)
    inner = (slice(None),) + tuple(slice(b, b + n) for b, n in zip(g.pad_before, size[1:]))
    assert torch.equal(img[inner], x) and torch.equal(lout[inner], lab)
    assert img.isinf().sum() == 1 and not img.isnan().any() and img.numel() - x.numel() == (img == 0).sum() - (x == 0).sum()
    # mirrored and permuted at unit scale: still a copy
    A = R.make_affine("PIR", (1, 1, 1))
    g = ft.spacing_geometry(size[1:], A, 1.0)
    img, _ = ft.resample_volume(x, g)
    assert torch.equal(img, x.permute(0, 3, 1, 2).flip(2, 3))


# ---- inverse ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(R.CASES))
@pytest.mark.parametrize("K,dtype", [(1, F32), (5, F32), (5, BF16)])
def test_restore_equals_the_reference(name, K, dtype):
    x, lab, A, kw, g, ref = geometry_of(name)
    ls = [torch.from_numpy(l).to(dtype) for l in R.make_logits(3, ref["out"], K)]
    want = R.inverse([l.float().numpy() for l in ls], ref)
    arg = [l[None] for l in ls] if K > 1 else ls[0][None]
    prob = ft.restore_spaced_prediction(arg, g, threshold=None)
    assert prob.dtype == F32 and tuple(prob.shape) == (3,) + tuple(ref["orig"])
    err = np.abs(prob.numpy() - want).max()
    print(name, K, dtype, "probability max abs err", err)
    assert err <= PROB_BOUND
    mask = ft.restore_spaced_prediction(arg, g, threshold=0.3)
    sure = np.abs(want - 0.3) > 1e-5
    assert mask.dtype == U8 and (~sure).mean() <= 1e-3
    assert np.array_equal(mask.numpy()[sure], (want >= 0.3)[sure])
    raw = ft.restore_spaced_prediction(arg, g, sigmoid=False, threshold=None)
    want_raw = R.inverse([l.float().numpy() for l in ls], ref, use_sigmoid=False)
    # without the sigmoid the K − 1 fp32 additions and the 1 / K product show: each within 2^-24 of a partial sum <= M
    M = sum(np.abs(l.float().numpy()).max() for l in ls)
    assert np.abs(raw.numpy() - want_raw).max() <= (IMG_BOUND + K * 2.0 ** -24) * M
    if kw.get("box_start"):
        outside = np.ones(ref["orig"], dtype=bool)
        outside[tuple(slice(s, s + n) for s, n in zip(ref["start"], ref["size"]))] = False
        assert outside.any() and (prob.numpy()[:, outside] == 0).all() and (mask.numpy()[:, outside] == 0).all()


@pytest.mark.parametrize("name", ["grow_transposed_mirror", "mixed_cyclic_two_mirrors", "boxed", "2d", "1d"])
def test_round_trip_of_a_field_linear_in_world_coordinates(name):
    """resampling a world-linear field forth and back reproduces it inside the box to 1e-5, voxels whose forward or inverse
    position was clamped left out (bilinear interpolation is exact on linear fields)"""
    x, lab, A, kw, g, ref = geometry_of(name)
    nd = len(g.src_size)
    coef = np.array([0.013, -0.021, 0.008][:nd])
    idx = np.stack(np.meshgrid(*[np.arange(n) for n in g.orig_size], indexing="ij"), -1).astype(np.float64)
    world = idx @ A[:nd, :nd].T + A[:nd, nd]
    field = world @ coef + 0.5                                               # (*orig)
    box = tuple(slice(s, s + n) for s, n in zip(g.box_start, g.src_size))
    src = torch.from_numpy(field[box][None].astype(np.float32))
    fwd, _ = ft.resample_volume(src, g)
    back = ft.restore_spaced_prediction(fwd[None], g, sigmoid=False, threshold=None)[0].numpy()
    keep = R.unclamped(ref)
    assert keep.mean() > 0.5
    err = np.abs(back[box] - field[box])[keep].max()
    print(name, "round trip max abs err", err)
    assert err <= 1e-5
    outside = np.ones(g.orig_size, dtype=bool)
    outside[box] = False
    assert (back[outside] == 0).all()


def test_prepare_spaced_volume_is_the_chain():
    x, lab, A, kw = R.make_case("boxed")
    vol = np.zeros((2, 12, 20, 15), dtype=np.float32)
    vol[:, 3:9, 5:14, 4:10] = np.abs(x[:, :6, :9, :6]) + 0.1
    cls = np.zeros((12, 20, 15), dtype=np.uint8)
    cls[4:8, 6:12, 5:9] = 1
    v, c = torch.from_numpy(vol), torch.from_numpy(cls)
    got = ft.prepare_spaced_volume(v, A, c, pixdim=2.0, margin=1, roi_size=(24, 8, 8), classes=((1,),))
    p = ft.prepare_volume(v, c, margin=1, classes=((1,),))
    assert got.box_start == p.box_start == (2, 4, 3) and got.box_end == p.box_end and got.orig_size == (12, 20, 15)
    assert torch.equal(got.mean, p.mean) and torch.equal(got.std, p.std)
    g = ft.spacing_geometry((8, 11, 8), A, 2.0, box_start=(2, 4, 3), roi_size=(24, 8, 8), orig_size=(12, 20, 15))
    img, lout = ft.resample_volume(p.image[0], g, label=p.label[0])
    assert torch.equal(got.image[0], img) and torch.equal(got.label[0], lout) and got.pad_before == g.pad_before
    assert got.geometry.res_size == g.res_size and torch.equal(got.geometry.dst_affine, g.dst_affine)
    ref = R.geometry((8, 11, 8), A, 2.0, box_start=(2, 4, 3), roi=(24, 8, 8), orig_size=(12, 20, 15))
    assert np.array_equal(lout.numpy(), R.forward(p.label[0].numpy(), ref, "nearest"))
    mask = ft.restore_spaced_prediction(20.0 * got.label.float() - 10.0, got)
    assert mask.shape == (1, 12, 20, 15) and mask.dtype == U8 and mask.sum() > 0
    assert (mask[0][torch.from_numpy(cls) == 0].float().mean()) < 0.25       # the prediction comes back where the class was


# ---- argument errors ---------------------------------------------------------------------------------------------------------------
def test_argument_errors():
    A = np.eye(4)
    for pix in (0.0, -1.0, (2.0, 0.0, 2.0), float("nan"), (2.0, 2.0)):
        with pytest.raises(ValueError):
            ft.spacing_geometry((4, 5, 6), A, pix)
    for bad in (np.eye(3), np.zeros((4, 3)), np.eye(5), np.zeros(4)):
        with pytest.raises(ValueError):
            ft.spacing_geometry((4, 5, 6), bad, 2.0)
    with pytest.raises(ValueError):
        ft.orientation_of(np.zeros((2, 3)))
    for code in ("RAX", "RRS", "RA", "RAL", 7 * "R"):
        with pytest.raises(ValueError):
            ft.spacing_geometry((4, 5, 6), A, 2.0, axcodes=code)
    with pytest.raises(ValueError):
        ft.spacing_geometry((4, 5), np.eye(3), 2.0, axcodes="RS")            # a 2-D grid names the first two world axes
    g = ft.spacing_geometry((4, 5, 6), A, 2.0)
    x = torch.zeros(1, 4, 5, 6)
    with pytest.raises(ValueError):
        ft.resample_volume(x, g, mode="cubic")
    with pytest.raises(ValueError):
        ft.resample_volume(torch.zeros(1, 4, 5, 7), g)
    with pytest.raises(ValueError):
        ft.resample_volume(x, g, label=torch.zeros(1, 4, 5, 6))              # labels are uint8
    with pytest.raises(ValueError):
        ft.resample_volume(x.to(torch.int16), g)
    z = torch.zeros((1, 2) + g.out_size)
    with pytest.raises(ValueError):
        ft.restore_spaced_prediction([z] * 9, g)
    with pytest.raises(ValueError):
        ft.restore_spaced_prediction([], g)
    with pytest.raises(ValueError):
        ft.restore_spaced_prediction(torch.zeros(1, 2, 4, 5, 6), g)
    with pytest.raises(ValueError):
        ft.restore_spaced_prediction([z, z.double()], g)


def test_host_side_argument_checks_of_the_entry_points():
    """fz_vol_respace / fz_vol_unspace refuse bad arguments with a message before touching the device"""
    from factorizer_amd import _native
    lib = _native.lib()
    E_ARG, E_SHAPE = -4, -1
    p8 = ctypes.c_void_p(8)
    g = ft.spacing_geometry((4, 5, 6), R.make_affine("PIR", (1, 3, 1)), 2.0, roi_size=(8, 8, 8))

    def respace(geom, C=1, L=0, kind=_native.VOL_F32, mode=0):
        return lib.fz_vol_respace(p8, C, p8, kind, p8, L, p8, ctypes.byref(geom), mode, None)

    table = (ctypes.c_void_p * 9)(*[8] * 9)

    def unspace(geom, K=2, kind=_native.VOL_F32):
        return lib.fz_vol_unspace(table, K, kind, 3, ctypes.byref(geom), 1, 1, 0.5, p8, None)

    assert unspace(g.native(), K=9) == E_ARG and b"K" in lib.fz_last_error_string()
    assert unspace(g.native(), kind=_native.VOL_U8) == E_ARG
    assert respace(g.native(), kind=_native.VOL_U8) == E_ARG and respace(g.native(), mode=2) == E_ARG
    assert respace(g.native(), C=65535, L=1) == E_SHAPE and respace(g.native(), C=0) == E_SHAPE
    for field, index, value, word in (("src_axis", 1, 2, b"permutation"), ("pad", 0, 7, b"exceeds"), ("res_size", 2, 0, b"positive"),
                                      ("scale", 1, 0.0, b"scales"), ("inv_scale", 2, float("inf"), b"scales"),
                                      ("scale", 0, float("nan"), b"scales"), ("box_start", 0, (1 << 30) + 1, b"box")):
        bad = g.native()
        getattr(bad, field)[index] = value
        for rc in (respace(bad), unspace(bad)):
            assert rc == E_ARG and word in lib.fz_last_error_string(), (field, lib.fz_last_error_string())
    bad = g.native()
    bad.nd = 4
    assert respace(bad) == E_ARG and b"nd" in lib.fz_last_error_string()
    two = ft.spacing_geometry((5, 6), np.eye(3), 2.0).native()
    two.src_size[0] = 2
    assert respace(two) == E_ARG and b"lifted" in lib.fz_last_error_string()
