"""-m gpu: the resampling kernels (csrc/respace.hip) against the independent float64 reference tests/respace_ref.py.

Pass conditions (derived, not measured).  Positions are float64 on the device, so a bilinear value differs from the float64
reference by three nested fp32 lerps of three roundings each plus the fp32 rounding of the weight against a neighbour
difference of at most 2·max|v| per axis: about 15 · 2^-24 ≈ 9e-7, doubled — 2e-6 · max|v| absolute.  The probability path
adds the fp32 sigmoid: 4e-6.  bf16 outputs equal the reference's fp32 value rounded the same way, 1 bf16 ulp allowed where
the fp32 values differ.  Nearest labels are exactly equal except at positions within 1e-9 of a half-integer on an axis whose
scale is no dyadic rational (at most 0.1 % of the voxels; none for these inputs); thresholded masks are exactly equal except
where the float64 probability is within 1e-5 of the threshold (at most 0.1 %).  Two runs are bitwise equal."""
import ctypes
import warnings

import numpy as np
import pytest
import torch

import factorizer_amd as ft
from factorizer_amd import _native
import respace_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F32, BF16, U8 = torch.float32, torch.bfloat16, torch.uint8
IMG_BOUND, PROB_BOUND = 2e-6, 4e-6


class Launches:
    """Asserts that the native library launched kernels inside the block and that nothing was composed."""

    def __enter__(self):
        self.n0 = _native.launch_count()
        self.w = warnings.catch_warnings()
        self.w.__enter__()
        warnings.simplefilter("error")
        return self

    def __exit__(self, *a):
        self.w.__exit__(*a)
        torch.cuda.synchronize()
        assert a[0] is not None or _native.launch_count() > self.n0, "native kernels were not launched"


def _bits(t):
    return t.view(torch.int16) if t.dtype == BF16 else (t.view(torch.int32) if t.dtype == F32 else t)


_cache = {}


def case(name):
    """the case's inputs, geometries and float64 references, computed once"""
    if name not in _cache:
        x, lab, A, kw = R.make_case(name)
        g = ft.spacing_geometry(x.shape[1:], A, kw["pixdim"], roi_size=kw["roi"], box_start=kw.get("box_start"),
                                orig_size=kw.get("orig_size"))
        ref = R.geometry(x.shape[1:], A, **kw)
        _cache[name] = dict(x=x, lab=lab, g=g, ref=ref, image=R.forward(x, ref), label=R.forward(lab, ref, "nearest"),
                            nearest=R.forward(x, ref, "nearest"), ties=R.near_ties(ref))
    return _cache[name]


@pytest.mark.parametrize("name", sorted(R.CASES))
def test_resample_equals_the_reference(name):
    c = case(name)
    g, ref = c["g"], c["ref"]
    xd, ld = torch.from_numpy(c["x"]).to(DEV), torch.from_numpy(c["lab"]).to(DEV)
    with Launches():
        img, lab = ft.resample_volume(xd, g, label=ld)
        img2, lab2 = ft.resample_volume(xd, g, label=ld)
        half, _ = ft.resample_volume(xd, g, out_dtype=BF16)
        near, _ = ft.resample_volume(xd, g, mode="nearest")
    assert img.is_cuda and img.dtype == F32 and tuple(img.shape) == c["image"].shape and lab.dtype == U8
    assert torch.equal(_bits(img), _bits(img2)) and torch.equal(lab, lab2)             # replay: bitwise equal
    scale = np.abs(c["x"]).max()
    err = np.abs(img.cpu().numpy().astype(np.float64) - c["image"]).max()
    print(name, "bilinear max abs err", err, "bound", IMG_BOUND * scale)
    assert err <= IMG_BOUND * scale
    # nearest: exact outside the near-ties of non-dyadic scales
    inner = (slice(None),) + tuple(slice(b, b + n) for b, n in zip(ref["pad"], ref["res"]))
    sure = ~c["ties"]
    print(name, "near-tie share", 1.0 - sure.mean())
    assert 1.0 - sure.mean() <= 1e-3
    assert np.array_equal(lab.cpu().numpy()[inner][:, sure], c["label"][inner][:, sure])
    assert np.array_equal(near.cpu().numpy()[inner][:, sure], c["nearest"][inner][:, sure])
    pad = np.ones(ref["out"], dtype=bool)
    pad[inner[1:]] = False
    for t in (img, lab, half, near):
        assert (t.cpu().float().numpy()[:, pad] == 0).all()                                # the pad is written, as zeros
    # bf16: the reference's fp32 value rounded to nearest even; 1 bf16 ulp where the fp32 values differ
    want32 = torch.from_numpy(c["image"].astype(np.float32))
    got, want = _bits(half.cpu()).int(), _bits(want32.to(BF16)).int()
    same32 = img.cpu() == want32
    assert half.dtype == BF16 and torch.equal(got[same32], want[same32]) and (got - want).abs().max() <= 1
    assert torch.equal(_bits(half.cpu()), _bits(img.cpu().to(BF16)))


def test_half_ties_follow_the_half_even_rule_bit_for_bit():
    c = case("half_ties")
    assert not c["ties"].any() and (R.forward_positions(c["ref"])[0] % 1 == 0.5).sum() >= 4
    with Launches():
        near, lab = ft.resample_volume(torch.from_numpy(c["x"]).to(DEV), c["g"], label=torch.from_numpy(c["lab"]).to(DEV),
                                       mode="nearest")
    assert np.array_equal(near.cpu().numpy(), c["nearest"]) and np.array_equal(lab.cpu().numpy(), c["label"])


@pytest.mark.parametrize("size,roi", [((2, 5, 6, 8), None), ((2, 5, 6, 7), (5, 8, 10)), ((1, 3, 4, 12), (3, 4, 16))])
def test_the_identity_map_is_bit_identical_to_indexing(size, roi):
    """W % 4 == 0 (vector stores) and W % 4 != 0 (scalar stores); an infinity would poison an interpolating path"""
    g0 = torch.Generator().manual_seed(1)
    x = torch.randn(size, generator=g0)
    x[0, 1, 2, 3] = float("inf")
    lab = torch.randint(0, 255, size, generator=g0).to(U8)
    g = ft.spacing_geometry(size[1:], np.eye(4), 1.0, roi_size=roi)
    with Launches():
        img, lout = ft.resample_volume(x.to(DEV), g, label=lab.to(DEV))
        perm, _ = ft.resample_volume(x.to(DEV), ft.spacing_geometry(size[1:], R.make_affine("PIR", (1, 1, 1)), 1.0))
    inner = (slice(None),) + tuple(slice(b, b + n) for b, n in zip(g.pad_before, size[1:]))
    assert torch.equal(img.cpu()[inner], x) and torch.equal(lout.cpu()[inner], lab)
    assert not img.isnan().any() and int((img != 0).sum()) == int((x != 0).sum())
    assert torch.equal(perm.cpu(), x.permute(0, 3, 1, 2).flip(2, 3))


def test_unaligned_base_takes_the_scalar_stores():
    """rows of 16 voxels: an aligned output is written in vectors, one that starts an element into its buffer element by
    element — the same bits"""
    c = case("grow_transposed_mirror")
    g = c["g"]
    xd = torch.from_numpy(c["x"]).to(DEV)
    with Launches():
        a, _ = ft.resample_volume(xd, g)
    assert a.shape[-1] % 4 == 0 and a.data_ptr() % 16 == 0
    out = torch.empty(a.numel() + 1, dtype=F32, device=DEV)[1:].view(a.shape)
    rc = _native.lib().fz_vol_respace(xd.data_ptr(), xd.shape[0], out.data_ptr(), _native.VOL_F32, None, 0, None,
                                      ctypes.byref(g.native()), _native.RESPACE_BILINEAR, _native.stream_ptr(xd))
    torch.cuda.synchronize()
    assert rc == 0 and out.data_ptr() % 16 == 4 and torch.equal(_bits(out), _bits(a))


@pytest.mark.parametrize("name", sorted(R.CASES))
@pytest.mark.parametrize("K,dtype", [(1, F32), (5, F32), (1, BF16), (5, BF16)])
def test_restore_equals_the_reference(name, K, dtype):
    c = case(name)
    g, ref = c["g"], c["ref"]
    ls = [torch.from_numpy(l).to(dtype) for l in R.make_logits(3, ref["out"], K)]
    want = R.inverse([l.float().numpy() for l in ls], ref)
    ld = [l[None].to(DEV) for l in ls]
    arg = ld if K > 1 else ld[0]
    with Launches():
        prob = ft.restore_spaced_prediction(arg, g, threshold=None)
        prob2 = ft.restore_spaced_prediction(arg, g, threshold=None)
        mask = ft.restore_spaced_prediction(arg, g, threshold=0.3)
        mask2 = ft.restore_spaced_prediction(arg, g, threshold=0.3)
    assert prob.dtype == F32 and tuple(prob.shape) == (3,) + tuple(ref["orig"]) and mask.dtype == U8
    assert torch.equal(_bits(prob), _bits(prob2)) and torch.equal(mask, mask2)
    err = np.abs(prob.cpu().numpy() - want).max()
    print(name, K, dtype, "probability max abs err", err, "bound", PROB_BOUND)
    assert err <= PROB_BOUND
    sure = np.abs(want - 0.3) > 1e-5
    print(name, "share within 1e-5 of the threshold", 1.0 - sure.mean())
    assert 1.0 - sure.mean() <= 1e-3
    assert np.array_equal(mask.cpu().numpy()[sure], (want >= 0.3)[sure])
    outside = np.ones(ref["orig"], dtype=bool)
    outside[tuple(slice(s, s + n) for s, n in zip(ref["start"], ref["size"]))] = False
    assert (prob.cpu().numpy()[:, outside] == 0).all() and (mask.cpu().numpy()[:, outside] == 0).all()


def test_round_trip_on_device():
    c = case("boxed")
    g = c["g"]
    nd = 3
    A = R.make_case("boxed")[2]
    idx = np.stack(np.meshgrid(*[np.arange(n) for n in g.orig_size], indexing="ij"), -1).astype(np.float64)
    field = (idx @ A[:nd, :nd].T + A[:nd, nd]) @ np.array([0.013, -0.021, 0.008]) + 0.5
    box = tuple(slice(s, s + n) for s, n in zip(g.box_start, g.src_size))
    src = torch.from_numpy(field[box][None].astype(np.float32))
    with Launches():
        fwd, _ = ft.resample_volume(src.to(DEV), g)
        back = ft.restore_spaced_prediction(fwd[None], g, sigmoid=False, threshold=None)
    cpu = ft.restore_spaced_prediction(ft.resample_volume(src, g)[0][None], g, sigmoid=False, threshold=None)
    assert (back.cpu() - cpu).abs().max() <= 2 * IMG_BOUND * np.abs(field).max()
    keep = R.unclamped(c["ref"])                             # forward and inverse positions were not clamped
    assert keep.mean() > 0.3
    assert np.abs(back.cpu().numpy()[0][box] - field[box])[keep].max() <= 1e-5


def test_prepare_spaced_volume_on_device_equals_the_cpu_call():
    x, lab, A, kw = R.make_case("boxed")
    vol = np.zeros((2, 12, 20, 15), dtype=np.float32)
    vol[:, 3:9, 5:14, 4:10] = np.abs(x[:, :6, :9, :6]) + 0.1
    cls = np.zeros((12, 20, 15), dtype=np.uint8)
    cls[4:8, 6:12, 5:9] = 1
    v, c = torch.from_numpy(vol), torch.from_numpy(cls)
    kw = dict(pixdim=2.0, margin=1, roi_size=(24, 8, 8), classes=((1,),))
    want = ft.prepare_spaced_volume(v, A, c, **kw)
    with Launches():
        got = ft.prepare_spaced_volume(v.to(DEV), A, c.to(DEV), **kw)
        half = ft.prepare_spaced_volume(v.to(DEV), A, c.to(DEV), out_dtype=BF16, **kw)
    assert got.box_start == want.box_start and got.box_end == want.box_end and got.pad_before == want.pad_before
    assert got.geometry.res_size == want.geometry.res_size and got.image.shape == want.image.shape
    for k in ("mean", "std"):                                # one fp32 ulp: only the float64 summation order differs
        a, b = getattr(got, k).cpu(), getattr(want, k)
        assert ((_bits(a).int() - _bits(b).int()).abs() <= 1).all()
    # both paths are within IMG_BOUND of the float64 resampling of their normalised box, which differ by the statistics' ulp
    # (2^-22 (|v| + |mean| / std), the bound of tests/test_gpu_vol_prep.py)
    scale = float(want.image.abs().max())
    bound = 2 * IMG_BOUND * scale + 2.0 ** -22 * (scale + float((want.mean.abs() / want.std).max()))
    err = (got.image.cpu() - want.image).abs().max().item()
    print("image max abs difference", err, "bound", bound)
    assert err <= bound
    assert torch.equal(got.label.cpu(), want.label)
    assert half.image.dtype == BF16 and torch.equal(_bits(half.image), _bits(got.image.to(BF16)))


def test_kinds_outside_the_native_set_are_composed_and_warn_once():
    from factorizer_amd import composed
    composed._warned.discard("respace:resample_volume:torch.float64,torch.float32")
    c = case("grow_transposed_mirror")
    x = torch.from_numpy(c["x"]).double()
    with pytest.warns(RuntimeWarning, match="composed") as rec:
        a, _ = ft.resample_volume(x.to(DEV), c["g"])
        ft.resample_volume(x.to(DEV), c["g"])
    assert len([w for w in rec if "resample_volume" in str(w.message)]) == 1
    assert a.is_cuda and a.dtype == F32                       # the composed result: framework ops on the device
    assert np.abs(a.cpu().numpy() - c["image"]).max() <= IMG_BOUND * np.abs(c["x"]).max()
