"""-m gpu: the volume kernels (csrc/volprep.hip) against the independent float64 reference tests/vol_prep_ref.py.

Pass conditions (derived, not measured): box, encoded label, restored mask and label map equal bit for bit; mean and std
within one fp32 ulp of the float64 reference rounded to fp32 (only the float64 summation order differs); the fp32 image
bit-equal to torch.where(sel, (x − mean) / std, x) evaluated in fp32 on the CPU from the returned statistics, and within
2^-22 (|x| + |mean|) / std of the float64 reference (four roundings of at most 2^-24 relative each: mean, std, the
subtraction, the quotient); the bf16 image bit-equal to the fp32 native result .to(bfloat16); two calls bit-identical."""
import warnings

import pytest
import torch

import factorizer_amd as ft
from factorizer_amd import _native
import vol_prep_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F32, BF16, U8, I16 = torch.float32, torch.bfloat16, torch.uint8, torch.int16


class Launches:
    """Asserts that the native library actually launched kernels inside the block."""

    def __enter__(self):
        self.n0 = _native.launch_count()
        return self

    def __exit__(self, *a):
        torch.cuda.synchronize()
        assert _native.launch_count() > self.n0, "native kernels were not launched"


def _dev(x, offset=0):
    """x on the device, its first element `offset` elements into its buffer (an unaligned base)"""
    buf = torch.zeros(x.numel() + offset, dtype=x.dtype)
    buf[offset:] = x.reshape(-1)
    return buf.to(DEV)[offset:].view(x.shape)


def _bits(t):
    return t.view(torch.int16) if t.dtype == BF16 else t.view(torch.int32)


def _native_prepare(x, lab, offset=0, **kw):
    """prepare_volume on the device with nothing composed: fp32 and bf16 results, and a second fp32 call"""
    xd, ld = _dev(x, offset), None if lab is None else _dev(lab, offset)
    with Launches(), warnings.catch_warnings():
        warnings.simplefilter("error")                       # inside the native gate: nothing composed
        a = ft.prepare_volume(xd, ld, **kw)
        b = ft.prepare_volume(xd, ld, **kw)
        h = ft.prepare_volume(xd, ld, out_dtype=BF16, **kw)
    assert a.image.is_cuda and a.mean.is_cuda
    # replay: bit-identical tensors and statistics
    assert torch.equal(_bits(a.image), _bits(b.image)) and torch.equal(_bits(a.mean), _bits(b.mean))
    assert torch.equal(_bits(a.std), _bits(b.std)) and (a.label is None or torch.equal(a.label, b.label))
    # bf16: the fp32 result rounded to nearest even
    assert h.image.dtype == BF16 and torch.equal(_bits(h.image), _bits(a.image.to(BF16)))
    assert torch.equal(_bits(h.mean), _bits(a.mean)) and (a.label is None or torch.equal(a.label, h.label))
    return a


@pytest.mark.parametrize("name", sorted(R.CASES))
def test_prepare_equals_the_reference(name):
    x, kw = R.make_case(name)
    lab = R.class_map(x.shape[1:], 1)
    got = _native_prepare(x, lab, classes=R.BRATS_CLASSES, **kw)
    ref = R.prepare(x, lab, classes=R.BRATS_CLASSES, **kw)
    R.check_prepared(got, ref)
    R.check_label(got, ref)
    with Launches():
        s, e = ft.foreground_bbox(_dev(x), kw["margin"], kw.get("allow_smaller", True))
    assert (s, e) == (ref["start"], ref["end"]) and all(isinstance(v, int) for v in s + e)


@pytest.mark.parametrize("offset", [1, 3])
@pytest.mark.parametrize("dtype", [F32, I16])
def test_unaligned_base_and_rows_that_are_no_multiple_of_the_vector(offset, dtype):
    """(1, 19, 21, 130): 130 is no multiple of 4, and the buffers start 1 and 3 elements off a 16-byte boundary"""
    vk, kw = R.CASES["3d_long_rows"]
    x = R.volume(**dict(vk, dtype=dtype))
    lab = R.class_map(x.shape[1:], 2, dtype=I16 if dtype == I16 else U8)
    got = _native_prepare(x, lab, offset=offset, classes=R.BRATS_CLASSES, **kw)
    ref = R.prepare(x, lab, classes=R.BRATS_CLASSES, **kw)
    R.check_prepared(got, ref)
    R.check_label(got, ref)


def test_label_forms():
    x, kw = R.make_case("odd_pads")
    lab = R.class_map(x.shape[1:], 3, dtype=I16, top=6)
    lab[0, 0, :4] = torch.tensor([-1, 31, 32, 300], dtype=I16)               # ids outside every set, outside 0 .. 31 too
    two = ((1, 4), (0, 2, 5, 31))
    kw = dict(kw, margin=30)                                                 # the whole image: the planted ids are inside
    for l in (lab, lab[None]):
        R.check_label(_native_prepare(x, l, classes=two, **kw), R.prepare(x, lab, classes=two, **kw))
    ready = R.encode(lab, two)
    ready[1][ready[1] != 0] = 200                                            # channel-first: copied as it is
    R.check_label(_native_prepare(x, ready, **kw), R.prepare(x, ready, **kw))
    assert _native_prepare(x, None, **kw).label is None


def test_recipe_plane_int16():
    """(1, 240, 240, 155) int16, the size at which the input passes grow their per-workgroup share (more than 1024 chunks
    otherwise); no roi, the inference recipe"""
    x = R.volume((1, 240, 240, 155), ((30, 200), (25, 215), (8, 140)), 18, dtype=I16)
    with Launches(), warnings.catch_warnings():
        warnings.simplefilter("error")
        got = ft.prepare_volume(_dev(x), margin=10)
    R.check_prepared(got, R.prepare(x, margin=10))
    assert got.box_start == (20, 15, 0) and got.box_end == (210, 225, 150)


@pytest.mark.parametrize("nonzero,channel_wise", [(True, True), (False, True), (True, False), (False, False)])
def test_normalize_intensity(nonzero, channel_wise):
    x = R.volume((3, 9, 12, 10), ((1, 8), (2, 11), (0, 9)), 21, neg_inside=True)
    b = torch.stack([x, x.flip(1)])
    with Launches(), warnings.catch_warnings():
        warnings.simplefilter("error")
        got = ft.normalize_intensity(b.to(DEV), nonzero, channel_wise)
    for i in range(2):
        ref = R.prepare(b[i], margin=100, nonzero=nonzero, channel_wise=channel_wise)       # the box is the whole image
        err = (got[i].cpu().double() - ref["image"]).abs()
        view = (-1, 1, 1, 1)
        m64, s64 = (torch.tensor(ref[k], dtype=torch.float64).view(view) for k in ("mean", "std"))
        bound = 2.0 ** -22 * (b[i].double().abs() + m64.abs()) / s64
        print("image max abs err", err.max().item(), "worst err / bound", (err / bound.clamp_min(1e-300)).max().item())
        assert (err <= bound).all()
        assert torch.equal(got[i].cpu() == 0, b[i] == 0) or not nonzero
        # the same bits as the chain run over the whole image, whose statistics and fp32 formula check_prepared pins
        p = ft.prepare_volume(b[i].to(DEV), margin=100, nonzero=nonzero, channel_wise=channel_wise)
        R.check_prepared(p, ref)
        assert torch.equal(_bits(got[i]), _bits(p.image[0]))


# ---- restore ---------------------------------------------------------------------------------------------------------------------
def _restore_check(p, C, K, dtype, offset=0, threshold=0.3, label_values=(7, 200, 9)):
    shape = (C,) + tuple(p.image.shape[2:])
    ls = R.logits_for(shape, K, 31 + K, dtype, threshold=threshold)
    gap = (R.ensemble64(ls) - R.bound64(threshold)).abs().min().item()
    print("smallest distance of an ensemble mean from the bound", gap)
    assert gap > 1e-3                                        # the fp32 summation cannot flip a decision
    ld = [_dev(t, offset) for t in ls]
    args = (p.box_start, p.box_end, p.pad_before, p.orig_size)
    with Launches(), warnings.catch_warnings():
        warnings.simplefilter("error")
        mask = ft.restore_prediction(ld if K > 1 else ld[0], p, threshold=threshold)
        lm = ft.restore_prediction(ld, p, threshold=threshold, label_values=label_values[:C])
        mask2 = ft.restore_prediction(ld, p, threshold=threshold)
    assert mask.dtype == U8 and mask.shape == (C,) + p.orig_size and torch.equal(mask, mask2)
    assert torch.equal(mask.cpu(), R.restore(ls, *args, threshold=threshold))
    assert lm.dtype == U8 and lm.shape == p.orig_size
    assert torch.equal(lm.cpu(), R.restore(ls, *args, threshold=threshold, label_values=label_values[:C]))


@pytest.mark.parametrize("K", [1, 3, 8])
@pytest.mark.parametrize("dtype", [F32, BF16])
def test_restore_mask_and_label_map(K, dtype):
    x, kw = R.make_case("3d_mixed_pad")
    _restore_check(ft.prepare_volume(x, **kw), 3, K, dtype)


@pytest.mark.parametrize("name,offset", [("margin_outside", 0), ("3d_long_rows", 1), ("3d_long_rows", 3), ("2d", 0),
                                         ("1d", 0), ("1d_padded", 2), ("no_roi", 0)])
def test_restore_geometries(name, offset):
    x, kw = R.make_case(name)
    _restore_check(ft.prepare_volume(x, **kw), 2 if name.startswith("1d") else 3, 3, F32, offset)


def test_restore_threshold_one_half_and_priority():
    geo = dict(box_start=(0, 0), box_end=(2, 4), pad_before=(0, 0), orig_size=(2, 4))
    z = torch.tensor([[[-1., 1, -1, 1], [-1, -1, 1, 1]], [[-1., 1, 1, -1], [1, -1, 1, 1]],
                      [[-1., 1, 1, 1], [1, 1, -1, 1]]])[None]
    with Launches():
        lm = ft.restore_prediction(z.to(DEV), geo, label_values=ft.BRATS_LABEL_VALUES)
    assert lm.cpu().tolist() == [[0, 3, 1, 3], [1, 2, 3, 3]]


def test_round_trip_on_device():
    x, kw = R.make_case("3d_mixed_pad")
    g = torch.Generator().manual_seed(5)
    lab = torch.zeros(x.shape[1:], dtype=U8)
    r = torch.rand(x.shape[1:], generator=g)
    lab[r < 0.6] = 2
    lab[r < 0.4] = 1
    lab[r < 0.2] = 3
    with Launches():
        p = ft.prepare_volume(x.to(DEV), lab.to(DEV), classes=ft.BRATS_CLASSES, **kw)
        ls = [t.to(DEV) for t in R.logits_for(tuple(p.label.shape[1:]), 5, 41, BF16, target=p.label[0].cpu() != 0)]
        out = ft.restore_prediction(ls, p, label_values=ft.BRATS_LABEL_VALUES).cpu()
    box = tuple(slice(max(s, 0), min(e, n)) for s, e, n in zip(p.box_start, p.box_end, p.orig_size))
    inside = torch.zeros_like(lab, dtype=torch.bool)
    inside[box] = True
    assert torch.equal(out[box], lab[box]) and (out[~inside] == 0).all()


def test_label_map_over_more_than_eight_channels_is_composed_and_says_so():
    from factorizer_amd import composed
    composed._warned.discard("volume:restore_prediction:other")
    geo = dict(box_start=(1, 2), box_end=(7, 9), pad_before=(1, 0), orig_size=(8, 10))
    ls = R.logits_for((9, 8, 7), 2, 51, F32)
    vals = tuple(range(1, 10))
    with pytest.warns(RuntimeWarning, match="label map over 9 channels") as rec:
        a = ft.restore_prediction([t.to(DEV) for t in ls], geo, label_values=vals)
        ft.restore_prediction([t.to(DEV) for t in ls], geo, label_values=vals)
    assert len(rec) == 1
    assert torch.equal(a.cpu(), R.restore(ls, (1, 2), (7, 9), (1, 0), (8, 10), label_values=vals))
    with Launches(), warnings.catch_warnings():
        warnings.simplefilter("error")                       # the mask form takes any channel count
        m = ft.restore_prediction([t.to(DEV) for t in ls], geo)
    assert torch.equal(m.cpu(), R.restore(ls, (1, 2), (7, 9), (1, 0), (8, 10)))


def test_kinds_outside_the_native_set_are_composed_and_warn_once():
    from factorizer_amd import composed
    composed._warned.discard("volume:prepare_volume:torch.float16,torch.float32")
    x, kw = R.make_case("odd_pads")
    x = x.half()                                             # fp16 values are fp32 values: the reference sees the same numbers
    with pytest.warns(RuntimeWarning, match="composed") as rec:
        a = ft.prepare_volume(x.to(DEV), **kw)
        ft.prepare_volume(x.to(DEV), **kw)
    assert len([w for w in rec if "prepare_volume" in str(w.message)]) == 1
    R.check_prepared(a, R.prepare(x, **kw))
