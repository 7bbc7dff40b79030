"""-m gpu: the augmentation kernels (csrc/augment.hip) against the independent float64 reference tests/aug_ref.py: identity
and flips bit for bit, linear resample, nearest labels, the noise field, smoothing, the whole pipeline, and the native gate."""
import itertools
import warnings

import numpy as np
import pytest
import torch

import factorizer_amd as ft
from factorizer_amd import _native, composed
import aug_cases as K
import aug_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F32, BF16 = torch.float32, torch.bfloat16


class Launches:
    """Asserts that the native library launched exactly `n` kernels inside the block (None: at least one)."""

    def __init__(self, n=None):
        self.n = n

    def __enter__(self):
        self.n0 = _native.launch_count()
        return self

    def __exit__(self, *a):
        torch.cuda.synchronize()
        got = _native.launch_count() - self.n0
        assert got > 0 if self.n is None else got == self.n, f"{got} native launches"


def _np(t):
    return t.detach().cpu().double().numpy()


def _bf16_steps(a, b):
    """distance of two bf16 tensors in representable values (0 = equal, 1 = neighbours)"""
    def key(t):
        i = t.cpu().contiguous().view(torch.int16).to(torch.int32)
        return torch.where(i >= 0, i, -(i & 0x7FFF))
    return (key(a) - key(b)).abs().max().item()


_REF = {}


def _resample_ref(nd, i, dtype):
    """float64 image and label reference of resample case i, computed once and shared"""
    k = (nd, i, dtype)
    if k not in _REF:
        shape, A, F = K.resample_cases(nd)[i]
        x, l = K.image(shape, 10 + i, dtype), K.label(shape, 10 + i, 2)
        p = ft.AugmentParams.identity(shape[0], nd)
        p.affine, p.flip = A, F
        ri, rl = R.augment(x.double().numpy(), l.numpy(), A.double().numpy(), F.numpy(), p.noise_std.numpy(), p.sigma.numpy(),
                           p.gain.numpy(), p.offset.numpy())
        ri.setflags(write=False)
        rl.setflags(write=False)
        _REF[k] = (x, l, p, ri, rl)
    return _REF[k]


# ---- 1. identity and flips ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [F32, BF16])
@pytest.mark.parametrize("shape", [(2, 3, 9, 10, 11), (2, 2, 13, 18)])
def test_identity_and_every_flip_subset_is_a_bit_exact_permutation(shape, dtype):
    nd = len(shape) - 2
    x, l = K.image(shape, 1, dtype).to(DEV), K.label(shape, 1, 2).to(DEV)
    subsets = list(itertools.product((False, True), repeat=nd))
    for j in range(0, len(subsets), 2):                                 # two subsets per call: one per sample
        p = ft.AugmentParams.identity(2, nd)
        p.flip = torch.tensor([subsets[j], subsets[j + 1]])
        with Launches(1):
            gi, gl = ft.augment_batch(x, l, p)
        for b in range(2):
            dims = [1 + k for k in range(nd) if p.flip[b, k]]
            assert torch.equal(gi[b], torch.flip(x[b], dims)), (subsets[j + b], "image")
            assert torch.equal(gl[b], torch.flip(l[b], dims)), (subsets[j + b], "label")
    assert gi.dtype == dtype and gl.dtype == torch.uint8


def test_identity_on_vector_width_extents_and_bool_labels():
    """W % 4 == 0 takes the 16-byte path (the odd shapes above never do); flipped x reverses inside the vector"""
    shape = (2, 2, 6, 5, 16)
    for dtype in (F32, BF16):
        x = K.image(shape, 2, dtype).to(DEV)
        l = (K.label(shape, 2, 1) > 1).to(DEV)
        p = ft.AugmentParams.identity(2, 3)
        p.flip = torch.tensor([[False, False, True], [True, True, False]])
        gi, gl = ft.augment_batch(x, l, p)
        assert gl.dtype == torch.bool
        assert torch.equal(gi[0], x[0].flip(3)) and torch.equal(gl[0], l[0].flip(3))
        assert torch.equal(gi[1], x[1].flip(1, 2)) and torch.equal(gl[1], l[1].flip(1, 2))


# ---- 2. linear resample, 3. nearest labels -----------------------------------------------------------------------------------
CASES = [(3, i) for i in range(6)] + [(2, i) for i in range(3)]


@pytest.mark.parametrize("nd,i", CASES)
def test_linear_resample_fp32(nd, i):
    x, l, p, ri, rl = _resample_ref(nd, i, F32)
    shape = x.shape
    for b in range(shape[0]):
        if not torch.equal(p.affine[b], torch.eye(nd)):
            assert R.clamp_share(_np(p.affine[b]), p.flip[b].tolist(), shape[2:]) > 0.01   # border padding is exercised
    with Launches(1):
        gi, gl = ft.augment_batch(x.to(DEV), l.to(DEV), p)
    err = np.abs(_np(gi) - ri).max()
    print(f"resample nd={nd} case {i}: max abs err {err:.3e}")
    assert err <= 2e-5
    # labels: exact outside the voxels whose float64 position is within 1e-3 of a half-integer
    for b in range(shape[0]):
        exempt = R.near_half(_np(p.affine[b]), p.flip[b].tolist(), shape[2:])
        print(f"  sample {b}: exempt share {exempt.mean():.4f}")
        assert exempt.mean() <= 0.02
        assert np.array_equal(gl[b].cpu().numpy()[:, ~exempt], rl[b][:, ~exempt])


@pytest.mark.parametrize("nd,i", [(3, 0), (3, 4), (2, 1)])
def test_linear_resample_bf16_within_one_ulp(nd, i):
    x, l, p, ri, _ = _resample_ref(nd, i, BF16)
    gi, _ = ft.augment_batch(x.to(DEV), None, p)
    assert gi.dtype == BF16
    steps = _bf16_steps(gi, torch.from_numpy(ri).to(BF16))
    print(f"bf16 resample nd={nd} case {i}: {steps} bf16 steps")
    assert steps <= 1


def test_label_only_and_image_only_calls():
    x, l, p, ri, rl = _resample_ref(3, 1, F32)
    gi, none = ft.affine_resample(x.to(DEV), None, p.affine, p.flip)
    assert none is None and np.abs(_np(gi) - ri).max() <= 2e-5
    none, gl = ft.affine_resample(None, l.to(DEV), p.affine, p.flip)
    both = ft.augment_batch(x.to(DEV), l.to(DEV), p)[1]
    assert none is None and torch.equal(gl, both)


# ---- 4. noise field ----------------------------------------------------------------------------------------------------------
def test_noise_field_matches_the_restatement():
    shape, seed = (2, 3, 7, 9, 11), 0x0123456789ABCDEF                   # 693 voxels per plane: not a multiple of 4
    with Launches(1):
        z = ft.gaussian_noise_field(shape, seed, DEV)
    ref = R.noise_field(shape, seed)
    err = np.abs(_np(z) - ref).max()
    print(f"noise field: max abs err {err:.3e}, max |z| {np.abs(ref).max():.3f}")
    assert z.dtype == F32 and z.shape == shape and err <= 2e-5
    assert torch.equal(z, ft.gaussian_noise_field(shape, seed, DEV))
    seed_t = torch.tensor([seed], dtype=torch.int64, device=DEV)         # a device seed: used where it is
    assert torch.equal(z, ft.gaussian_noise_field(shape, seed_t))
    other = ft.gaussian_noise_field(shape, seed + 1, DEV)
    assert not torch.equal(z, other) and np.abs(_np(other) - R.noise_field(shape, seed + 1)).max() <= 2e-5
    planes = z.reshape(6, -1)
    for a in range(6):
        for b in range(a + 1, 6):
            assert not torch.equal(planes[a], planes[b])                # channel and sample change the counter
    quads = planes[:, :692].reshape(6, 173, 4)
    assert not torch.equal(quads[:, 0], quads[:, 1]) and len({tuple(q.tolist()) for q in quads[0]}) == 173


# ---- 5. smoothing ------------------------------------------------------------------------------------------------------------
SMOOTH = [((3, 2, 17, 19, 23), [[0.5, 0.75, 1.0], [0.0, 0.0, 0.0], [0.0, 0.9, 0.0]]),
          ((3, 2, 21, 37), [[0.0, 0.0], [0.75, 1.0], [0.6, 0.0]]),
          ((2, 2, 5, 19, 9), [[1.0, 0.5, 1.0], [1.0, 0.0, 0.0]]),        # an extent of 5 under 9 taps: zero padding both sides
          ((2, 1, 5, 40), [[1.0, 1.0], [0.0, 0.5]])]


@pytest.mark.parametrize("shape,sigma", SMOOTH)
@pytest.mark.parametrize("dtype", [F32, BF16])
def test_smoothing(shape, sigma, dtype):
    x = K.image(shape, 4, dtype)
    sig = torch.tensor(sigma)
    ns = int((sig > 0).any(1).sum())
    with Launches(2):                                                   # the resample launch + ONE smoothing launch
        got = ft.gaussian_smooth(x.to(DEV), sig)
    ref = np.stack([R.smooth(x[b].double().numpy(), sigma[b]) for b in range(shape[0])])
    assert got.dtype == dtype and ns >= 1
    if dtype == F32:
        err = np.abs(_np(got) - ref).max()
        print(f"smooth {shape}: max abs err {err:.3e}")
        assert err <= 1e-5
    else:                                                               # fp32 inside, ONE rounding at the store
        tol = 1e-5 + np.abs(ref) * 2.0 ** -8                            # half a bf16 step is at most |x| 2^-8
        assert (np.abs(_np(got) - ref) <= tol).all()
    for b in range(shape[0]):
        if not any(s > 0 for s in sigma[b]):
            assert torch.equal(got[b].cpu(), x[b])                      # not listed: untouched


def test_no_smoothing_drawn_launches_once():
    x = K.image((2, 1, 8, 9, 10), 6).to(DEV)
    with Launches(1):
        ft.augment_batch(x, None, ft.AugmentParams.identity(2, 3))


# ---- 6. whole pipeline --------------------------------------------------------------------------------------------------------
def _pipeline_params():
    p = ft.AugmentParams.identity(4, 3, seed=0x7EA5EED0BADC0DE)
    A = torch.tensor(R.matrix((0.2, -0.26, 0.1), (1.15, 0.85, 1.2), 3), dtype=F32)
    p.affine[0], p.affine[2] = A, torch.tensor(R.matrix((-0.1, 0.05, 0.26), (0.9, 1.1, 1.0), 3), dtype=F32)
    p.flip[0] = torch.tensor([True, False, True])
    p.flip[2] = torch.tensor([False, True, False])
    p.noise_std[0], p.noise_std[3] = 0.1, 0.07
    p.sigma[0] = torch.tensor([0.5, 0.75, 1.0])
    p.sigma[3] = torch.tensor([1.0, 0.0, 0.8])
    p.gain[0], p.offset[0] = 1.25, -0.08
    p.gain[2], p.offset[2] = 0.75, 0.1
    return p                # samples: all steps, none, resample + intensity only, noise + smooth only


@pytest.mark.parametrize("dtype", [F32, BF16])
def test_whole_pipeline(dtype):
    shape = (4, 3, 20, 24, 28)
    x, l = K.image(shape, 20, dtype), K.label(shape, 20, 1)
    p = _pipeline_params()
    with Launches(2):
        gi, gl = ft.augment_batch(x.to(DEV), l.to(DEV), p)
    z = ft.gaussian_noise_field(shape, p.seed, DEV)
    ri, rl = R.augment(x.double().numpy(), l.numpy(), p.affine.double().numpy(), p.flip.numpy(), p.noise_std.double().numpy(),
                       p.sigma.double().numpy(), p.gain.double().numpy(), p.offset.double().numpy(), _np(z))
    d = np.abs(_np(gi) - ri)
    print(f"pipeline {dtype}: max abs err per sample {[float(d[b].max()) for b in range(4)]}")
    if dtype == F32:
        assert d.max() <= 3e-5
        assert torch.equal(gi[1].cpu(), x[1])
    else:       # the fp32 bound plus the one rounding of the store (half a bf16 step <= |x| 2^-8)
        assert (d <= 3e-5 + np.abs(ri) * 2.0 ** -8).all()
        assert torch.equal(gi[1].cpu(), x[1])
    for b in range(4):
        exempt = R.near_half(p.affine[b].double().numpy(), p.flip[b].tolist(), shape[2:])
        assert exempt.mean() <= 0.02
        assert np.array_equal(gl[b].cpu().numpy()[:, ~exempt], rl[b][:, ~exempt])
    gi2, gl2 = ft.augment_batch(x.to(DEV), l.to(DEV), p)
    assert torch.equal(gi, gi2) and torch.equal(gl, gl2)                # two runs: bitwise equal


def test_batch_augment_module_on_device():
    shape = (4, 2, 12, 14, 16)
    x, l = K.image(shape, 30).to(DEV), K.label(shape, 30, 1).to(DEV)
    aug = ft.BatchAugment(3, affine_prob=0.6, noise_prob=0.6, smooth_prob=0.6)
    aug.eval()
    a, b = aug(x, l)
    assert a is x and b is l
    aug.train()
    g = torch.Generator().manual_seed(11)
    with Launches():
        a, b = aug(x, l, generator=g)
    params = ft.draw_augment_params(4, 3, generator=torch.Generator().manual_seed(11), **aug.kwargs)
    c, d = ft.augment_batch(x, l, params)
    assert torch.equal(a, c) and torch.equal(b, d) and not a.requires_grad and a.shape == x.shape
    ci, cl = ft.augment_batch(x.cpu(), l.cpu(), params)                 # the composed CPU path means the same
    assert (a.cpu() - ci).abs().max().item() <= 3e-5


# ---- 7. gate -----------------------------------------------------------------------------------------------------------------
def _gate_params(B, nd):
    p = ft.AugmentParams.identity(B, nd, seed=99)
    p.affine[0] = ft.augment.affine_matrix((0.2,) * {1: 0, 2: 1, 3: 3}[nd], (1.1,) * nd, nd)
    p.flip[1, nd - 1] = True
    p.noise_std[0] = 0.05
    p.sigma[1] = 0.8
    p.gain[0], p.offset[1] = 1.2, 0.05
    return p


@pytest.mark.parametrize("shape,dtype,tol", [((2, 2, 10, 12, 14), torch.float16, 1e-3), ((2, 3, 57), F32, 1e-5)])
def test_outside_the_gate_warns_once_and_matches_the_cpu(shape, dtype, tol):
    nd = len(shape) - 2
    x, l = K.image(shape, 40, dtype), K.label(shape, 40, 1)
    p = _gate_params(shape[0], nd)
    for k in [k for k in composed._warned if k.startswith("augment:")]:
        composed._warned.discard(k)
    n0 = _native.launch_count()
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        gi, gl = ft.augment_batch(x.to(DEV), l.to(DEV), p)
        ft.augment_batch(x.to(DEV), l.to(DEV), p)
    assert len([m for m in w if "composed framework ops" in str(m.message)]) == 1
    assert _native.launch_count() == n0
    ci, cl = ft.augment_batch(x, l, p)
    assert gi.dtype == dtype and gi.is_cuda
    assert (gi.cpu().double() - ci.double()).abs().max().item() <= tol
    assert torch.equal(gl.cpu(), cl)


def test_wide_sigma_runs_composed_with_one_warning():
    x = K.image((1, 1, 12, 14), 41)
    for k in [k for k in composed._warned if k.startswith("augment:")]:
        composed._warned.discard(k)
    with pytest.warns(RuntimeWarning, match="composed framework ops"):
        got = ft.gaussian_smooth(x.to(DEV), 1.3)
    assert np.abs(_np(got)[0] - R.smooth(x[0].double().numpy(), [1.3, 1.3])).max() <= 1e-5
