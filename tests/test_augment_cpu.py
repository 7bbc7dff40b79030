"""ft.augment_batch and its pieces on CPU tensors (the composed path and the host logic) against the independent float64
reference tests/aug_ref.py, the record draws, the taps, the Box-Muller restatement, and the host-side argument checks of the
fz_aug_* entry points (called through ctypes; nothing touches a device)."""
import ctypes
import warnings

import numpy as np
import pytest
import torch

import factorizer_amd as ft
from factorizer_amd import augment as AG
import aug_cases as K
import aug_ref as R
import philox_ref as PR


def _params(B, nd, seed=1234):
    return ft.AugmentParams.identity(B, nd, seed)


def _ref(image, label, p, noise=None):
    return R.augment(None if image is None else image.double().numpy(), None if label is None else label.numpy(),
                     p.affine.double().numpy(), p.flip.numpy(), p.noise_std.double().numpy(), p.sigma.double().numpy(),
                     p.gain.double().numpy(), p.offset.double().numpy(), noise)


@pytest.mark.parametrize("nd", [3, 2])
def test_composed_pipeline_matches_the_reference(nd):
    """every sample of the batch runs all four steps with its own record; fp32 composed ops against float64: the resample
    alone differs by 2.3e-6 at these shapes, noise and nine-tap sums add a few 1e-6 -> 3e-5 as on the device"""
    shape, A, F = K.resample_cases(nd)[0]
    B = shape[0]
    x, l = K.image(shape, 3), K.label(shape, 3)
    p = _params(B, nd, seed=0x1234567890ABCDE)
    p.affine, p.flip = A, F
    p.noise_std = torch.tensor([0.1, 0.05, 0.0][:B])
    p.sigma = torch.tensor([[0.5, 0.75, 1.0], [1.0, 0.0, 0.6], [0.0, 0.0, 0.0]])[:B, :nd].clone()
    p.gain = torch.tensor([1.3, 0.7, 1.0][:B])
    p.offset = torch.tensor([-0.1, 0.05, 0.0][:B])
    with warnings.catch_warnings():
        warnings.simplefilter("error")                       # CPU tensors: composed ops, silently
        gi, gl = ft.augment_batch(x, l, p)
        z = ft.gaussian_noise_field(shape, p.seed)
    ri, rl = _ref(x, l, p, R.noise_field(shape, p.seed))
    assert gi.dtype == x.dtype and gl.dtype == l.dtype and gi.shape == x.shape and gl.shape == l.shape
    assert np.abs(z.double().numpy() - R.noise_field(shape, p.seed)).max() <= 2e-5
    err = np.abs(gi.double().numpy() - ri).max()
    print("composed pipeline max abs err", err)
    assert err <= 3e-5
    for b in range(B):
        ok = ~R.near_half(p.affine[b].double().numpy(), p.flip[b].tolist(), shape[2:])
        assert ok.mean() >= 0.98
        assert np.array_equal(gl[b].numpy()[:, ok], rl[b][:, ok])


@pytest.mark.parametrize("nd", [3, 2])
def test_composed_identity_is_a_flip_bit_for_bit(nd):
    shape = K.SHAPE3 if nd == 3 else K.SHAPE2
    x, l = K.image(shape, 5, torch.bfloat16), K.label(shape, 5)
    p = _params(shape[0], nd)
    p.flip[0, nd - 1] = True
    p.flip[1, 0] = True
    gi, gl = ft.augment_batch(x, l, p)
    for b, dims in ((0, [nd]), (1, [1])):
        assert torch.equal(gi[b], torch.flip(x[b], dims)) and torch.equal(gl[b], torch.flip(l[b], dims))
    gi, gl = ft.affine_resample(x, l)
    assert torch.equal(gi, x) and torch.equal(gl, l) and gi is not x


def test_fixed_matrices_cover_flips_and_the_clamp():
    for nd in (2, 3):
        assert K.all_flip_subsets_appear(nd)
        for shape, A, F in K.resample_cases(nd):
            ident = [b for b in range(shape[0]) if torch.equal(A[b], torch.eye(nd))]
            assert len(ident) == 1
            for b in range(shape[0]):
                if b not in ident:
                    assert R.clamp_share(A[b].double().numpy(), F[b].tolist(), shape[2:]) > 0.01


# ---- draws ---------------------------------------------------------------------------------------------------------------
def _same(p, q):
    return all(torch.equal(getattr(p, k), getattr(q, k)) for k in ("affine", "flip", "noise_std", "sigma", "gain", "offset")) \
        and p.seed == q.seed


@pytest.mark.parametrize("nd", [2, 3])
def test_draws_repeat_with_the_generator_state(nd):
    g = torch.Generator().manual_seed(7)
    state = g.get_state()
    p = ft.draw_augment_params(16, nd, generator=g)
    q = ft.draw_augment_params(16, nd, generator=g)
    g.set_state(state)
    r = ft.draw_augment_params(16, nd, generator=g)
    assert _same(p, r) and not _same(p, q)


@pytest.mark.parametrize("nd", [2, 3])
def test_probabilities_zero_and_one(nd):
    g = torch.Generator().manual_seed(8)
    never = dict(affine_prob=0, noise_prob=0, smooth_prob=0, scale_intensity_prob=0, shift_intensity_prob=0, flip_prob=0)
    p = ft.draw_augment_params(64, nd, generator=g, **never)
    assert _same(p, ft.AugmentParams.identity(64, nd, p.seed))            # nothing drawn: the identity record
    always = {k: 1 for k in never}
    p = ft.draw_augment_params(64, nd, generator=g, **always)
    eye = torch.eye(nd)
    assert all(not torch.equal(p.affine[b], eye) for b in range(64))
    assert p.flip.all() and (p.noise_std > 0).all() and (p.sigma > 0).all()
    assert (p.gain != 1).all() and (p.offset != 0).all()
    p = ft.draw_augment_params(64, nd, generator=g, flip_prob=1, flip_axes=(nd - 1,))
    assert p.flip[:, nd - 1].all() and not p.flip[:, :nd - 1].any()


@pytest.mark.parametrize("nd", [2, 3])
def test_ranges_over_2000_draws(nd):
    g = torch.Generator().manual_seed(9)
    p = ft.draw_augment_params(2000, nd, generator=g, affine_prob=1, noise_prob=1, smooth_prob=1, scale_intensity_prob=1,
                               shift_intensity_prob=1)
    assert 0 < float(p.noise_std.min()) and float(p.noise_std.max()) <= 0.1
    assert float(p.sigma.min()) >= 0.5 and float(p.sigma.max()) <= 1.0 and AG.native_sigma_ok(p.sigma)
    assert float((p.gain - 1).abs().max()) <= 0.3 + 1e-6 and float(p.offset.abs().max()) <= 0.1 + 1e-7
    A = p.affine.double()
    s = A.norm(dim=1)                                                    # column norms of R diag(s) are the scales
    assert float(s.min()) >= 0.8 - 1e-6 and float(s.max()) <= 1.2 + 1e-6
    Rm = A / s[:, None, :]
    assert float((Rm.transpose(1, 2) @ Rm - torch.eye(nd, dtype=torch.float64)).abs().max()) < 1e-6
    assert float((torch.linalg.det(Rm) - 1).abs().max()) < 1e-6
    if nd == 2:
        ang = torch.atan2(Rm[:, 1, 0], Rm[:, 0, 0])
        assert float(ang.abs().max()) <= 0.26 + 1e-6 and float(ang.min()) < -0.2 and float(ang.max()) > 0.2
    else:                                                                # Rx Ry Rz: R[0, 2] = sin(theta1)
        assert float(torch.asin(Rm[:, 0, 2]).abs().max()) <= 0.26 + 1e-6
        th0 = torch.atan2(-Rm[:, 1, 2], Rm[:, 2, 2])
        th2 = torch.atan2(-Rm[:, 0, 1], Rm[:, 0, 0])
        assert float(th0.abs().max()) <= 0.26 + 1e-6 and float(th2.abs().max()) <= 0.26 + 1e-6
    rate = float(p.flip.float().mean())
    assert 0.45 < rate < 0.55                                           # 2000 nd fair coins: sigma <= 0.008
    q = ft.draw_augment_params(2000, nd, generator=g)                    # the recipe's probabilities
    drawn = [float((q.noise_std > 0).float().mean()), float((q.sigma > 0).any(1).float().mean()),
             float((q.gain != 1).float().mean()), float((q.offset != 0).float().mean()),
             float(((q.affine - torch.eye(nd)).abs().amax((1, 2)) > 0).float().mean())]
    assert all(0.16 < d < 0.24 for d in drawn), drawn                   # p = 0.2, n = 2000: sigma = 0.009


def test_affine_matrix_follows_the_stated_rotation_order():
    A = AG.affine_matrix((0.2, -0.1, 0.15), (1.1, 0.9, 1.2), 3).double().numpy()
    assert np.abs(A - R.matrix((0.2, -0.1, 0.15), (1.1, 0.9, 1.2), 3)).max() == 0
    A = AG.affine_matrix((0.2,), (1.1, 0.9), 2).double().numpy()
    assert np.abs(A - R.matrix((0.2,), (1.1, 0.9), 2)).max() == 0


# ---- taps ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sigma,n", [(0.5, 5), (0.75, 7), (1.0, 9)])
def test_tap_lengths_and_sums(sigma, n):
    w = AG.gaussian_taps(sigma)
    assert w.dtype == torch.float32 and w.numel() == n and torch.equal(w, w.flip(0))
    assert np.array_equal(w.double().numpy(), R.taps(sigma))
    total = float(w.double().sum())
    print("tap sum", sigma, total)
    assert abs(total - 1.0) <= 1e-4
    assert AG.native_sigma_ok([sigma])


def test_tail_five_is_outside_the_native_gate():
    assert AG.gaussian_tail(1.124) == 4 and AG.native_sigma_ok([1.124, 0.0])
    assert AG.gaussian_tail(1.125) == 5 and AG.gaussian_taps(1.125).numel() == 11
    assert not AG.native_sigma_ok([0.5, 1.125])
    x = K.image((1, 1, 12, 14), 2)
    got = ft.gaussian_smooth(x, 1.3)                                     # runs composed on the CPU whatever the tail
    assert np.abs(got.double().numpy()[0] - R.smooth(x[0].double().numpy(), [1.3, 1.3])).max() <= 1e-5


# ---- Box-Muller restatement ---------------------------------------------------------------------------------------------------
def test_philox_words_behind_the_normals_pass_the_known_answer_vectors():
    for ctr, key, want in PR.KAT:
        assert tuple(int(v) for v in PR.philox4x32_10(*ctr, *key)) == want
        got = AG._philox4x32_10(*(torch.tensor([c], dtype=torch.int64) for c in ctr),
                                *(torch.tensor([k], dtype=torch.int64) for k in key))
        assert tuple(int(v) for v in got) == want
        z = R.box_muller([np.array([w]) for w in want])[0]
        u = [((w >> 8) + 0.5) / 2 ** 24 for w in want]
        assert abs(z[0] - np.sqrt(-2 * np.log(u[0])) * np.cos(2 * np.pi * u[1])) < 1e-12
        assert abs(z[3] - np.sqrt(-2 * np.log(u[2])) * np.sin(2 * np.pi * u[3])) < 1e-12


def test_a_million_restated_normals_have_mean_zero_and_unit_variance():
    z = R.noise_field((2, 5, 100, 1000), seed=0x5EED5EED5EED)
    assert z.size == 10 ** 6
    print("normals: mean", z.mean(), "var", z.var())
    assert abs(z.mean()) <= 0.01 and abs(z.var() - 1.0) <= 0.01
    assert np.abs(z).max() <= 5.9                                        # 24-bit uniforms: |z| <= sqrt(2 ln 2^25)
    got = ft.gaussian_noise_field((2, 5, 100, 50), 0x5EED5EED5EED).double().numpy()   # the package's host restatement
    assert np.abs(got - R.noise_field((2, 5, 100, 50), 0x5EED5EED5EED)).max() <= 2e-5


# ---- host-side argument checks (ctypes, no device work) -------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    from factorizer_amd import _native, build
    build.build(verbose=False)
    return _native.lib()


P8 = ctypes.c_void_p(4096)   # a non-null, aligned pointer value the host code never dereferences
P9 = ctypes.c_void_p(8192)


def test_resample_argument_checks(lib):
    assert lib.fz_aug_record_floats() == AG.REC
    ok = dict(img=P8, out=P9, dt=0, C=2, lab=None, lab_out=None, L=0, table=P8, seed=None, ws=None, ns=0, B=2, nd=3, D=8, H=8, W=8)

    def call(**kw):
        a = {**ok, **kw}
        return lib.fz_aug_resample(a["img"], a["out"], a["dt"], a["C"], a["lab"], a["lab_out"], a["L"], a["table"], a["seed"],
                                   a["ws"], a["ns"], a["B"], a["nd"], a["D"], a["H"], a["W"], None)
    assert call(table=None) == -4 and b"table" in lib.fz_last_error_string()
    assert call(img=None) == -4 and call(out=None) == -4 and call(L=1) == -4          # label planes without pointers
    assert call(out=P8) == -4 and b"alias" in lib.fz_last_error_string()
    assert call(dt=7) == -4 and b"act_dtype" in lib.fz_last_error_string()
    assert call(nd=1) == -4 and call(nd=4) == -4 and b"nd" in lib.fz_last_error_string()
    assert call(W=2049) == -1 and b"2048" in lib.fz_last_error_string()
    assert call(D=2049) == -1 and call(H=2049) == -1
    assert call(nd=2) == -1                                                           # D must be 1 for a 2-D image
    assert call(C=0) == -1 and call(B=0) == -1 and call(W=0) == -1
    assert call(ns=1) == -4 and call(ns=3, ws=P8) == -4                               # slots need a workspace, ns <= B
    assert call(D=2048, H=2048, W=512) == -2                                          # 2^31 voxels per plane: unsupported
    assert call(img=ctypes.c_void_p(4098)) == -4


def test_smooth_and_noise_argument_checks(lib):
    def smooth(ws=P8, out=P9, dt=0, C=2, table=P8, lst=P8, ns=1, B=2, nd=3, D=8, H=8, W=8):
        return lib.fz_aug_smooth(ws, out, dt, C, table, lst, ns, B, nd, D, H, W, None)
    assert smooth(out=None) == -4 and smooth(table=None) == -4 and smooth(ws=None) == -4 and smooth(lst=None) == -4
    assert smooth(dt=3) == -4 and b"act_dtype" in lib.fz_last_error_string()
    assert smooth(nd=1) == -4 and smooth(nd=2) == -1 and smooth(H=4096) == -1 and smooth(C=0) == -1
    assert smooth(ns=3) == -4 and smooth(ns=-1) == -4
    assert smooth(ns=0, ws=None, lst=None) == 0                                      # nothing drawn: nothing launched
    n0 = lib.fz_launch_count()
    assert smooth(ns=0) == 0 and lib.fz_launch_count() == n0

    def noise(out=P8, seed=P8, B=1, C=1, V=16):
        return lib.fz_aug_noise_field(out, seed, B, C, V, None)
    assert noise(out=None) == -4 and noise(seed=None) == -4
    assert noise(B=0) == -1 and noise(C=70000) == -1 and noise(V=0) == -1 and noise(V=2 ** 35) == -1
    assert noise(seed=ctypes.c_void_p(4100)) == -4


def test_batch_augment_module_modes():
    aug = ft.BatchAugment(3)
    x, l = K.image((2, 1, 6, 7, 8), 1), K.label((2, 1, 6, 7, 8), 1)
    aug.eval()
    a, b = aug(x, l)
    assert a is x and b is l
    aug.train()
    g = torch.Generator().manual_seed(3)
    a, b = aug(x, l, generator=g)
    g.manual_seed(3)
    c, d = aug(x, l, generator=g)
    assert torch.equal(a, c) and torch.equal(b, d) and a.shape == x.shape and not a.requires_grad
    with pytest.raises(ValueError):
        ft.BatchAugment(2)(x, l)
    with pytest.raises(ValueError):
        ft.BatchAugment(3, sigma_range=((0.5, 1.0),))
