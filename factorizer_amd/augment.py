"""Random training augmentations of the recipe, applied to a whole batch on device.

Every bundle's ``train.yaml`` (model_zoo/factorizer_brats23/configs/train.yaml, ``random_transforms``; 2-D in the FIVES
bundles) lists ``RandAffined`` (prob 0.2, rotate ±0.26 rad, scale ±0.2, bilinear image / nearest label, border padding),
``RandGaussianNoised`` (prob 0.2, std 0.1), ``RandGaussianSmoothd`` (prob 0.2, σ ∈ [0.5, 1] per axis),
``RandScaleIntensityd`` (prob 0.2, factors 0.3), ``RandShiftIntensityd`` (prob 0.2, offsets 0.1) and one ``RandFlipd``
(prob 0.5) per spatial axis.  MONAI is third-party and absent here, and it draws from numpy's ``RandomState`` inside loader
workers, so neither its code nor its random stream is reproduced.  The semantics are **restated**:

A batch is ``image (B, C, *S)`` and optionally ``label (B, L, *S)`` with ``nd = len(S)`` spatial axes.  Every sample ``b``
has one parameter record (`AugmentParams`): ``affine[b]`` (nd × nd, identity = not drawn), ``flip[b]`` (nd booleans),
``noise_std[b]`` (0 = none), ``sigma[b]`` (nd floats, all 0 = no smoothing), ``gain[b]`` (1) and ``offset[b]`` (0).  The
output is defined by four steps per sample, in this order:

1. **resample** (one gather).  For output voxel index ``o`` let ``o' = o`` with ``o'_k = N_k − 1 − o_k`` on flipped axes; the
   source position is ``p = A · (o' − c) + c`` with ``c_k = (N_k − 1) / 2``, clamped per axis to ``[0, N_k − 1]`` (border
   padding).  Image channels take the (bi/tri)linear interpolation at ``p`` (weights and sums in fp32), label channels the
   voxel at ``floor(p + 0.5)``.  ``A = R · diag(s)`` with ``s_k = 1 + U(−scale_range_k, scale_range_k)``; in 3-D
   ``R = Rx(θ0) · Ry(θ1) · Rz(θ2)`` with ``Rx = [[1,0,0],[0,c,−s],[0,s,c]]``, ``Ry = [[c,0,s],[0,1,0],[−s,0,c]]``,
   ``Rz = [[c,−s,0],[s,c,0],[0,0,1]]``; in 2-D ``R = [[c,−s],[s,c]]``.  A sample whose ``A`` is exactly the identity is a pure
   index permutation: its values (bf16 included) and labels come through bit for bit.
2. **noise**: ``image += noise_std[b] · z(b, c, v)``; ``z`` is the counter-based field of `gaussian_noise_field`.
3. **smoothing**: a separable convolution with zero padding along every axis ``k`` with ``sigma[b][k] > 0``; taps
   ``w(x) = max(0, ½ (erf(t (x + ½)) − erf(t (x − ½))))``, ``t = 0.70710678 / σ``, ``x = −tail … tail``,
   ``tail = int(max(4σ, 0.5) + 0.5)``, computed on the host in float64, rounded to fp32 and not renormalised (`gaussian_taps`).
   All channels of a sample share the σ.
4. **intensity**: ``image = image · gain[b] + offset[b]``, one fp32 FMA per voxel.

The recipe applies its flips last; here they are folded into the gather of step 1.  Steps 2 and 4 are pointwise, the noise
is i.i.d. and the smoothing taps are symmetric, so the result has the same distribution, and a volume is read once less.
Label channels see step 1 only.  bf16 images are rounded once, at the final store; every intermediate value is fp32.

**Noise field.**  For sample ``b``, channel ``c`` and flat voxel ``v``: word ``v & 3`` of
``Philox4x32-10((v >> 2, c, b, 0x41554731), (seed lo, seed hi))`` (csrc/fz_philox.h), words turned into normals by two
Box-Muller pairs per counter: ``u_i = ((w_i >> 8) + 0.5) · 2⁻²⁴``, ``(z0, z1) = sqrt(−2 ln u0) · (cos, sin)(2π u1)``,
likewise ``(u2, u3) → (z2, z3)``, with the accurate ``log / sin / cos`` in fp32.  (``n + 0.5`` has 25 significant bits once
``n ≥ 2²³``; fp32 then rounds it to even, a shift of ``u`` by 2⁻²⁵ — below 3·10⁻⁶ in ``z`` unless ``u0`` is within 10⁻⁶ of
1.)  The seed is an int64 that lives on the device, as the dropout seed does: no host sync.

**Paths.**  Device tensors inside the native gate — fp32 / bf16 image, uint8 / bool label, 2 or 3 spatial axes, every
extent ≤ 2048 (and fewer than 2³¹ voxels per channel: the kernels' in-plane offsets are 32-bit) — run the kernels of
csrc/augment.hip: one resample launch for the whole batch (noise, and gain / offset of the samples that do not smooth, ride in
it) and one smoothing launch over the samples that drew one (none: no launch).  CPU tensors run composed framework ops that
implement the same contract, Philox restated with integer tensor ops; device tensors outside the gate (fp16 / fp64, 1-D,
σ ≥ 1.125, i.e. more than 9 taps) run those composed ops on device and say so once.  Nothing here needs autograd; the outputs
do not require grad.

**Random crop.**  The first entry of the recipe's ``random_transforms`` is ``RandSpatialCropd(roi_size, random_size=False)``
with its default ``random_center=True``; restated (MONAI's numpy stream is not reproduced, for the reason given above): per
sample and spatial axis ``k`` an integer origin ``g_k`` uniform in ``[0, N_k − roi_k]`` (`draw_crop_origins`); the sample is
the box ``[g, g + roi)`` of its source, and every step above then runs on that box — step 1 with ``N = roi``, border padding
at the crop's border.  `crop_augment_batch` takes the B sources where they are (ragged shapes, e.g. the
``PreparedVolume.image`` tensors kept in HBM as the bundles' ``CacheDataset(cache_rate=1.0)`` keeps them on the host), and

    crop_augment_batch([x_i], [l_i], g, roi, params) == augment_batch(stack(x_i[box_i]), stack(l_i[box_i]), params)

bit for bit on every path: the positions of step 1 are formed in crop coordinates and clamped to ``[0, roi_k − 1]`` by the
same arithmetic, the integer origin is added to the integer corner indices afterwards, no voxel outside a box is read, and
the noise counter stays the flat OUTPUT voxel.  Natively (csrc/aug_crop.hip) the crop costs the gather a base pointer, two
strides and three offsets per sample, which travel with the records in the one host-to-device copy of the batch: one launch,
plus the smoothing launch if a sample drew one.  The gate is `augment_batch`'s on the roi and the dtypes, plus: every source
contiguous (made so otherwise, with a one-time warning: a full copy of that source per call), every source plane below 2³¹
voxels, B and the plane counts within the grid limits.  Outside it the boxes are sliced and stacked and `augment_batch`'s
paths take over.  `RandCropAugment` is the module: crop origins first, then the records, from one generator.
"""
from __future__ import annotations

import math
from dataclasses import dataclass

import torch

from . import _native as N
from . import composed
from . import functional as Fn

MAX_AXIS = 2048          # native gate: extent per axis
MAX_TAIL = 4             # native gate: 9 taps, sigma < 1.125
NOISE_STREAM = 0x41554731
_MASK32 = 0xFFFFFFFF


# ---- parameter records ------------------------------------------------------------------------------------------------------
@dataclass
class AugmentParams:
    """Per-sample records of one batch, CPU tensors: ``affine`` (B, nd, nd) fp32, ``flip`` (B, nd) bool, ``noise_std`` (B,),
    ``sigma`` (B, nd), ``gain`` (B,), ``offset`` (B,) fp32; ``seed``: the noise seed, a Python int in [0, 2⁶³) or an int64
    tensor of one element (a device tensor is used where it is)."""
    affine: torch.Tensor
    flip: torch.Tensor
    noise_std: torch.Tensor
    sigma: torch.Tensor
    gain: torch.Tensor
    offset: torch.Tensor
    seed: object = 0

    @property
    def batch(self) -> int:
        return int(self.affine.shape[0])

    @property
    def spatial_dims(self) -> int:
        return int(self.affine.shape[-1])

    @staticmethod
    def identity(B: int, spatial_dims: int, seed=0) -> "AugmentParams":
        """the records of a batch in which nothing was drawn"""
        nd = int(spatial_dims)
        return AugmentParams(affine=torch.eye(nd, dtype=torch.float32).repeat(B, 1, 1),
                             flip=torch.zeros(B, nd, dtype=torch.bool), noise_std=torch.zeros(B), sigma=torch.zeros(B, nd),
                             gain=torch.ones(B), offset=torch.zeros(B), seed=seed)


def _per_axis(v, nd, name):
    if isinstance(v, (int, float)):
        return (float(v),) * nd
    t = tuple(float(x) for x in v)
    if len(t) != nd:
        raise ValueError(f"{name} needs one value per axis ({nd}), got {t}")
    return t


def rotation_matrix(angles, spatial_dims: int) -> torch.Tensor:
    """float64 R of the module docstring: 3-D ``Rx(θ0) · Ry(θ1) · Rz(θ2)`` from three angles, 2-D ``[[c,−s],[s,c]]`` from one"""
    if spatial_dims == 2:
        c, s = math.cos(angles[0]), math.sin(angles[0])
        return torch.tensor([[c, -s], [s, c]], dtype=torch.float64)
    if spatial_dims != 3:
        raise ValueError("rotations exist for 2 or 3 spatial axes")
    (c0, s0), (c1, s1), (c2, s2) = ((math.cos(a), math.sin(a)) for a in angles)
    rx = torch.tensor([[1, 0, 0], [0, c0, -s0], [0, s0, c0]], dtype=torch.float64)
    ry = torch.tensor([[c1, 0, s1], [0, 1, 0], [-s1, 0, c1]], dtype=torch.float64)
    rz = torch.tensor([[c2, -s2, 0], [s2, c2, 0], [0, 0, 1]], dtype=torch.float64)
    return rx @ ry @ rz


def affine_matrix(angles, scales, spatial_dims: int) -> torch.Tensor:
    """``A = R · diag(s)`` formed in float64, rounded to fp32 (the precision of the records)"""
    nd = int(spatial_dims)
    s = torch.tensor(_per_axis(scales, nd, "scales"), dtype=torch.float64)
    r = rotation_matrix(tuple(angles), nd) if nd > 1 else torch.ones(1, 1, dtype=torch.float64)
    return (r * s[None, :]).to(torch.float32)


def draw_augment_params(B: int, spatial_dims: int, *, affine_prob=0.2, rotate_range=0.26, scale_range=0.2, noise_prob=0.2,
                        noise_std=0.1, smooth_prob=0.2, sigma_range=None, scale_intensity_prob=0.2, factors=0.3,
                        shift_intensity_prob=0.2, offsets=0.1, flip_prob=0.5, flip_axes=None, sample_std=True,
                        generator=None) -> AugmentParams:
    """Draw the records of a batch of ``B`` samples on the host from the CPU ``generator`` (None: torch's default CPU
    generator).  Per sample, each with its own probability: an affine matrix (rotation angles ``U(−rotate_range_k,
    rotate_range_k)`` — three in 3-D, one in 2-D, none in 1-D — and scales ``1 + U(−scale_range_k, scale_range_k)``), a noise
    std (``U(0, noise_std)`` as MONAI's ``sample_std=True`` default does, or ``noise_std`` itself), one σ per axis from
    ``sigma_range`` (default ``(0.5, 1.0)`` per axis), a gain ``1 + U(−factors, factors)``, an offset ``U(−offsets,
    offsets)``, and a flip per axis of ``flip_axes`` (default: every spatial axis).  What is not drawn keeps its identity value.
    All uniforms of a batch come from ONE ``torch.rand`` call and the seed from one ``torch.randint``, so a generator state
    determines the records."""
    nd = int(spatial_dims)
    if nd < 1 or nd > 3:
        raise ValueError("1 to 3 spatial axes")
    nrot = {1: 0, 2: 1, 3: 3}[nd]
    rot = _per_axis(rotate_range, nrot, "rotate_range") if nrot else ()
    sc = _per_axis(scale_range, nd, "scale_range")
    if sigma_range is None:
        sigma_range = ((0.5, 1.0),) * nd
    sigma_range = tuple((float(lo), float(hi)) for lo, hi in sigma_range)
    if len(sigma_range) != nd:
        raise ValueError(f"sigma_range needs one (low, high) pair per axis ({nd})")
    axes = tuple(range(nd)) if flip_axes is None else tuple(int(a) for a in flip_axes)
    if any(a < 0 or a >= nd for a in axes):
        raise ValueError(f"flip_axes must name spatial axes 0 .. {nd - 1}")
    # columns of the uniform matrix
    k_aff, k_rot, k_sc = 0, 1, 1 + nrot
    k_noise = k_sc + nd
    k_smooth = k_noise + 2
    k_gain = k_smooth + 1 + nd
    k_shift = k_gain + 2
    k_flip = k_shift + 2
    u = torch.rand(B, k_flip + nd, generator=generator, dtype=torch.float64)
    seed = int(torch.randint(0, 2 ** 62, (1,), generator=generator, dtype=torch.int64))
    p = AugmentParams.identity(B, nd, seed)
    ul = u.tolist()
    for b in range(B):
        r = ul[b]
        if r[k_aff] < affine_prob:
            angles = [(2 * r[k_rot + j] - 1) * rot[j] for j in range(nrot)]
            scales = [1 + (2 * r[k_sc + j] - 1) * sc[j] for j in range(nd)]
            p.affine[b] = affine_matrix(angles, scales, nd)
        if r[k_noise] < noise_prob:
            p.noise_std[b] = r[k_noise + 1] * noise_std if sample_std else noise_std
        if r[k_smooth] < smooth_prob:
            p.sigma[b] = torch.tensor([lo + r[k_smooth + 1 + j] * (hi - lo) for j, (lo, hi) in enumerate(sigma_range)])
        if r[k_gain] < scale_intensity_prob:
            p.gain[b] = 1 + (2 * r[k_gain + 1] - 1) * factors
        if r[k_shift] < shift_intensity_prob:
            p.offset[b] = (2 * r[k_shift + 1] - 1) * offsets
        for a in axes:
            p.flip[b, a] = r[k_flip + a] < flip_prob
    return p


# ---- taps -------------------------------------------------------------------------------------------------------------------
def gaussian_tail(sigma: float) -> int:
    return int(max(4.0 * float(sigma), 0.5) + 0.5)


def gaussian_taps(sigma: float) -> torch.Tensor:
    """the ``2 · tail + 1`` fp32 taps of step 3 for one σ > 0 (float64 erf differences, clipped at 0, not renormalised)"""
    sigma = float(sigma)
    if not sigma > 0:
        raise ValueError("sigma must be positive")
    tail = gaussian_tail(sigma)
    t = 0.70710678 / sigma
    w = [max(0.0, 0.5 * (math.erf(t * (x + 0.5)) - math.erf(t * (x - 0.5)))) for x in range(-tail, tail + 1)]
    return torch.tensor(w, dtype=torch.float64).to(torch.float32)


def native_sigma_ok(sigma) -> bool:
    """every σ of the records is 0 (axis not smoothed) or needs at most 9 taps (tail ≤ 4, σ < 1.125)"""
    return all(s <= 0 or gaussian_tail(s) <= MAX_TAIL for s in torch.as_tensor(sigma, dtype=torch.float64).flatten().tolist())


# ---- noise field -------------------------------------------------------------------------------------------------------------
def _philox4x32_10(c0, c1, c2, c3, k0, k1):
    """Philox4x32-10 over int64 tensors that hold 32-bit words (csrc/fz_philox.h restated: the 64-bit products wrap in
    int64, which keeps their bit pattern; the arithmetic shift's sign bits are masked off)"""
    m0, m1 = 0xD2511F53, 0xCD9E8D57
    for _ in range(10):
        p0, p1 = c0 * m0, c2 * m1
        c0, c1, c2, c3 = ((p1 >> 32) & _MASK32) ^ c1 ^ k0, p1 & _MASK32, ((p0 >> 32) & _MASK32) ^ c3 ^ k1, p0 & _MASK32
        k0 = (k0 + 0x9E3779B9) & _MASK32
        k1 = (k1 + 0xBB67AE85) & _MASK32
    return c0, c1, c2, c3


def _seed_tensor(seed, device):
    """int64 (1,) on `device`; a Python int is uploaded (no sync), a tensor moved only if it lives elsewhere"""
    if torch.is_tensor(seed):
        return seed.reshape(1).to(device=device, dtype=torch.int64)
    return torch.tensor([int(seed)], dtype=torch.int64, device=device)


def _noise_composed(B, C, V, seed_t):
    """the field with integer / fp32 tensor ops on seed_t's device, (B, C, V) fp32"""
    dev = seed_t.device
    k0, k1 = seed_t & _MASK32, (seed_t >> 32) & _MASK32
    nq = (V + 3) // 4
    q = torch.arange(nq, dtype=torch.int64, device=dev).expand(B, C, nq)
    c = torch.arange(C, dtype=torch.int64, device=dev)[None, :, None].expand(B, C, nq)
    b = torch.arange(B, dtype=torch.int64, device=dev)[:, None, None].expand(B, C, nq)
    w = _philox4x32_10(q, c, b, torch.full_like(q, NOISE_STREAM), k0, k1)
    u = [((x >> 8).to(torch.float32) + 0.5) * (2.0 ** -24) for x in w]
    z = []
    for i in (0, 2):
        r = torch.sqrt(-2.0 * torch.log(u[i]))
        a = 6.283185307179586 * u[i + 1]
        z += [r * torch.cos(a), r * torch.sin(a)]
    return torch.stack(z, dim=-1).reshape(B, C, 4 * nq)[..., :V].contiguous()


def gaussian_noise_field(shape, seed, device=None) -> torch.Tensor:
    """fp32 tensor ``shape = (B, C, *S)`` of the normals ``z(b, c, v)`` of the module docstring.  ``seed``: an int or an int64
    tensor.  A device runs fz_aug_noise_field, the CPU the restated tensor ops."""
    shape = tuple(int(s) for s in shape)
    if len(shape) < 3:
        raise ValueError("shape must be (B, C, *S)")
    if device is None:
        device = seed.device if torch.is_tensor(seed) else "cpu"
    device = torch.device(device)
    B, C = shape[:2]
    V = math.prod(shape[2:])
    st = _seed_tensor(seed, device)
    if B * C * V == 0:
        return torch.empty(shape, dtype=torch.float32, device=device)
    if device.type == "cuda":
        return Fn.aug_noise_field(st, B, C, V).reshape(shape)
    return _noise_composed(B, C, V, st).reshape(shape)


# ---- composed path ----------------------------------------------------------------------------------------------------------
def _source_positions(A, flip, spatial, dtype, device):
    """clamped source positions of every output voxel: a list of nd tensors shaped like the image"""
    nd = len(spatial)
    grids = []
    for k, n in enumerate(spatial):
        o = torch.arange(n, dtype=dtype, device=device)
        if bool(flip[k]):
            o = (n - 1) - o
        grids.append((o - (n - 1) / 2).reshape([-1 if j == k else 1 for j in range(nd)]))
    pos = []
    for k, n in enumerate(spatial):
        p = sum(float(A[k, j]) * grids[j] for j in range(nd)) + (n - 1) / 2
        pos.append(p.expand(spatial).clamp(0, n - 1))
    return pos


def _resample_composed(x, lab, A, flip, ct):
    """step 1 of one sample: x (C, *S) or None -> ct values, lab (L, *S) or None -> same dtype"""
    ref = x if x is not None else lab
    spatial = tuple(ref.shape[1:])
    nd = len(spatial)
    identity = torch.equal(A.to(torch.float64), torch.eye(nd, dtype=torch.float64))
    if identity:
        dims = [1 + k for k in range(nd) if bool(flip[k])]
        fl = (lambda t: torch.flip(t, dims)) if dims else (lambda t: t.clone())
        return (fl(x).to(ct) if x is not None else None), (fl(lab) if lab is not None else None)
    pos = _source_positions(A, flip, spatial, ct, ref.device)
    out_x = out_l = None
    if lab is not None:
        idx = tuple(torch.floor(p + 0.5).to(torch.int64) for p in pos)
        out_l = lab[(slice(None),) + idx]
    if x is not None:
        xs = x.to(ct)
        i0 = [torch.floor(p).to(torch.int64) for p in pos]
        f = [p - i.to(ct) for p, i in zip(pos, i0)]
        i1 = [torch.clamp(i + 1, max=n - 1) for i, n in zip(i0, spatial)]
        out_x = torch.zeros((x.shape[0],) + spatial, dtype=ct, device=x.device)
        for corner in range(1 << nd):
            w = torch.ones(spatial, dtype=ct, device=x.device)
            idx = []
            for k in range(nd):
                hi = (corner >> k) & 1
                idx.append(i1[k] if hi else i0[k])
                w = w * (f[k] if hi else 1 - f[k])
            out_x += w * xs[(slice(None),) + tuple(idx)]
    return out_x, out_l


def _smooth_composed(x, sigma):
    """step 3 of one sample: x (C, *S) in its compute dtype; zero padding, one pass per axis with sigma > 0"""
    nd = x.dim() - 1
    for k in range(nd):
        s = float(sigma[k])
        if s <= 0:
            continue
        w = gaussian_taps(s).tolist()
        tail = (len(w) - 1) // 2
        n = x.shape[1 + k]
        pad = [0, 0] * nd
        pad[2 * (nd - 1 - k)] = pad[2 * (nd - 1 - k) + 1] = tail
        xp = torch.nn.functional.pad(x, pad)
        acc = torch.zeros_like(x)
        for j, wj in enumerate(w):
            acc += wj * xp.narrow(1 + k, j, n)
        x = acc
    return x


def _augment_composed(image, label, params):
    ref = image if image is not None else label
    B = ref.shape[0]
    dev = ref.device
    out_i = out_l = None
    if image is not None:
        ct = torch.float64 if image.dtype == torch.float64 else torch.float32
        out_i = torch.empty_like(image)
        noise = None
        if bool((params.noise_std > 0).any()):
            noise = gaussian_noise_field_composed(image.shape, params.seed, dev)
    if label is not None:
        out_l = torch.empty_like(label)
    for b in range(B):
        x, l = _resample_composed(image[b] if image is not None else None, label[b] if label is not None else None,
                                  params.affine[b], params.flip[b], ct if image is not None else torch.float32)
        if l is not None:
            out_l[b] = l
        if x is None:
            continue
        std, g, o = float(params.noise_std[b]), float(params.gain[b]), float(params.offset[b])
        if std > 0:
            x = x + std * noise[b].to(ct)
        if bool((params.sigma[b] > 0).any()):
            x = _smooth_composed(x, params.sigma[b])
        if g != 1.0 or o != 0.0:
            x = x * g + o
        out_i[b] = x.to(image.dtype)
    return out_i, out_l


def gaussian_noise_field_composed(shape, seed, device):
    """the field through the restated tensor ops on any device (what the composed path adds)"""
    shape = tuple(int(s) for s in shape)
    return _noise_composed(shape[0], shape[1], math.prod(shape[2:]), _seed_tensor(seed, torch.device(device))).reshape(shape)


# ---- native path -------------------------------------------------------------------------------------------------------------
REC = 48   # include/factorizer_hip.h: fz_aug_record_floats()


def _records(params: AugmentParams, nd: int):
    """(table, list) of one batch as ONE CPU fp32 tensor of B · REC + B words (the index list rides behind the records as
    int32 bit patterns), and the number of smoothing samples"""
    B = params.batch
    buf = torch.zeros(B * REC + B, dtype=torch.float32)
    t = buf[:B * REC].view(B, REC)
    pad = 3 - nd
    A = torch.eye(3, dtype=torch.float32).repeat(B, 1, 1)
    A[:, pad:, pad:] = params.affine.to(torch.float32)
    t[:, 0:9] = A.reshape(B, 9)
    t[:, 9 + pad:12] = params.flip.to(torch.float32)
    t[:, 12] = params.noise_std.to(torch.float32)
    t[:, 13] = params.gain.to(torch.float32)
    t[:, 14] = params.offset.to(torch.float32)
    t[:, 15] = -1.0
    listed = []
    sig = params.sigma.to(torch.float64).tolist()
    for b in range(B):
        if any(s > 0 for s in sig[b]):
            t[b, 15] = float(len(listed))
            listed.append(b)
            for k, s in enumerate(sig[b]):
                if s > 0:
                    w = gaussian_taps(s)
                    tail = (w.numel() - 1) // 2
                    t[b, 16 + pad + k] = float(tail)
                    t[b, 19 + 9 * (pad + k) + 4 - tail:19 + 9 * (pad + k) + 5 + tail] = w
    if listed:
        buf[B * REC:].view(torch.int32)[:len(listed)] = torch.tensor(listed, dtype=torch.int32)
    return buf, len(listed)


def _outside_gate(B, planes, spatial, image_dtype, label_dtype, params):
    """why a batch of B samples x `planes` planes of the spatial shape `spatial` (the OUTPUT geometry) is outside the native
    kernel set, or None; a dtype of None: no such tensor"""
    nd = len(spatial)
    if nd not in (2, 3):
        return f"{nd} spatial axis"
    if image_dtype is not None and image_dtype not in (torch.float32, torch.bfloat16):
        return f"{image_dtype} image"
    if label_dtype is not None and label_dtype not in (torch.uint8, torch.bool):
        return f"{label_dtype} label"
    if max(spatial) > MAX_AXIS or math.prod(spatial) >= 2 ** 31:
        return f"spatial shape {tuple(spatial)}"
    if B > 65535 or planes > 65535:
        return "more than 65535 samples or planes"
    if params is not None and not native_sigma_ok(params.sigma):
        return "a sigma of 1.125 or more (over 9 taps)"
    return None


def _gate(image, label, params, what):
    """True: the native kernels take this call.  False: composed (announced once where the tensors are on a device)."""
    ref = image if image is not None else label
    if not ref.is_cuda or ref.numel() == 0:
        return False
    why = _outside_gate(ref.shape[0], (0 if image is None else image.shape[1]) + (0 if label is None else label.shape[1]),
                        tuple(ref.shape[2:]), None if image is None else image.dtype, None if label is None else label.dtype,
                        params)
    if why is None:
        return True
    composed.warn_once(f"augment:{what}:{why}", f"{what}: {why} is outside the native kernel set (fp32 / bf16 image, uint8 / "
                       "bool label, 2 or 3 spatial axes of at most 2048, sigma < 1.125): composed framework ops")
    return False


def _check(image, label, params):
    ref = image if image is not None else label
    if ref is None:
        raise ValueError("neither image nor label given")
    if ref.dim() < 3 or ref.dim() > 5:
        raise ValueError("augmentations take (B, C, *S) tensors with 1, 2 or 3 spatial axes")
    if image is not None and label is not None and (image.shape[0] != label.shape[0] or image.shape[2:] != label.shape[2:]):
        raise ValueError(f"image {tuple(image.shape)} and label {tuple(label.shape)} differ in batch or spatial shape")
    if image is not None and not image.is_floating_point():
        raise TypeError(f"the image must be a floating-point tensor, got {image.dtype}")
    if image is not None and label is not None and image.device != label.device:
        raise ValueError("image and label live on different devices")
    _check_records(params, ref.shape[0], ref.dim() - 2)


def _check_records(params, B, nd):
    if params.batch != B or params.spatial_dims != nd:
        raise ValueError(f"records for B = {params.batch}, nd = {params.spatial_dims}; tensors have B = {B}, nd = {nd}")
    for name, shape in (("flip", (params.batch, nd)), ("noise_std", (params.batch,)), ("sigma", (params.batch, nd)),
                        ("gain", (params.batch,)), ("offset", (params.batch,))):
        if tuple(getattr(params, name).shape) != shape:
            raise ValueError(f"params.{name} must have shape {shape}")


def augment_batch(image, label, params: AugmentParams):
    """Apply the records ``params`` to ``image (B, C, *S)`` and / or ``label (B, L, *S)`` (either may be None) as the module
    docstring defines; returns ``(image, label)`` as new tensors of the same dtypes.  Deterministic: the same tensors, records
    and seed give bitwise the same result."""
    _check(image, label, params)
    return _run(image, label, params, _gate(image, label, params, "augment_batch"))


def _run(image, label, params, native):
    """the checked call on the path its gate chose"""
    if not native:
        with torch.no_grad():
            return _augment_composed(image, label, params)
    ref = image if image is not None else label
    nd = ref.dim() - 2
    buf, ns = _records(params, nd)
    dev_buf = buf.to(ref.device, non_blocking=True)        # the one host-to-device copy of the batch
    seed = None
    if image is not None and bool((params.noise_std > 0).any()):
        seed = _seed_tensor(params.seed, ref.device)
    with torch.no_grad():
        return Fn.aug_apply(image.contiguous() if image is not None else None,
                            label.contiguous() if label is not None else None, dev_buf, params.batch * REC, ns, seed)


def affine_resample(image, label=None, affine=None, flip=None):
    """Step 1 alone: ``affine`` (B, nd, nd) (None: identity), ``flip`` (B, nd) bool (None: no flips).  Returns (image, label)."""
    ref = image if image is not None else label
    B, nd = ref.shape[0], ref.dim() - 2
    p = AugmentParams.identity(B, nd)
    if affine is not None:
        p.affine = torch.as_tensor(affine).detach().to("cpu", torch.float32).reshape(B, nd, nd)
    if flip is not None:
        p.flip = torch.as_tensor(flip).to("cpu", torch.bool).reshape(B, nd)
    return augment_batch(image, label, p)


def gaussian_smooth(image, sigma):
    """Step 3 alone: ``sigma`` (B, nd), (nd,) or a scalar; an entry of 0 leaves that axis alone."""
    B, nd = image.shape[0], image.dim() - 2
    p = AugmentParams.identity(B, nd)
    s = torch.as_tensor(sigma, dtype=torch.float32).detach().cpu()
    p.sigma = s.expand(B, nd).clone() if s.dim() < 2 else s.reshape(B, nd).clone()
    return augment_batch(image, None, p)[0]


# ---- random crop inside the gather -----------------------------------------------------------------------------------------
SRC = 8    # include/factorizer_hip.h: fz_aug_source_words()


def _roi(roi_size, nd):
    roi = (int(roi_size),) * nd if isinstance(roi_size, int) else tuple(int(r) for r in roi_size)
    if len(roi) != nd or min(roi) < 1:
        raise ValueError(f"roi_size needs one positive extent per spatial axis ({nd}), got {roi_size}")
    return roi


def draw_crop_origins(shapes, roi_size, generator=None) -> torch.Tensor:
    """The origins of ``RandSpatialCropd(roi_size, random_size=False)`` for a batch: int64 CPU tensor ``(B, nd)``, origin ``k``
    of sample ``b`` uniform over the integers ``[0, N_k − roi_k]``.  ``shapes``: B spatial shapes; a tensor ``(C, *S)`` or
    ``(1, C, *S)`` stands for its ``S`` (the last ``len(roi_size)`` axes; an int ``roi_size`` needs shapes, not tensors).  All
    origins come from ONE ``torch.rand`` call in float64 on the CPU ``generator`` (None: torch's default), ``g = floor(u · (N −
    roi + 1))``, so a generator state determines them; ``roi_k == N_k`` gives 0, ``roi_k > N_k`` raises."""
    shapes = list(shapes)
    if not shapes:
        raise ValueError("no shapes given")
    if isinstance(roi_size, int):
        if any(torch.is_tensor(sh) for sh in shapes):
            raise ValueError("an int roi_size needs spatial shapes (a tensor's spatial axes are counted by len(roi_size))")
        nd = len(shapes[0])
    else:
        nd = len(tuple(roi_size))
    roi = _roi(roi_size, nd)
    sp = []
    for b, sh in enumerate(shapes):
        t = tuple(int(n) for n in (sh.shape[-nd:] if torch.is_tensor(sh) else sh))
        if len(t) != nd:
            raise ValueError(f"sample {b}: spatial shape {t} does not have {nd} axes")
        for k in range(nd):
            if roi[k] > t[k]:
                raise ValueError(f"sample {b}, axis {k}: roi {roi[k]} exceeds the extent {t[k]} (pad the volume to the roi first)")
        sp.append(t)
    free = torch.tensor(sp, dtype=torch.float64) - torch.tensor(roi, dtype=torch.float64)     # N - roi, (B, nd)
    u = torch.rand(len(sp), nd, generator=generator, dtype=torch.float64)
    return torch.minimum(torch.floor(u * (free + 1)), free).to(torch.int64)


def _crop_sources(images, labels, origins, roi_size):
    """checked views of one batch: (images, labels) as lists of (C, *S_i) / (L, *S_i) tensors or None, origins as a list of
    B tuples, roi"""
    origins = torch.as_tensor(origins).detach().to("cpu", torch.int64)
    if origins.dim() != 2:
        raise ValueError("origins must be (B, nd)")
    B, nd = origins.shape
    if nd < 1 or nd > 3:
        raise ValueError("1 to 3 spatial axes")
    roi = _roi(roi_size, nd)
    if images is None and labels is None:
        raise ValueError("neither images nor labels given")
    out = []
    for name, seq in (("image", images), ("label", labels)):
        if seq is None:
            out.append(None)
            continue
        seq = list(seq)
        if len(seq) != B:
            raise ValueError(f"{len(seq)} {name}s for {B} origins")
        ts = []
        for b, t in enumerate(seq):
            if t.dim() == nd + 2 and t.shape[0] == 1:
                t = t[0]                                                  # PreparedVolume.image is (1, C, *P)
            if t.dim() != nd + 1:
                raise ValueError(f"{name} {b}: expected (C, *S) or (1, C, *S) with {nd} spatial axes, got {tuple(t.shape)}")
            if ts and t.shape[0] != ts[0].shape[0]:
                raise ValueError(f"{name} {b} has {t.shape[0]} channels, {name} 0 has {ts[0].shape[0]}")
            if ts and (t.dtype != ts[0].dtype or t.device != ts[0].device):
                raise ValueError(f"{name} {b} is {t.dtype} on {t.device}, {name} 0 is {ts[0].dtype} on {ts[0].device}")
            ts.append(t)
        out.append(ts)
    imgs, labs = out
    if imgs is not None and not imgs[0].is_floating_point():
        raise TypeError(f"the images must be floating-point tensors, got {imgs[0].dtype}")
    if imgs is not None and labs is not None:
        if imgs[0].device != labs[0].device:
            raise ValueError("images and labels live on different devices")
        for b in range(B):
            if imgs[b].shape[1:] != labs[b].shape[1:]:
                raise ValueError(f"sample {b}: image {tuple(imgs[b].shape)} and label {tuple(labs[b].shape)} differ in "
                                 "spatial shape")
    g = [tuple(row) for row in origins.tolist()]
    for b, t in enumerate(imgs if imgs is not None else labs):
        for k in range(nd):
            if g[b][k] < 0 or g[b][k] + roi[k] > t.shape[1 + k]:
                raise ValueError(f"sample {b}, axis {k}: box [{g[b][k]}, {g[b][k] + roi[k]}) leaves the extent {t.shape[1 + k]}")
    return imgs, labs, g, roi


def _crop_table(imgs, labs, g, roi):
    """the source table of one batch: int64 CPU tensor (B, SRC) = image address, label address (0: none), the three source
    extents, the three origins — 2-D lifted with a leading extent 1 / origin 0 (layout: include/factorizer_hip.h)"""
    ref = imgs if imgs is not None else labs
    pad = 3 - len(roi)
    rows = [[imgs[b].data_ptr() if imgs is not None else 0, labs[b].data_ptr() if labs is not None else 0,
             *((1,) * pad + tuple(ref[b].shape[1:])), *((0,) * pad + tuple(g[b]))] for b in range(len(ref))]
    return torch.tensor(rows, dtype=torch.int64)


def source_vector_loads(table, roi, image_bytes=4):
    """Which samples of a source table (`_crop_table`) the kernel reads with vector loads on the identity path, restating
    csrc/aug_crop.hip: bool (B, 2) for (image, label).  The output side must allow vectors at all (roi W a multiple of 4);
    then every lane's first element must sit on a 4-byte boundary: always for fp32, origin x and source W even and the base
    4-byte aligned for bf16, all three multiples of 4 for the one-byte label."""
    t = torch.as_tensor(table, dtype=torch.int64)
    per = 4 // int(image_bytes)                                           # elements per 4 bytes
    out = torch.full((t.shape[0],), int(roi[-1]) % 4 == 0)
    img = out & (t[:, 0] != 0) & (t[:, 7] % per == 0) & (t[:, 4] % per == 0) & (t[:, 0] % 4 == 0)
    lab = out & (t[:, 1] != 0) & (t[:, 7] % 4 == 0) & (t[:, 4] % 4 == 0) & (t[:, 1] % 4 == 0)
    return torch.stack([img, lab], dim=1)


def _box(t, g, roi):
    return t[(slice(None),) + tuple(slice(o, o + r) for o, r in zip(g, roi))]


def crop_augment_batch(images, labels, origins, roi_size, params: AugmentParams = None):
    """Cut the box ``[origins[b], origins[b] + roi_size)`` out of every sample's own source and apply the records ``params``
    to the batch of boxes, as the module docstring defines: returns ``(image (B, C, *roi), label (B, L, *roi))``, bit for bit
    what `augment_batch` gives on the stacked boxes.  ``images`` / ``labels``: sequences of B tensors ``(C, *S_b)`` or
    ``(1, C, *S_b)`` (either may be None; a tensor may appear more than once); ``origins``: integers ``(B, nd)``, e.g. from
    `draw_crop_origins`; ``params=None``: identity records, i.e. a pure batched crop.  Sources and the call share the current
    stream."""
    imgs, labs, g, roi = _crop_sources(images, labels, origins, roi_size)
    ref = imgs if imgs is not None else labs
    B, nd = len(ref), len(roi)
    if params is None:
        params = AugmentParams.identity(B, nd)
    C = imgs[0].shape[0] if imgs is not None else 0
    L = labs[0].shape[0] if labs is not None else 0
    idt = imgs[0].dtype if imgs is not None else None
    ldt = labs[0].dtype if labs is not None else None
    native = ref[0].is_cuda and (C + L) * math.prod(roi) > 0
    if native:
        why = _outside_gate(B, C + L, roi, idt, ldt, params)
        if why is None and any(math.prod(t.shape[1:]) >= 2 ** 31 for t in ref):
            why = "a source plane of 2^31 voxels or more"
            composed.warn_once(f"augment:crop_augment_batch:{why}", f"crop_augment_batch: {why} is outside the native crop "
                               "kernel (32-bit in-plane offsets): the boxes are sliced and stacked first")
        native = why is None
    if not native:
        image = torch.stack([_box(t, g[b], roi) for b, t in enumerate(imgs)]) if imgs is not None else None
        label = torch.stack([_box(t, g[b], roi) for b, t in enumerate(labs)]) if labs is not None else None
        _check(image, label, params)
        return _run(image, label, params, _gate(image, label, params, "crop_augment_batch"))
    _check_records(params, B, nd)
    if not all(t.is_contiguous() for seq in (imgs, labs) if seq is not None for t in seq):
        composed.warn_once("augment:crop_augment_batch:contiguous", "crop_augment_batch: a source is not contiguous and is "
                           "copied whole on every call (one read and one write of the full volume); keep the prepared volumes "
                           "contiguous")
        imgs = [t.contiguous() for t in imgs] if imgs is not None else None
        labs = [t.contiguous() for t in labs] if labs is not None else None
    rec, ns = _records(params, nd)
    table = _crop_table(imgs, labs, g, roi)
    buf = torch.empty(2 * SRC * B + rec.numel(), dtype=torch.float32)
    buf[:2 * SRC * B].view(torch.int64).copy_(table.reshape(-1))          # the table first: its words are 8-byte aligned
    buf[2 * SRC * B:].view(torch.int32).copy_(rec.view(torch.int32))
    dev = ref[0].device
    dev_buf = buf.to(dev, non_blocking=True)                               # still the one host-to-device copy of the batch
    seed = None
    if imgs is not None and bool((params.noise_std > 0).any()):
        seed = _seed_tensor(params.seed, dev)
    with torch.no_grad():                                                  # imgs / labs stay referenced until the launches are enqueued
        return Fn.aug_crop_apply(dev_buf, 2 * SRC * B, B * REC, ns, seed, roi, C, L, idt, ldt)


class BatchAugment(torch.nn.Module):
    """The recipe's ``random_transforms`` for a whole batch: ``aug(image, label=None, generator=None)`` draws one record per
    sample (`draw_augment_params`; ``generator``: a CPU ``torch.Generator``) and applies it (`augment_batch`), returning
    ``(image, label)``.  The defaults are the recipe's.  In ``eval()`` mode it is the identity and returns the same objects.

        aug = ft.BatchAugment(3)
        for image, label in loader:                       # the loaders only load, crop and stack (`RandCropAugment`
                                                          # crops volumes that are already on the device)
            image, label = aug(image.cuda(non_blocking=True), label.cuda(non_blocking=True))
            loss = loss_fn(model(image), label)
    """

    def __init__(self, spatial_dims, affine_prob=0.2, rotate_range=0.26, scale_range=0.2, noise_prob=0.2, noise_std=0.1,
                 smooth_prob=0.2, sigma_range=None, scale_intensity_prob=0.2, factors=0.3, shift_intensity_prob=0.2,
                 offsets=0.1, flip_prob=0.5, flip_axes=None, sample_std=True):
        super().__init__()
        self.spatial_dims = int(spatial_dims)
        self.kwargs = dict(affine_prob=affine_prob, rotate_range=rotate_range, scale_range=scale_range, noise_prob=noise_prob,
                           noise_std=noise_std, smooth_prob=smooth_prob, sigma_range=sigma_range,
                           scale_intensity_prob=scale_intensity_prob, factors=factors,
                           shift_intensity_prob=shift_intensity_prob, offsets=offsets, flip_prob=flip_prob, flip_axes=flip_axes,
                           sample_std=sample_std)
        draw_augment_params(1, self.spatial_dims, generator=torch.Generator().manual_seed(0), **self.kwargs)   # validates

    def forward(self, image, label=None, generator=None):
        if not self.training:
            return image, label
        if image.dim() - 2 != self.spatial_dims:
            raise ValueError(f"BatchAugment({self.spatial_dims}) got a tensor with {image.dim() - 2} spatial axes")
        params = draw_augment_params(image.shape[0], self.spatial_dims, generator=generator, **self.kwargs)
        return augment_batch(image, label, params)

    def extra_repr(self):
        return f"spatial_dims={self.spatial_dims}, " + ", ".join(f"{k}={v}" for k, v in self.kwargs.items())


class RandCropAugment(torch.nn.Module):
    """The recipe's whole ``random_transforms`` list, the leading ``RandSpatialCropd(roi_size, random_size=False)`` included,
    on sources that already sit on the device: ``aug(images, labels=None, generator=None)`` takes B tensors ``(C, *S_b)`` or
    ``(1, C, *S_b)`` of any sizes ≥ roi, draws the crop origins (`draw_crop_origins`) and THEN one record per sample
    (`draw_augment_params`) from the same CPU ``generator``, and applies both in one gather (`crop_augment_batch`), returning
    ``(image (B, C, *roi), label (B, L, *roi))``.  The keyword arguments are `BatchAugment`'s.  In ``eval()`` mode it takes the
    centred box ``g_k = (N_k − roi_k) // 2`` with identity records.

        cache = [ft.prepare_volume(x, l, roi_size=roi) for x, l in subjects]         # prepared volumes stay in HBM
        aug = ft.RandCropAugment(3, roi)
        for idx in batches:
            image, label = aug([cache[i].image for i in idx], [cache[i].label for i in idx])
            loss = loss_fn(model(image), label)
    """

    def __init__(self, spatial_dims, roi_size, **kwargs):
        super().__init__()
        self.spatial_dims = int(spatial_dims)
        self.roi_size = _roi(roi_size, self.spatial_dims)
        self.kwargs = BatchAugment(self.spatial_dims, **kwargs).kwargs       # the same defaults, validated the same way

    def forward(self, images, labels=None, generator=None):
        ref = list(images if images is not None else labels)
        if self.training:
            origins = draw_crop_origins(ref, self.roi_size, generator)
            params = draw_augment_params(len(ref), self.spatial_dims, generator=generator, **self.kwargs)
        else:
            shapes = torch.tensor([tuple(t.shape[-self.spatial_dims:]) for t in ref], dtype=torch.int64)
            origins = torch.div(shapes - torch.tensor(self.roi_size), 2, rounding_mode="floor")
            params = None
        return crop_augment_batch(images, labels, origins, self.roi_size, params)

    def extra_repr(self):
        return f"spatial_dims={self.spatial_dims}, roi_size={self.roi_size}, " + ", ".join(f"{k}={v}" for k, v in self.kwargs.items())
