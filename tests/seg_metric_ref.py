"""Independent reference of the segmentation metrics, written for the tests: CPU only, int64 / float64, no kernels and
nothing imported from factorizer_amd.metrics.  Counts are plain boolean reductions, edges come from shifting the zero-padded
mask along each axis, directed distances from brute force over all (query, target) edge pairs in chunks, the quantile from
torch.quantile in float64."""
from __future__ import annotations

import math

import torch
import torch.nn.functional as F


def bound64(sigmoid=True, threshold=0.5):
    """float64 decision bound on the stored value"""
    if not sigmoid:
        return float(threshold)
    return math.log(threshold / (1.0 - threshold))


def decide(pred, sigmoid=True, threshold=0.5):
    """bool foreground: masks by non-zero, values by x >= bound in float64"""
    pred = pred.detach().cpu()
    if pred.dtype in (torch.uint8, torch.bool):
        return pred != 0
    return pred.to(torch.float64) >= bound64(sigmoid, threshold)


def counts(pred, label, sigmoid=True, threshold=0.5):
    """int64 (B, C, 3) = |P and Y|, |P|, |Y|"""
    p = decide(pred, sigmoid, threshold)
    y = label.detach().cpu().to(torch.float64) != 0
    B, C = p.shape[:2]
    p, y = p.reshape(B, C, -1), y.reshape(B, C, -1)
    return torch.stack([(p & y).sum(-1), p.sum(-1), y.sum(-1)], dim=-1).to(torch.int64)


def dice(cnt, include_background=True, ignore_empty=False):
    """float64 (B, C) Dice values of a counts tensor, the four cases of the table written out one by one"""
    B, C = cnt.shape[:2]
    out = torch.empty((B, C), dtype=torch.float64)
    for b in range(B):
        for c in range(C):
            i, p, y = (int(v) for v in cnt[b, c])
            if y > 0:
                out[b, c] = 2.0 * i / (p + y)
            elif ignore_empty:
                out[b, c] = math.nan
            else:
                out[b, c] = 1.0 if p == 0 else 0.0
    return out if include_background else out[:, 1:]


def edges(mask):
    """bool edges of (B, C, *S): foreground voxels with a background face neighbour, the image padded by one zero voxel"""
    m = mask.detach().cpu() != 0
    nd = m.dim() - 2
    padded = F.pad(m.to(torch.uint8), (1, 1) * nd).bool()
    centre = tuple(slice(1, 1 + s) for s in m.shape[2:])
    all_nb = torch.ones_like(m)
    for ax in range(nd):
        for sh in (-1, 1):
            sl = list(centre)
            sl[ax] = slice(1 + sh, 1 + sh + m.shape[2 + ax])
            all_nb &= padded[(slice(None), slice(None)) + tuple(sl)]
    return m & ~all_nb


def min_dist2(q, t, spacing=None, chunk=1 << 22):
    """float64 (nq,) minimum squared spacing-scaled distance from each row of q (nq, nd) to the rows of t (nt, nd)"""
    nd = q.shape[1]
    s = torch.ones(nd, dtype=torch.float64) if spacing is None else torch.tensor([float(v) for v in spacing], dtype=torch.float64)
    qs, ts = q.to(torch.float64) * s, t.to(torch.float64) * s
    step = max(1, chunk // max(1, ts.shape[0]))
    out = torch.empty(qs.shape[0], dtype=torch.float64)
    for i in range(0, qs.shape[0], step):
        d = qs[i:i + step, None, :] - ts[None, :, :]
        out[i:i + step] = (d * d).sum(-1).min(dim=1).values
    return out


def min_dist2_int(q, t, chunk=1 << 22):
    """the same for unit spacing in exact int64 arithmetic"""
    q, t = q.to(torch.int64), t.to(torch.int64)
    step = max(1, chunk // max(1, t.shape[0]))
    out = torch.empty(q.shape[0], dtype=torch.int64)
    for i in range(0, q.shape[0], step):
        d = q[i:i + step, None, :] - t[None, :, :]
        out[i:i + step] = (d * d).sum(-1).min(dim=1).values
    return out


def _quantiles(d, percentiles):
    return [float(d.max() if p is None else torch.quantile(d, p / 100.0)) for p in percentiles]


def directed(eq, et, percentiles, spacing):
    """one float per percentile: quantile of the nearest-edge distances from the edge plane eq to the edge plane et (bool,
    spatial axes only); None stands for the maximum"""
    q, t = torch.nonzero(eq), torch.nonzero(et)
    if q.shape[0] == 0:
        return [math.nan] * len(percentiles)
    if t.shape[0] == 0:
        return [math.inf] * len(percentiles)
    return _quantiles(min_dist2(q, t, spacing).sqrt(), percentiles)


def hausdorff_table(pred_mask, label_mask, percentiles, spacing=None):
    """{percentile: (directed, undirected)}, each float64 (B, C); the all-pairs distances are formed once per plane and
    direction.  directed: NaN when the prediction has no edge, inf when only the label has none; undirected: the maximum
    of the two directions, NaN if either is NaN."""
    ep, ey = edges(pred_mask), edges(label_mask)
    nd = ep.dim() - 2
    if spacing is not None and isinstance(spacing, (int, float)):
        spacing = (float(spacing),) * nd
    B, C = ep.shape[:2]
    out = {p: (torch.empty((B, C), dtype=torch.float64), torch.empty((B, C), dtype=torch.float64)) for p in percentiles}
    for b in range(B):
        for c in range(C):
            fwd = directed(ep[b, c], ey[b, c], percentiles, spacing)
            bwd = directed(ey[b, c], ep[b, c], percentiles, spacing)
            for p, v, v2 in zip(percentiles, fwd, bwd):
                out[p][0][b, c] = v
                out[p][1][b, c] = math.nan if (math.isnan(v) or math.isnan(v2)) else max(v, v2)
    return out


def hausdorff(pred_mask, label_mask, percentile=95, spacing=None, directed_only=False, include_background=True):
    """float64 (B, C) of one percentile (see hausdorff_table)"""
    out = hausdorff_table(pred_mask, label_mask, [percentile], spacing)[percentile][0 if directed_only else 1]
    return out if include_background else out[:, 1:]


def blobs(shape, seed, level=0.0, smooth=3):
    """bool blobs (B, C, *S): box-smoothed Gaussian noise above `level` standard deviations"""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(shape, generator=g)
    nd = len(shape) - 2
    B, C = shape[:2]
    x = x.reshape(B * C, 1, *shape[2:])
    pool = (F.avg_pool1d, F.avg_pool2d, F.avg_pool3d)[nd - 1]
    k = 2 * smooth + 1
    for _ in range(2):
        x = pool(x, k, stride=1, padding=smooth, count_include_pad=True)
    x = x.reshape(shape)
    dims = tuple(range(2, len(shape)))
    return (x - x.mean(dims, keepdim=True)) / x.std(dims, keepdim=True) > level
