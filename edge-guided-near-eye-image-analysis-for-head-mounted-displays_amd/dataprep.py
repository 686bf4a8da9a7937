"""Device-side batch preparation: what the reference's Dataset does per sample on the host
(CurriculumLib.py:127-139) for the tensors the hot path consumes, as batched HIP kernels.

    dist_maps(label)  ->  distMap   float32 [B,3,H,W]   helperfunctions.one_hot2dist per class (:356-371), bit-identical
    zscore(img)       ->  img       float32 [B,1,H,W]   (img - img.mean()) / img.std() per image (CurriculumLib.py:139)

    spatial_weights(label) -> spatWts float32 [B,H,W]  1 + 20 * dilate(Canny(label, 0, 1) / 255, (3, 3)) (CurriculumLib.py:128-129);
                                                          PARITY UNPINNED - OpenCV is not available in the build container and the
                                                          reference holds no fixture, so this follows OpenCV's published algorithm
                                                          (restated in oracle/dataprep.py, which the kernel matches bit for bit)

    ellipse_targets(label) -> pupil_center [B,2], iris_center [B,2], elNorm [B,2,5], cond [B,4]   float32: the ellipse part of the batch
                                                          contract (CurriculumLib.py:152-165, :189-193) from the labels alone, through
                                                          the reference's own estimator (utils.ellipse_ransac_from_mask)
"""
import math

import torch

from . import _lib
from .engine import require_cuda


def dist_maps(label, ncls=3):
    require_cuda(label, "label")
    if label.dtype != torch.int64 or label.dim() != 3:
        raise ValueError("label must be an int64 [B,H,W] tensor")
    label = label.contiguous()
    B, H, W = label.shape
    L = _lib.lib()
    out = torch.empty((B, ncls, H, W), dtype=torch.float32, device=label.device)
    ws = torch.empty(int(L.egne_dist_maps_workspace_bytes(B, H, W, ncls)), dtype=torch.uint8, device=label.device)
    _lib.check(L.egne_dist_maps(label.data_ptr(), B, H, W, ncls, out.data_ptr(), ws.data_ptr(), _lib.stream_ptr()), "dist_maps")
    return out


def zscore(img):
    require_cuda(img, "img")
    x = img.to(torch.float32).contiguous()
    B = x.shape[0]
    out = torch.empty_like(x)
    _lib.check(_lib.lib().egne_zscore(x.data_ptr(), out.data_ptr(), B, x.numel() // B, _lib.stream_ptr()), "zscore")
    return out


def spatial_weights(label):
    """CurriculumLib.py:128-129 on the device (parity unpinned, see the module docstring)."""
    require_cuda(label, "label")
    if label.dtype != torch.int64 or label.dim() != 3:
        raise ValueError("label must be an int64 [B,H,W] tensor")
    label = label.contiguous()
    B, H, W = label.shape
    out = torch.empty((B, H, W), dtype=torch.float32, device=label.device)
    _lib.check(_lib.lib().egne_spatial_weights(label.data_ptr(), B, H, W, out.data_ptr(), _lib.stream_ptr()), "spatial_weights")
    return out


def _mat3(rows):
    return torch.stack([torch.stack(r, dim=-1) for r in rows], dim=-2)


def _ellipse_transform(param, Hi):
    """my_ellipse(param).transform(H)[0][:-1] (helperfunctions.py:25-33, :50-63, :102-129) for param [...,5] float64 through the
    conic; ``Hi`` [3,3] is the INVERSE of H."""
    cx, cy, a, b, th = param.unbind(-1)
    one, zero = torch.ones_like(cx), torch.zeros_like(cx)

    def rot(t):
        c, s = torch.cos(t), torch.sin(t)
        return _mat3([[c, -s, zero], [s, c, zero], [zero, zero, one]])

    def trans(x, y):
        return _mat3([[one, zero, x], [zero, one, y], [zero, zero, one]])

    T = lambda m: m.transpose(-1, -2)      # noqa: E731
    Hr, Ht = rot(-th), trans(-cx, -cy)
    Q = _mat3([[1 / a ** 2, zero, zero], [zero, 1 / b ** 2, zero], [zero, zero, -one]])
    mat = T(Ht) @ T(Hr) @ Q @ Hr @ Ht
    m = Hi.T @ mat @ Hi
    qa, qb, qc, qd, qe = m[..., 0, 0], 2 * m[..., 0, 1], m[..., 1, 1], 2 * m[..., 0, 2], 2 * m[..., 1, 2]
    flat = qb.abs() <= 1e-40
    t2 = torch.where(flat, torch.where(qa <= qc, zero, one * (math.pi / 2)), 0.5 * torch.atan2(qb, qa - qc))
    den = qb ** 2 - 4 * qa * qc
    tx, ty = (2 * qc * qd - qb * qe) / den, (2 * qa * qe - qb * qd) / den
    R2, T2 = rot(t2), trans(tx, ty)
    mn = T(R2) @ T(T2) @ m @ T2 @ R2
    major, minor = torch.sqrt(1 / mn[..., 0, 0]), torch.sqrt(1 / mn[..., 1, 1])
    return torch.stack([tx, ty, major, minor, t2], dim=-1)


def _ellipse_info(param, H, W):
    """get_ellipse_info(param, H, cond=False)[1] (helperfunctions.py:488-518) for param [...,5] float64: my_ellipse.transform with
    H = [[2/W, 0, -1], [0, 2/H, -1], [0, 0, 1]], mat2param, and the axis swap that keeps param 3 >= param 2."""
    Hi = torch.tensor([[W / 2, 0, W / 2], [0, H / 2, H / 2], [0, 0, 1]], dtype=param.dtype, device=param.device)      # inverse of H
    tx, ty, major, minor, t2 = _ellipse_transform(param, Hi).unbind(-1)
    swap = major > minor
    return torch.stack([tx, ty, torch.where(swap, minor, major), torch.where(swap, major, minor),
                        torch.where(swap, 0.5 * math.pi + t2, t2)], dim=-1)


def ellipse_targets(label, **ransac_args):
    """(pupil_center [B,2], iris_center [B,2], elNorm [B,2,5], cond [B,4]) float32 on the device from int64 labels [B,H,W]: the
    reference's ElliFit + RANSAC on the iris and pupil boundaries (utils.ellipse_ransac_from_mask with its default regions;
    ``ransac_args``: n_min, iters, thres, n_good, draws, seed, max_pts), then the batch contract of CurriculumLib.py:152-165, :189-193.
    Vectorised over the batch in float64, no per-frame Python loop, no synchronisation.

    A fit is accepted when |verify| < 0.05 (dataset_generation/ExtractRITEyes_general.py:203-209).  A rejected pupil fit falls back to
    the centroid of the class-2 pixels for pupil_center; iris_center is the pupil centre where the iris fit is rejected
    (CurriculumLib.py:153).  elNorm is get_ellipse_info's normalisation (H = [[2/W, 0, -1], [0, 2/H, -1], [0, 0, 1]], axis swap kept;
    the search's W/(W-1) correction is not applied).  cond = (no pupil centre, label all background, pupil ellipse rejected or absent,
    iris ellipse rejected or absent); a rejected ellipse is -1 five times.  The reference DROPS a frame whose pupil or iris fit it
    rejects when it builds a dataset; a batch cannot, so such frames stay in it with their cond flags set."""
    from .utils import DEFAULT_RANSAC_REGIONS, ellipse_ransac_from_mask
    require_cuda(label, "label")
    if label.dtype != torch.int64 or label.dim() != 3:
        raise ValueError("label must be an int64 [B,H,W] tensor")
    B, H, W = label.shape
    _, fo, _, raw, _, sf, _, _, _ = ellipse_ransac_from_mask(label, DEFAULT_RANSAC_REGIONS, return_stats=True, **ransac_args)
    raw = raw.view(B, 2, 5)
    ok = (fo.view(B, 2) >= 0) & (sf[:, 1].view(B, 2).abs() < 0.05)
    pup = label == 2
    cnt = pup.sum(dim=(1, 2))
    sx = (pup.sum(dim=1) * torch.arange(W, device=label.device)).sum(dim=1)
    sy = (pup.sum(dim=2) * torch.arange(H, device=label.device)).sum(dim=1)
    cen = torch.stack([sx.double(), sy.double()], dim=1) / cnt.clamp(min=1).double()[:, None]
    minus = torch.full((B, 2), -1.0, dtype=torch.float64, device=label.device)
    pc = torch.where(ok[:, 1:2], raw[:, 1, :2], torch.where((cnt > 0)[:, None], cen, minus))
    ic = torch.where(ok[:, 0:1], raw[:, 0, :2], pc)
    el = torch.where(ok[..., None], _ellipse_info(torch.where(ok[..., None], raw, torch.ones_like(raw)), H, W), -torch.ones_like(raw))
    cond = torch.stack([~ok[:, 1] & (cnt == 0), (label == 0).flatten(1).all(dim=1), ~ok[:, 1], ~ok[:, 0]], dim=1)
    return pc.float(), ic.float(), el.float(), cond.float()
