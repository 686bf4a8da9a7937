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

    pack_annotations / labels_from_annotations -> Masks_noSkin, Masks   int8 [B,R,C]: the label maps the reference's
                                                          dataset_generation/Extract_TEyeD_*_histo.py scripts draw from a TEyeD annotation
                                                          (eyeball circle, iris and pupil ellipses, 34 eyelid landmarks).  The arguments
                                                          handed to cv2.circle / ellipse / fillPoly are pinned by the reference
                                                          (tests/golden/annot.npz); PIXEL PARITY WITH OpenCV IS UNPINNED: the pixels are
                                                          this project's rules (include/egne_hip.h, csrc/annot_core.h)
    annotation_fits / annotation_keep                     pupil_loc, Fits/pupil, Fits/iris and the acceptance rule of the same scripts (host)
"""
import math

import numpy as np
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


# ---- label maps from TEyeD annotations (csrc/annot.hip) ---------------------------------------------------------------------------------
ANNOT_RECORD_WORDS, ANNOT_MAX_VERTS, ANNOT_MAX_COORD = 150, 64, 1 << 20
ANNOT_HAS_BALL, ANNOT_HAS_IRIS, ANNOT_HAS_PUPIL, ANNOT_HAS_LID = 1, 2, 4, 8
ANNOT_IRIS_ZERO_AXIS, ANNOT_PUPIL_ZERO_AXIS, ANNOT_EMPTY = 1, 2, 4


def _trunc_int(v, what):
    """int() of the scripts for an array: truncation toward zero; what the record cannot hold is refused."""
    v = np.asarray(v, np.float64)
    if not np.all(np.abs(v) <= ANNOT_MAX_COORD):          # (NaN fails the comparison too)
        raise ValueError("pack_annotations: %s beyond 2**20 (or not finite): the kernel's int64 products would not hold it" % what)
    return np.trunc(v).astype(np.int32)


def pack_annotations(ball, iris, pupil, lid, present=None):
    """TEyeD annotation rows -> the records egne_labels_from_annotations reads (int32 [B,150], include/egne_hip.h), on the host.
    float64 rows as the annotation files hold them behind their frame number: ``ball`` [B,3] = (r, cx, cy); ``iris`` / ``pupil``
    [B,5] = (angle in degrees, cx, cy, full width, full height); ``lid`` [B,n,2] (x, y), n <= 64.  Any of them may be None (absent
    for all frames); ``present`` bool [B,4] (ball, iris, pupil, lid) switches shapes off per frame.

    Exactly what the scripts apply before they draw (Extract_TEyeD_NvGaze_AR_histo.py:150-179, pinned by tests/golden/annot.npz):
    int() truncation of centres, radius and lid points, int(w / 2) and int(h / 2), the angle unmodified; c, s = cos, sin of
    radians(angle) in float64.  A value beyond 2**20 in magnitude is refused, so that no int64 product of the rules can overflow."""
    given = [a is not None for a in (ball, iris, pupil, lid)]
    B = next((len(a) for a in (ball, iris, pupil, lid) if a is not None), None)
    if B is None:
        raise ValueError("pack_annotations: no annotation at all")
    pres = np.ones((B, 4), bool) if present is None else np.asarray(present, bool).reshape(B, 4).copy()
    pres &= np.array(given)[None, :]
    rec = np.zeros((B, ANNOT_RECORD_WORDS), np.int32)
    dbl = rec.view(np.float64)                        # word 2k is float64 k
    rec[:, 0] = pres @ np.array([ANNOT_HAS_BALL, ANNOT_HAS_IRIS, ANNOT_HAS_PUPIL, ANNOT_HAS_LID])
    if ball is not None:
        b = np.where(pres[:, 0:1], np.asarray(ball, np.float64).reshape(B, 3), 0.0)
        rec[:, 2:5] = _trunc_int(b[:, [1, 2, 0]], "an eyeball centre or radius")
    for k, (e, word) in enumerate(((iris, 6), (pupil, 14)), 1):
        if e is None:
            continue
        e = np.where(pres[:, k:k + 1], np.asarray(e, np.float64).reshape(B, 5), 0.0)
        rec[:, word:word + 2] = _trunc_int(e[:, 1:3], "an ellipse centre")
        rec[:, word + 2:word + 4] = _trunc_int(e[:, 3:5] / 2, "an ellipse half-axis")
        if not np.all(np.isfinite(e[:, 0])):
            raise ValueError("pack_annotations: an ellipse angle is not finite")
        t = np.radians(e[:, 0])
        dbl[:, word // 2 + 2] = np.where(pres[:, k], np.cos(t), 0.0)          # (an absent shape leaves its words zero)
        dbl[:, word // 2 + 3] = np.where(pres[:, k], np.sin(t), 0.0)
    if lid is not None:
        v = np.asarray(lid, np.float64)
        if v.ndim != 3 or v.shape[0] != B or v.shape[2] != 2 or v.shape[1] > ANNOT_MAX_VERTS:
            raise ValueError("pack_annotations: lid must be [B,n,2] with n <= %d, not %s" % (ANNOT_MAX_VERTS, v.shape))
        n = v.shape[1]
        rec[:, 1] = np.where(pres[:, 3], n, 0)
        rec[:, 22:22 + 2 * n] = _trunc_int(np.where(pres[:, 3, None, None], v, 0.0), "a lid point").reshape(B, 2 * n)
    return rec


def annotation_keep(ball, iris, pupil):
    """The scripts' acceptance rule (Extract_TEyeD_NvGaze_AR_histo.py:141-146) for rows as pack_annotations takes them: bool [B], False
    where the eyeball's r, cx or cy, the iris' cx or cy or the pupil's cx or cy is negative."""
    ball, iris, pupil = (np.asarray(a, np.float64) for a in (ball, iris, pupil))
    return ~((ball[:, :3] < 0).any(1) | (iris[:, 1:3] < 0).any(1) | (pupil[:, 1:3] < 0).any(1))


def annotation_fits(iris, pupil):
    """(pupil_loc [B,2], Fits_pupil [B,5], Fits_iris [B,5]) float64 in the archive's conventions (Extract_TEyeD_NvGaze_AR_histo.py:186-210):
    pupil_loc = the pupil's (cx, cy); a fit is (cx, cy, w / 2, h / 2, theta) with theta = deg2rad(a if a <= 90 else -(180 - a))."""
    def fit(e):
        e = np.asarray(e, np.float64).reshape(-1, 5)
        a = np.where(e[:, 0] > 90, -(180 - e[:, 0]), e[:, 0])
        return np.stack([e[:, 1], e[:, 2], e[:, 3] / 2, e[:, 4] / 2, np.deg2rad(a)], axis=1)
    fp = fit(pupil)
    return fp[:, :2].copy(), fp, fit(iris)


def labels_from_annotations(records, size, src_hw=None, with_skin=True, out=None, return_status=False, device=None):
    """The label maps of a batch of records (pack_annotations) on the device, on the current stream (egne_labels_from_annotations: three
    launches, no synchronisation).  ``records`` int32 [B,150], NumPy or a device tensor; ``size`` the canvas (R, C); ``src_hw`` int32
    [B,2] (NumPy or device) the frames' own (rows, columns): pixels at or beyond them stay 0.  Returns int8 [B,R,C] maps:
    (Masks_noSkin, Masks) with ``with_skin``, else Masks_noSkin alone; with ``return_status`` the int32 [B] status words behind them
    (ANNOT_IRIS_ZERO_AXIS, ANNOT_PUPIL_ZERO_AXIS, ANNOT_EMPTY).  ``out``: the map buffer(s) to fill instead of new ones.

    The pixels are this project's rules (include/egne_hip.h); a present ellipse with a zero half-axis paints nothing and sets its status
    bit, where OpenCV would draw a line segment."""
    R, C = int(size[0]), int(size[1])
    if isinstance(records, np.ndarray):
        dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        if records.dtype != np.int32:
            raise ValueError("labels_from_annotations: records must be int32 [B,%d]" % ANNOT_RECORD_WORDS)
        records = torch.from_numpy(np.ascontiguousarray(records)).to(dev)
    require_cuda(records, "records")
    if records.dtype != torch.int32 or records.dim() != 2 or records.shape[1] != ANNOT_RECORD_WORDS or records.shape[0] < 1:
        raise ValueError("labels_from_annotations: records must be int32 [B,%d]" % ANNOT_RECORD_WORDS)
    records = records.contiguous()
    B, dev = records.shape[0], records.device
    hw = None
    if src_hw is not None:
        hw = src_hw if torch.is_tensor(src_hw) else torch.from_numpy(np.ascontiguousarray(np.asarray(src_hw, np.int32).reshape(B, 2)))
        hw = hw.to(dev).contiguous()
        if hw.dtype != torch.int32 or tuple(hw.shape) != (B, 2):
            raise ValueError("labels_from_annotations: src_hw must be int32 [B,2]")
    outs = [] if out is None else ([out] if torch.is_tensor(out) else list(out))
    if len(outs) not in (0, 2 if with_skin else 1):
        raise ValueError("labels_from_annotations: out must hold %d map(s)" % (2 if with_skin else 1))
    for t in outs:
        require_cuda(t, "out")
        if t.dtype != torch.int8 or tuple(t.shape) != (B, R, C) or not t.is_contiguous():
            raise ValueError("labels_from_annotations: out must be contiguous int8 [%d,%d,%d]" % (B, R, C))
    if not outs:
        outs = [torch.empty((B, R, C), dtype=torch.int8, device=dev) for _ in range(2 if with_skin else 1)]
    status = torch.empty(B, dtype=torch.int32, device=dev)
    _lib.check(_lib.lib().egne_labels_from_annotations(records.data_ptr(), None if hw is None else hw.data_ptr(), B, R, C, outs[0].data_ptr(),
                                                       outs[1].data_ptr() if with_skin else None, status.data_ptr(), _lib.stream_ptr()),
               "labels_from_annotations")
    res = tuple(outs) if with_skin else outs[0]
    return (res, status) if return_status else res
