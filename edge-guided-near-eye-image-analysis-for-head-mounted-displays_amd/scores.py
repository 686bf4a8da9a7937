"""Score tracking on the device: the per-batch scores of the reference's training and test loops (utils.py:120-170 getSeg_metrics /
getPoint_metric / getAng_metric, the loop body train.py:289-338) from the tensors that already are in HBM, without copying a class
map or a label map to the host (csrc/scores.hip).

    seg_confusion_counts(y_true, y_pred)   uint32 [B,ncls,3] on the device: (n_true, n_pred, n_both) per frame and class
    ScoreLedger                            one float64 row per sample, appended by two launches per batch; one copy down per epoch
    seg_metrics / point_metric / ang_metric / epoch_summary     the host reductions over rows
    EllipseLedger, ellipse_summary         the ellipses against ground truth (test.py:108-155 behind bbox_iou_flag; csrc/ellipse_scores.hip):
                                           one row of ELL_FIELDS float64 per sample by one launch per batch, and the reference's reductions
    ellipse_box_corners / box_iou_counts   the box corners and the box IoU alone, for ellipses and boxes from elsewhere

A row holds raw per-sample values; every reduction over them is the host expression the scripts use otherwise (utils.getSeg_metrics'
own tail, the flag / sum / divide of getPoint_metric and getAng_metric, torch's float32 sum for the scale ratios), so equal rows give
equal bits.  Bit identity of the rows with the host path holds for float32 ellipse vectors and centres: that is what
_entry.SyntheticEyes, loader.device_batch and the curriculum objects (CurriculumLib.py:152-165 at the default --prec 32) deliver.
float64 centres make the host path subtract in float64; they are refused here, not rounded.
"""
import numpy as np
import torch

from . import _lib
from .engine import require_cuda
from .utils import seg_metrics_of_rows

# row layout: EGNE_SCORE_* of include/egne_hip.h
IOU, DIST_PUPIL_LATENT, DIST_PUPIL_SEG, DIST_IRIS_LATENT, DIST_IRIS_SEG = 0, 3, 4, 5, 6
ANG_IRIS, ANG_PUPIL, SCALE_IRIS, SCALE_PUPIL, COND0, COND1, LOSS, BATCH, SAMPLE, FIELDS = 7, 8, 9, 10, 11, 12, 13, 14, 15, 16
CHUNK = 2048          # EGNE_SCORES_CHUNK: pixels of a frame per workgroup
_DIST = {"pupil_latent": DIST_PUPIL_LATENT, "pupil_seg": DIST_PUPIL_SEG, "iris_latent": DIST_IRIS_LATENT, "iris_seg": DIST_IRIS_SEG}
_ANG = {"iris": ANG_IRIS, "pupil": ANG_PUPIL}
_SCALE = {"iris": SCALE_IRIS, "pupil": SCALE_PUPIL}


def _class_map(t, name):
    require_cuda(t, name)
    if t.dtype != torch.int64 or t.dim() != 3:
        raise TypeError("%s must be an int64 [B,H,W] tensor (got %s %s)" % (name, t.dtype, tuple(t.shape)))
    if not t.is_contiguous():
        raise ValueError("%s must be contiguous" % name)
    return t


def seg_confusion_counts(y_true, y_pred, ncls=3):
    """uint32 [B,ncls,3] on the device: per frame and class the pixels of that class in ``y_true``, in ``y_pred`` and in both (int64
    [B,H,W], contiguous, same device).  Values outside [0, ncls) count for no class.  Queued on the current stream."""
    _class_map(y_true, "y_true")
    _class_map(y_pred, "y_pred")
    if y_true.shape != y_pred.shape or y_true.device != y_pred.device:
        raise ValueError("y_true %s on %s and y_pred %s on %s differ" % (tuple(y_true.shape), y_true.device, tuple(y_pred.shape), y_pred.device))
    if ncls not in (2, 3):
        raise ValueError("ncls must be 2 or 3")
    B, H, W = y_true.shape
    counts = torch.empty((B, ncls, 3), dtype=torch.uint32, device=y_true.device)
    _lib.check(_lib.lib().egne_seg_confusion_counts(y_true.data_ptr(), y_pred.data_ptr(), B, H, W, ncls, counts.data_ptr(), _lib.stream_ptr()),
               "seg_confusion_counts")
    return counts


def _vec(t, name, shape, dev):
    require_cuda(t, name)
    if t.dtype != torch.float32:
        raise TypeError("%s must be float32 (got %s): the host path computes in the dtype it is given, and a silent rounding here "
                        "would break bit identity with it" % (name, t.dtype))
    if tuple(t.shape) != shape or t.device != dev:
        raise ValueError("%s must be %s on %s (got %s on %s)" % (name, shape, dev, tuple(t.shape), t.device))
    return t.detach().contiguous()


class ScoreLedger:
    """``capacity_rows`` rows of FIELDS float64 on ``device``.  ``append`` queues the counts and the row launch of one batch on the
    current stream and returns; the host only counts rows.  ``rows()`` is the one copy down."""

    def __init__(self, capacity_rows, device, ncls=3):
        if ncls not in (2, 3):
            raise ValueError("ncls must be 2 or 3")
        self.capacity, self.ncls, self.device = int(capacity_rows), ncls, torch.device(device)
        self.buf = torch.full((max(self.capacity, 1), FIELDS), float("nan"), dtype=torch.float64, device=self.device)
        self.n = self.batches = 0

    def append(self, labels, mask, elOut, elPred, pupil_center, iris_center, elNorm, cond, loss_terms=None):
        """labels, mask: int64 [B,H,W]; elOut, elPred [B,10], pupil_center, iris_center [B,2], elNorm [B,2,5]: float32 (float64 is
        refused); cond [B,>=2] bool or float; loss_terms: a float32 device tensor whose first element is the batch's loss."""
        B, H, W = labels.shape
        if self.n + B > self.capacity:
            raise RuntimeError("ScoreLedger: %d rows more do not fit (%d of %d used)" % (B, self.n, self.capacity))
        dev = labels.device
        counts = seg_confusion_counts(labels, mask, self.ncls)
        elOut, elPred = _vec(elOut, "elOut", (B, 10), dev), _vec(elPred, "elPred", (B, 10), dev)
        pc, ic = _vec(pupil_center, "pupil_center", (B, 2), dev), _vec(iris_center, "iris_center", (B, 2), dev)
        eln = _vec(elNorm, "elNorm", (B, 2, 5), dev)
        require_cuda(cond, "cond")
        if cond.dim() != 2 or cond.shape[0] != B or cond.shape[1] < 2:
            raise ValueError("cond must be [B, >= 2] (got %s)" % (tuple(cond.shape),))
        cf = cond.to(torch.float32).contiguous()
        lt = None
        if loss_terms is not None:
            lt = _vec(loss_terms.reshape(-1)[:1], "loss_terms", (1,), dev)
        _lib.check(_lib.lib().egne_score_rows(counts.data_ptr(), B, self.ncls, elOut.data_ptr(), elPred.data_ptr(), pc.data_ptr(), ic.data_ptr(),
                                              eln.data_ptr(), cf.data_ptr(), cf.shape[1], lt.data_ptr() if lt is not None else None, H, W,
                                              self.batches, self.buf.data_ptr(), self.n, self.capacity, _lib.stream_ptr()), "score_rows")
        # (counts, cf and the contiguous copies were allocated under the current stream: the caching allocator hands their memory on
        # in that stream's order, behind the two launches)
        self.n += B
        self.batches += 1

    def rows(self):
        """NumPy float64 [n, FIELDS]: the rows appended so far (synchronises: one copy down)."""
        return self.buf[:self.n].cpu().numpy()

    def reset(self):
        self.n = self.batches = 0
        self.buf.fill_(float("nan"))


# ---- ellipse scores against ground truth (csrc/ellipse_scores.hip): the block of test.py:108-155 behind bbox_iou_flag ------------
# row layout: EGNE_ELLSCORE_* of include/egne_hip.h; a region's fields start at region * ELL_REGION_FIELDS (0 iris, 1 pupil)
ELL_PRED, ELL_GT, ELL_CORNERS_PRED, ELL_CORNERS_GT, ELL_BOX_IOU, ELL_BOX_AND, ELL_BOX_OR = 0, 5, 10, 18, 26, 27, 28
ELL_PARA, ELL_AREA, ELL_MAP_PRED, ELL_MAP_GT, ELL_REGION_FIELDS = 29, 34, 37, 40, 43
ELL_COND0, ELL_COND1, ELL_BATCH, ELL_SAMPLE, ELL_FIELDS = 86, 87, 88, 89, 90
ELL_REGIONS = ("iris", "pupil")


def ell_field_names():
    """The ELL_FIELDS column names of an EllipseLedger row, in order."""
    per = (["pred_" + p for p in ("cx", "cy", "a", "b", "theta")] + ["gt_" + p for p in ("cx", "cy", "a", "b", "theta")] +
           ["corner_pred_%s%d" % (c, k) for k in range(4) for c in "xy"] + ["corner_gt_%s%d" % (c, k) for k in range(4) for c in "xy"] +
           ["box_iou", "box_and", "box_or"] + ["abs_" + p for p in ("cx", "cy", "a", "b", "theta")] +
           ["area_pred", "area_gt", "area_both", "map_pred_class", "map_pred_ell", "map_pred_both", "map_gt_class", "map_gt_ell", "map_gt_both"])
    assert len(per) == ELL_REGION_FIELDS
    return [r + "_" + n for r in ELL_REGIONS for n in per] + ["cond0", "cond1", "batch", "sample"]


def ellipse_box_corners(ell_px):
    """int32 [n,8] on the device: the corners (x0, y0, ..., x3, y3) of calc_bbox (calc_box_iou.py:13-27) for pixel ellipses ``ell_px``
    [n,5] float64 (cx, cy, a, b, theta), converted as ``np.array(ans, dtype=np.int32)`` converts them.  Queued on the current stream."""
    require_cuda(ell_px, "ell_px")
    if ell_px.dtype != torch.float64 or ell_px.dim() != 2 or ell_px.shape[1] != 5:
        raise TypeError("ell_px must be a float64 [n,5] tensor (got %s %s)" % (ell_px.dtype, tuple(ell_px.shape)))
    e = ell_px.contiguous()
    out = torch.empty((e.shape[0], 8), dtype=torch.int32, device=e.device)
    if e.shape[0]:
        _lib.check(_lib.lib().egne_ellipse_box_corners(e.data_ptr(), e.shape[0], out.data_ptr(), _lib.stream_ptr()), "ellipse_box_corners")
    return out


def box_iou_counts(corners_a, corners_b, H, W):
    """float64 [n,3] on the device: (IoU, n_and, n_or) of the closed quadrilaterals ``corners_a`` and ``corners_b`` (int32 [n,8]) on an
    H x W canvas; the fill rule is stated in include/egne_hip.h.  IoU is NaN where neither box touches the canvas."""
    for t, name in ((corners_a, "corners_a"), (corners_b, "corners_b")):
        require_cuda(t, name)
        if t.dtype != torch.int32 or t.dim() != 2 or t.shape[1] != 8:
            raise TypeError("%s must be an int32 [n,8] tensor (got %s %s)" % (name, t.dtype, tuple(t.shape)))
    if corners_a.shape != corners_b.shape or corners_a.device != corners_b.device:
        raise ValueError("corners_a %s and corners_b %s differ" % (tuple(corners_a.shape), tuple(corners_b.shape)))
    a, b = corners_a.contiguous(), corners_b.contiguous()
    out = torch.empty((a.shape[0], 3), dtype=torch.float64, device=a.device)
    if a.shape[0]:
        _lib.check(_lib.lib().egne_box_iou_counts(a.data_ptr(), b.data_ptr(), a.shape[0], int(H), int(W), out.data_ptr(), _lib.stream_ptr()),
                   "box_iou_counts")
    return out


class EllipseLedger:
    """``capacity_rows`` rows of ELL_FIELDS float64 on ``device``: per sample the scores of its iris and pupil ellipse against the
    ground truth.  ``append`` queues the launches of one batch on the current stream and returns; ``rows()`` is the one copy down.
    ``classes``: the class of the map the iris and the pupil are held against; a negative one leaves the region out (its fields are
    NaN) -- DeepVOG's two-class map is (-1, 1)."""

    def __init__(self, capacity_rows, device, classes=(1, 2)):
        self.capacity, self.device = int(capacity_rows), torch.device(device)
        self.classes = (int(classes[0]), int(classes[1]))
        if max(self.classes) < 0:
            raise ValueError("classes: at least one region to score")
        self.buf = torch.full((max(self.capacity, 1), ELL_FIELDS), float("nan"), dtype=torch.float64, device=self.device)
        self.n = self.batches = 0

    def append(self, mask, elPred, elNorm, cond, search=False, fit=None):
        """mask: int64 [B,H,W] class map; elPred [B,10], elNorm [B,2,5]: float32 (float64 is refused); cond [B,>=2] bool or float.
        What is scored against elNorm: the pixel forms of elPred; with ``search`` utils.fit_ellipses_from_pred(mask, elPred); with
        ``fit`` that device tensor, float64 [B,2,5] pixel ellipses (iris, pupil) from anywhere (elPred may then be None)."""
        from . import utils
        _class_map(mask, "mask")
        B, H, W = mask.shape
        if self.n + B > self.capacity:
            raise RuntimeError("EllipseLedger: %d rows more do not fit (%d of %d used)" % (B, self.n, self.capacity))
        dev = mask.device
        eln = _vec(elNorm, "elNorm", (B, 2, 5), dev)
        if fit is not None:
            require_cuda(fit, "fit")
            if fit.dtype != torch.float64 or tuple(fit.shape) != (B, 2, 5) or fit.device != dev:
                raise TypeError("fit must be a float64 [%d,2,5] tensor on %s (got %s %s)" % (B, dev, fit.dtype, tuple(fit.shape)))
            pred = fit.detach().contiguous()
        else:
            ep = _vec(elPred, "elPred", (B, 10), dev)
            if search:
                pred = utils.fit_ellipses_from_pred(mask, ep, classes=self.classes)
            else:
                pred = utils.ellipse_seeds_from_pred(ep, H, W)[0]
        require_cuda(cond, "cond")
        if cond.dim() != 2 or cond.shape[0] != B or cond.shape[1] < 2:
            raise ValueError("cond must be [B, >= 2] (got %s)" % (tuple(cond.shape),))
        cf = cond.to(torch.float32).contiguous()
        xs, ys = utils._mesh_axes(H, W, dev)
        _lib.check(_lib.lib().egne_ellipse_pair_scores(eln.data_ptr(), pred.data_ptr(), mask.data_ptr(), cf.data_ptr(), cf.shape[1], B, H, W,
                                                       self.classes[0], self.classes[1], xs.data_ptr(), ys.data_ptr(), self.batches,
                                                       self.buf.data_ptr(), self.n, self.capacity, _lib.stream_ptr()), "ellipse_pair_scores")
        # (pred, cf and the contiguous copies were allocated under the current stream: see ScoreLedger.append)
        self.n += B
        self.batches += 1

    def rows(self):
        """NumPy float64 [n, ELL_FIELDS]: the rows appended so far (synchronises: one copy down)."""
        return self.buf[:self.n].cpu().numpy()

    def reset(self):
        self.n = self.batches = 0
        self.buf.fill_(float("nan"))


def _iou_of_counts(a, b, both):
    with np.errstate(all="ignore"):
        return both / (a + b - both)


def _nanmean(v, axis=None):
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", category=RuntimeWarning)
        return np.nanmean(v, axis=axis)


def ellipse_summary(rows):
    """The reductions of the reference's ellipse block over EllipseLedger rows (test.py:151-155, :240-247), per region name:

      bbiou_<r>          np.nanmean over the batches of (sum of the batch's box IoUs, sample after sample) / batch size: one NaN sample
                         makes its batch NaN, as in the reference
      bbiou_batches_<r>  those per-batch values
      para_<r>           np.nanmean(|parameter differences|, 0) over the samples, [4] times 180.0 / 3.1415

    and plain per-sample means, each also as ``<key>_valid`` without the samples that cond[:, 1] flags:

      box_iou_<r>        the box IoU
      ell_iou_<r>        IoU of the scored against the ground-truth ellipse (n_both / (n_pred + n_gt - n_both))
      map_iou_pred_<r>, map_iou_gt_<r>    IoU of the scored / the ground-truth ellipse against the class map"""
    rows = np.asarray(rows, np.float64).reshape(-1, ELL_FIELDS)
    out = {}
    cut = np.flatnonzero(np.diff(rows[:, ELL_BATCH]) != 0) + 1 if len(rows) else []
    valid = rows[:, ELL_COND1] == 0
    for r, name in enumerate(ELL_REGIONS):
        reg = rows[:, r * ELL_REGION_FIELDS:(r + 1) * ELL_REGION_FIELDS]
        per_batch = []
        for b in (np.split(reg[:, ELL_BOX_IOU], cut) if len(rows) else []):
            s = 0
            for v in b:                      # the reference's `iris_bbiou += ...`: one float64 addition per sample, in order
                s = s + float(v)
            per_batch.append(s / len(b))
        out["bbiou_batches_" + name] = np.array(per_batch, np.float64)
        out["bbiou_" + name] = float(_nanmean(per_batch)) if per_batch else float("nan")
        para = _nanmean(reg[:, ELL_PARA:ELL_PARA + 5], 0) if len(rows) else np.full(5, np.nan)
        para[4] *= 180.0 / 3.1415
        out["para_" + name] = para
        per_sample = {
            "box_iou_": reg[:, ELL_BOX_IOU],
            "ell_iou_": _iou_of_counts(reg[:, ELL_AREA], reg[:, ELL_AREA + 1], reg[:, ELL_AREA + 2]),
            "map_iou_pred_": _iou_of_counts(reg[:, ELL_MAP_PRED], reg[:, ELL_MAP_PRED + 1], reg[:, ELL_MAP_PRED + 2]),
            "map_iou_gt_": _iou_of_counts(reg[:, ELL_MAP_GT], reg[:, ELL_MAP_GT + 1], reg[:, ELL_MAP_GT + 2]),
        }
        for key, v in per_sample.items():
            out[key + name] = float(_nanmean(v)) if len(v) else float("nan")
            out[key + name + "_valid"] = float(_nanmean(v[valid])) if valid.any() else float("nan")
    return out


def gather_rows(rows, fields=FIELDS, batch_col=BATCH):
    """Rows of all ranks, rank after rank, with the batch numbers made distinct (every rank counts its batches from 0).  ``fields``
    and ``batch_col``: the row width and the column of the batch number (the defaults are ScoreLedger's; EllipseLedger rows pass
    ELL_FIELDS and ELL_BATCH)."""
    from . import parallel
    if parallel.world_size() == 1:
        return rows
    parts, off = [], 0
    for r in parallel.gather_lists([rows]):
        r = np.array(r, dtype=np.float64).reshape(-1, fields)
        if len(r):
            r[:, batch_col] += off
            off = r[:, batch_col].max() + 1
        parts.append(r)
    return np.concatenate(parts, axis=0)


def seg_metrics(rows):
    """(mean IoU, per-class IoU, score_list): the triple of utils.getSeg_metrics for the samples of ``rows``."""
    return seg_metrics_of_rows(rows[:, IOU:IOU + 3], rows[:, COND1].astype(bool))


def _flagged(raw, cond):
    flag = (~cond.astype(bool)).astype(float)
    dist = flag * raw
    return (np.sum(dist) / np.sum(flag) if np.any(flag) else np.nan, dist)


def point_metric(rows, which, flag_col):
    """(mean over valid samples, per-sample distances): the pair of utils.getPoint_metric(..., do_unnorm=True).  ``which``:
    pupil_latent | pupil_seg | iris_latent | iris_seg; ``flag_col``: the column of cond (0 or 1) that invalidates a sample."""
    return _flagged(rows[:, _DIST[which]], rows[:, (COND0, COND1)[flag_col]])


def ang_metric(rows, which):
    """The pair of utils.getAng_metric on elNorm[:, k, 4] against elOut[:, 4 or 9] under cond[:, 1]; ``which``: iris | pupil.
    (rad2deg(flag * d) and flag * rad2deg(d) are the same bits for a flag of 0 or 1.)"""
    return _flagged(rows[:, _ANG[which]], rows[:, COND1])


def scale_sum(rows, which):
    """train.py:323-330: the batch's float32 sum of the scale ratios of the samples without cond[:, 1], as torch forms it."""
    sc = torch.from_numpy(np.ascontiguousarray(rows[:, _SCALE[which]])).to(torch.float32)      # (exact: the rows hold widened float32)
    ok = torch.from_numpy(rows[:, COND1] == 0).to(torch.float32)
    return torch.sum(sc * ok).item()


def batches(rows):
    """The rows of one batch after the other, in the order of appending."""
    if not len(rows):
        return []
    cut = np.flatnonzero(np.diff(rows[:, BATCH]) != 0) + 1
    return np.split(rows, cut)


def epoch_summary(rows):
    """The scalars the reference sends to TensorBoard at the end of an epoch (train.py:387-388, :402-427) under its tags: nanmean and
    nanstd over the batches of the per-batch centre distance, angular distance and scale-ratio sum, and ``train_iou``, the nanmean over
    the batches of the per-class IoU (a list of three)."""
    import warnings
    per = dict(iri_c=[], iri_ang=[], iri_sc=[], pup_c=[], pup_ang=[], pup_sc=[])
    ious = []
    for b in batches(rows):
        ious.append(seg_metrics(b)[1])
        per["iri_c"].append(point_metric(b, "iris_latent", 1)[0])
        per["pup_c"].append(point_metric(b, "pupil_latent", 0)[0])
        per["iri_ang"].append(ang_metric(b, "iris")[0])
        per["pup_ang"].append(ang_metric(b, "pupil")[0])
        per["iri_sc"].append(scale_sum(b, "iris"))
        per["pup_sc"].append(scale_sum(b, "pupil"))
    out = {}
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", category=RuntimeWarning)
        for k, v in per.items():
            out[k + "/mu"] = float(np.nanmean(v)) if v else float("nan")
            out[k + "/std"] = float(np.nanstd(v)) if v else float("nan")
        out["train_iou"] = [float(x) for x in np.nanmean(np.stack(ious, axis=0), axis=0)] if ious else [float("nan")] * 3
    return out
