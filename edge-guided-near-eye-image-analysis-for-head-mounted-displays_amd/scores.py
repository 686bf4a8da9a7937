"""Score tracking on the device: the per-batch scores of the reference's training and test loops (utils.py:120-170 getSeg_metrics /
getPoint_metric / getAng_metric, the loop body train.py:289-338) from the tensors that already are in HBM, without copying a class
map or a label map to the host (csrc/scores.hip).

    seg_confusion_counts(y_true, y_pred)   uint32 [B,ncls,3] on the device: (n_true, n_pred, n_both) per frame and class
    ScoreLedger                            one float64 row per sample, appended by two launches per batch; one copy down per epoch
    seg_metrics / point_metric / ang_metric / epoch_summary     the host reductions over rows

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


def gather_rows(rows):
    """Rows of all ranks, rank after rank, with the batch numbers made distinct (every rank counts its batches from 0)."""
    from . import parallel
    if parallel.world_size() == 1:
        return rows
    parts, off = [], 0
    for r in parallel.gather_lists([rows]):
        r = np.array(r, dtype=np.float64).reshape(-1, FIELDS)
        if len(r):
            r[:, BATCH] += off
            off = r[:, BATCH].max() + 1
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
