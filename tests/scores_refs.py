"""Seeded inputs and the NumPy / torch restatement of what csrc/scores.hip computes (egne_amd.scores); shared by
tests/golden/make_golden_scores.py (which runs the REFERENCE's utils.getSeg_metrics / getAng_metric / getPoint_metric on the same
inputs and records their outputs in tests/golden/scores.npz), tests/test_host_scores.py and tests/test_gpu_scores.py.

The restatement follows the host path operation for operation:
  counts      np.count_nonzero of (t == c), (p == c) and both per frame and class
  iou         n_both / (n_true + n_pred - n_both) as one float64 division for the classes present in the truth, NaN elsewhere and for
              samples whose cond[:, 1] is set                                    -- pinned by the reference's score_list, exactly
  distances   float32: (0.5 * W) * (x + 1), differences, squares, one add, sqrt  -- the reference goes through sklearn's
              expanded-square pairwise distances and agrees to rtol 1e-6 only
  angles      float32 |a - b|, widened, np.rad2deg                               -- pinned by the reference, exactly
  scales      float32 sqrt((a_gt^2 + b_gt^2) / (a_pred^2 + b_pred^2)), every operation rounded once (IEEE): lines of the reference's
              train.py (:323-329) in torch float32, not a function; the reference does NOT pin them, this restatement is the
              definition.  It is written in NumPy, not torch: torch's CPU square root is not correctly rounded (on an AVX-512 host
              733 of 100,000 float32 roots in [0.5, 1.5) came out one ulp beside np.sqrt's, and the same expression gave 1.1966949
              on one host and 1.1966948 on another), so "the bits torch gives" name no single value.  scale_torch is the script's
              expression as written; tests hold it within 2 ulps of this one (quotient within 1 ulp, which moves the root by half
              of that, plus the root's own ulp).
"""
import numpy as np
import torch

FIELDS = 16
IOU, DIST, ANG, SCALE, COND0, COND1, LOSS, BATCH, SAMPLE = 0, 3, 7, 9, 11, 12, 13, 14, 15

# ---- segmentation cases: (name, B); H x W = 9 x 11 (odd frame size) ------------------------------------------------------
SEG_HW = (9, 11)
SEG_CASES = ("all_present", "no_pupil", "one_class", "pred_has_extra_class", "cond_some", "cond_all", "cond_none")


def seg_case(name):
    """(y_true, y_pred int64 [B,H,W], cond1 float32 [B]) of a named case."""
    H, W = SEG_HW
    rng = np.random.RandomState(1000 + SEG_CASES.index(name))
    B = 4
    yt = rng.randint(0, 3, (B, H, W)).astype(np.int64)
    yp = np.where(rng.rand(B, H, W) < 0.7, yt, rng.randint(0, 3, (B, H, W))).astype(np.int64)
    cond = np.zeros(B, np.float32)
    if name == "no_pupil":                 # frame 1 has no class 2 in the truth (the prediction keeps some)
        yt[1][yt[1] == 2] = 1
    elif name == "one_class":              # frame 0 is background only, frame 2 iris only; prediction of frame 2 misses it entirely in a corner
        yt[0][:] = 0
        yt[2][:] = 1
        yp[2][:2] = 0
    elif name == "pred_has_extra_class":   # the truth of frames 0 and 3 lacks class 2 / class 0, the prediction has them
        yt[0][yt[0] == 2] = 0
        yp[0][:3, :3] = 2
        yt[3][yt[3] == 0] = 1
        yp[3][4:, 5:] = 0
    elif name == "cond_some":
        cond[[1, 2]] = 1
    elif name == "cond_all":
        cond[:] = 1
    return yt, yp, cond


def counts_ref(yt, yp, ncls=3):
    """uint32 [B,ncls,3]: (n_true, n_pred, n_both); values outside [0, ncls) count for no class."""
    B = yt.shape[0]
    out = np.zeros((B, ncls, 3), np.uint32)
    for i in range(B):
        for c in range(ncls):
            t, p = yt[i] == c, yp[i] == c
            out[i, c] = (np.count_nonzero(t), np.count_nonzero(p), np.count_nonzero(t & p))
    return out


def iou_ref(counts, cond1):
    """float64 [B,3] from the counts: the reference's score_list."""
    B, ncls = counts.shape[:2]
    out = np.full((B, 3), np.nan)
    for i in range(B):
        if cond1[i]:
            continue
        for c in range(ncls):
            nt, npred, nb = (int(v) for v in counts[i, c])
            if nt:
                out[i, c] = np.float64(nb) / np.float64(nt + npred - nb)
    return out


# ---- ellipse vectors ----------------------------------------------------------------------------------------------------
VEC_B, VEC_SEED, VEC_HW = 12, 77, (240, 320)      # the case the fixture records


def vec_inputs(B, seed, hw=(240, 320)):
    """float32 elOut, elPred [B,10], pupil_center, iris_center [B,2] (pixels), elNorm [B,2,5], cond bool [B,4].  Sample 0 (if B > 1:
    also sample 1) carries zero axes, so that the scale ratios meet x / 0 and 0 / 0."""
    H, W = hw
    g = torch.Generator().manual_seed(seed)
    elOut = (torch.rand(B, 10, generator=g) * 2 - 1).float()
    elPred = (torch.rand(B, 10, generator=g) * 2 - 1).float()
    pc = (torch.rand(B, 2, generator=g) * torch.tensor([W, H])).float()
    ic = (torch.rand(B, 2, generator=g) * torch.tensor([W, H])).float()
    elNorm = (torch.rand(B, 2, 5, generator=g) * 2 - 1).float()
    cond = torch.rand(B, 4, generator=g) < 0.3
    elOut[0, 2:4] = 0.0                     # iris: x / 0 -> inf
    if B > 1:
        elOut[1, 7:9] = 0.0                 # pupil: 0 / 0 -> NaN
        elNorm[1, 1, 2:4] = 0.0
    return elOut, elPred, pc, ic, elNorm, cond


def unnorm_ref(p, hw):
    """utils.unnormPts on a float32 array."""
    H, W = hw
    o = np.array(p, dtype=np.float32, copy=True)
    o[:, 0] = 0.5 * W * (o[:, 0] + 1)
    o[:, 1] = 0.5 * H * (o[:, 1] + 1)
    return o


def dist_ref(gt, pred, hw):
    """Raw centre distances: float32 arithmetic, widened."""
    d = np.asarray(gt, np.float32) - unnorm_ref(pred, hw)
    return np.sqrt((d ** 2).sum(axis=1)).astype(np.float64)


def ang_ref(gt, pred):
    """Raw angular distances in degrees: float32 |a - b|, widened, rad2deg."""
    return np.rad2deg(np.abs(np.asarray(gt, np.float32) - np.asarray(pred, np.float32)).astype(np.float64))


def scale_ref(gt_ab, pred_ab):
    """IEEE float32, widened (the reference does not pin this, and torch's own square root is not the IEEE one: module docstring)."""
    g, p = np.asarray(gt_ab, np.float32), np.asarray(pred_ab, np.float32)
    with np.errstate(all="ignore"):
        return np.sqrt((g[:, 0] * g[:, 0] + g[:, 1] * g[:, 1]) / (p[:, 0] * p[:, 0] + p[:, 1] * p[:, 1])).astype(np.float64)


def scale_torch(gt_ab, pred_ab):
    """train.py:323-329 as written, in torch float32 on this host's CPU."""
    gt_ab, pred_ab = torch.as_tensor(gt_ab, dtype=torch.float32), torch.as_tensor(pred_ab, dtype=torch.float32)
    return torch.sqrt(torch.sum(gt_ab ** 2, dim=1) / torch.sum(pred_ab ** 2, dim=1)).double().numpy()


def ulps32(a, b):
    """Largest distance in float32 ulps between two arrays of widened float32 values (NaN and inf must sit in the same places)."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    fin = np.isfinite(a)
    assert np.array_equal(fin, np.isfinite(b)) and np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(a[np.isinf(a)], b[np.isinf(b)])
    ia, ib = a[fin].astype(np.float32).view(np.int32).astype(np.int64), b[fin].astype(np.float32).view(np.int32).astype(np.int64)
    return int(np.abs(ia - ib).max()) if ia.size else 0


def rows_ref(yt, yp, elOut, elPred, pc, ic, elNorm, cond, loss=None, batch_no=0, ncls=3, hw=None):
    """The ledger rows of one batch, float64 [B, FIELDS] (``hw``: the image size the centres are un-normalised with, by default the maps')."""
    eo, ep, en = (np.asarray(t, np.float32) for t in (elOut, elPred, elNorm))
    pc, ic = np.asarray(pc, np.float32), np.asarray(ic, np.float32)
    c = np.asarray(cond).astype(bool)
    B = yt.shape[0]
    hw = tuple(yt.shape[1:]) if hw is None else hw
    r = np.full((B, FIELDS), np.nan)
    r[:, IOU:IOU + 3] = iou_ref(counts_ref(np.asarray(yt), np.asarray(yp), ncls), c[:, 1])
    r[:, DIST + 0] = dist_ref(pc, eo[:, 5:7], hw)
    r[:, DIST + 1] = dist_ref(pc, ep[:, 5:7], hw)
    r[:, DIST + 2] = dist_ref(ic, eo[:, 0:2], hw)
    r[:, DIST + 3] = dist_ref(ic, ep[:, 0:2], hw)
    r[:, ANG + 0] = ang_ref(en[:, 0, 4], eo[:, 4])
    r[:, ANG + 1] = ang_ref(en[:, 1, 4], eo[:, 9])
    with np.errstate(all="ignore"):
        r[:, SCALE + 0] = scale_ref(en[:, 0, 2:4], eo[:, 2:4])
        r[:, SCALE + 1] = scale_ref(en[:, 1, 2:4], eo[:, 7:9])
    r[:, COND0], r[:, COND1] = c[:, 0], c[:, 1]
    r[:, LOSS] = np.nan if loss is None else np.float64(np.float32(loss))
    r[:, BATCH] = batch_no
    r[:, SAMPLE] = np.arange(B)
    return r


# ---- maps for the counting kernel -----------------------------------------------------------------------------------------
def maps(B, H, W, seed, ncls=3, stray=True):
    """int64 [B,H,W] truth and prediction; with ``stray`` a few values outside [0, ncls) (negative, ncls, 2^32 + 1: a low word that
    looks like class 1) in both."""
    rng = np.random.RandomState(seed)
    yt = rng.randint(0, ncls, (B, H, W)).astype(np.int64)
    yp = np.where(rng.rand(B, H, W) < 0.6, yt, rng.randint(0, ncls, (B, H, W))).astype(np.int64)
    if stray:
        n = B * H * W
        for a, s in ((yt, 1), (yp, 2)):
            idx = rng.choice(n, size=max(1, n // 50), replace=False)
            a.reshape(-1)[idx] = rng.choice(np.array([-1, ncls, 2 ** 32 + 1, -2 ** 40, 255], np.int64), size=idx.size)
            if n > 2:
                a.reshape(-1)[(s * 7) % n] = 2 ** 32 + 1
    return yt, yp
