"""NumPy restatement of the ellipse scores of test.py's bbox_iou_flag block (csrc/ellipse_scores.hip, egne_amd.scores.EllipseLedger)
and the seeded inputs shared by tests/test_host_ellipse_scores.py, tests/test_gpu_ellipse_scores.py and the fixture generator
tests/golden/make_golden_ellipse_scores.py.

    box_corners / quad_fill / box_iou      calc_bbox with NumPy's int32 conversion; the closed-quadrilateral fill; n_and / n_or
    ell_map / ell_counts                   the membership rule of calc_ell_iou: oracle.fit.ell_inside, not a second form of it
    summary                                the per-batch and final reductions of test.py:151-155, :240-247
    inputs(H, W, N, seed)                  class maps, elPred, elNorm, cond with the guards the fixture asks for

The fill rule (include/egne_hip.h): a pixel belongs to a box iff every edge cross product, in exact integers, has the sign of the
box's signed area or is zero; a box without area holds the pixels exactly on its four segments.  cv2.fillPoly agrees with it away
from the edges; which edge pixels OpenCV sets is NOT restated (tests/test_host_ellipse_scores.py holds the rule against PIL within
one pixel of the drawn edges).
"""
import math

import numpy as np

from oracle import fit as ofit

import fit_cases as fc

NEAR_INT = 1e-6        # a float64 corner coordinate this close to an integer is rejected: device and host cos / sin differ in the last place
NEAR_ZERO = 1e-9       # a pixel whose wtMat is this close to zero likewise


def roa(x, y, a):
    """calc_box_iou.py:8-12."""
    return math.cos(a) * x - math.sin(a) * y, math.sin(a) * x + math.cos(a) * y


def box_corners_f64(el):
    """calc_box_iou.py:13-27: [4,2] float64, corners (-a,-b), (-a,+b), (+a,+b), (+a,-b) around the centre turned by -theta, turned back."""
    x, y, a, b, t = (float(v) for v in el[:5])
    xx, yy = roa(x, y, -t)
    return np.array([roa(px, py, t) for px, py in ((xx - a, yy - b), (xx - a, yy + b), (xx + a, yy + b), (xx + a, yy - b))], np.float64)


def to_i32(v):
    """np.array(v, dtype=np.int32) spelled out: truncation toward zero; NaN and values outside int32 give INT_MIN."""
    v = np.asarray(v, np.float64)
    ok = (v > -2147483649.0) & (v < 2147483648.0)
    return np.where(ok, np.trunc(np.where(ok, v, 0.0)), -2147483648.0).astype(np.int64).astype(np.int32)


def box_corners(el):
    """int32 [8] = (x0, y0, ..., x3, y3): what calc_ell_bbox_iou hands to fillPoly."""
    return to_i32(box_corners_f64(el)).reshape(8)


def near_integer(el):
    c = box_corners_f64(el)
    return bool(np.any(np.abs(c - np.round(c)) < NEAR_INT)) or not np.all(np.isfinite(c))


def quad_fill(corners, H, W):
    """bool [H,W]: the closed quadrilateral of int corners [8], pixel by pixel, in exact integers (Python ints beyond 2^29)."""
    c = [int(v) for v in np.asarray(corners).reshape(8)]
    xs, ys = c[0::2], c[1::2]
    a2 = ((xs[1] - xs[0]) * (ys[2] - ys[0]) - (ys[1] - ys[0]) * (xs[2] - xs[0]) +
          (xs[2] - xs[0]) * (ys[3] - ys[0]) - (ys[2] - ys[0]) * (xs[3] - xs[0]))
    sgn = (a2 > 0) - (a2 < 0)
    dt = np.int64 if max(abs(v) for v in c) < 1 << 29 else object
    py, px = np.mgrid[0:H, 0:W]
    px, py = px.astype(dt), py.astype(dt)
    inside, on_seg = np.ones((H, W), bool), np.zeros((H, W), bool)
    for k in range(4):
        n = (k + 1) % 4
        cr = (xs[n] - xs[k]) * (py - ys[k]) - (ys[n] - ys[k]) * (px - xs[k])
        inside &= np.asarray(cr >= 0 if sgn > 0 else cr <= 0, bool)
        on_seg |= (np.asarray(cr == 0, bool) & np.asarray((px >= min(xs[k], xs[n])) & (px <= max(xs[k], xs[n])), bool) &
                   np.asarray((py >= min(ys[k], ys[n])) & (py <= max(ys[k], ys[n])), bool))
    return inside if sgn != 0 else on_seg


def box_iou(ca, cb, H, W):
    """(IoU, n_and, n_or) of two boxes on the H x W canvas: calc_box_iou.py:28-38 with the fill above (NaN for 0 / 0, as NumPy)."""
    a, b = quad_fill(ca, H, W), quad_fill(cb, H, W)
    n_and, n_or = int(np.count_nonzero(a & b)), int(np.count_nonzero(a | b))
    return (n_and / n_or if n_or else float("nan")), n_and, n_or


def deg(el):
    """A pixel ellipse with the angle in the reference's degrees: what one evaluation of the search is handed."""
    el = np.array(el, np.float64)
    el[4] = el[4] * 180. / ofit.PI_REF
    return el


def ell_map(H, W, el_px):
    """bool [H,W]: calc_ell_iou's map of the pixel ellipse (cx, cy, a, b, theta in radians) -- oracle.fit.ell_inside."""
    with np.errstate(all="ignore"):
        return ofit.ell_inside((H, W), deg(el_px), ofit.mesh_f32(H, W))


def ell_counts(seg, el_px):
    """(pixels of seg, pixels of the ellipse, pixels of both): oracle.fit.ell_counts."""
    with np.errstate(all="ignore"):
        return ofit.ell_counts(seg, deg(el_px), ofit.mesh_f32(*seg.shape))


def membership_margin(H, W, el_px):
    """min |wtMat| over the pixels, by the operations of oracle.fit.ell_inside (the guard of the fixture only; the test holds
    (wt <= 0) equal to ell_inside)."""
    el = deg(el_px)
    el[4] = el[4] / 180. * ofit.PI_REF
    with np.errstate(all="ignore"):
        el = ofit.transform(el, np.array([[2 / W, 0, -1], [0, 2 / H, -1], [0, 0, 1]]))
        mx, my = ofit.mesh_f32(H, W)
        f = np.float32
        cx, cy, a, b, ct, st = f(el[0]), f(el[1]), f(el[2]), f(el[3]), f(np.cos(el[4])), f(np.sin(el[4]))
        dx, dy = mx - cx, my - cy
        u, v = (dx * ct + dy * st) / a, ((-dx) * st + dy * ct) / b
        wt = u * u + v * v - f(1)
    return wt


def to_pixels(el_norm, H, W):
    """my_ellipse(p).transform(H)[0][:5] with H = [[W/2,0,W/2],[0,H/2,H/2],[0,0,1]] on the WIDENED float32 parameters (what
    egne_ellipse_init_from_pred computes): oracle.fit.transform."""
    Hm = np.array([[W / 2, 0, W / 2], [0, H / 2, H / 2], [0, 0, 1]])
    with np.errstate(all="ignore"):
        return ofit.transform(np.asarray(el_norm, np.float32).astype(np.float64), Hm)


def region_scores(pred_px, gt_px, seg):
    """Everything the kernel writes for one (sample, region) from the two pixel ellipses and the class's bool map."""
    H, W = seg.shape
    cp, cg = box_corners(pred_px), box_corners(gt_px)
    iou, n_and, n_or = box_iou(cp, cg, H, W)
    gmap = ell_map(H, W, gt_px)
    n_gt, n_pred, n_both = ell_counts(gmap, pred_px)
    return dict(corners_pred=cp, corners_gt=cg, box_iou=iou, box_and=n_and, box_or=n_or,
                para=np.abs(np.asarray(pred_px, np.float64)[:5] - np.asarray(gt_px, np.float64)[:5]),
                area=(n_pred, n_gt, n_both), map_pred=ell_counts(seg, pred_px), map_gt=ell_counts(seg, gt_px))


def summary(box_iou_by_sample, para_by_sample, batch_sizes):
    """test.py:117-155, :240-247 over recorded per-sample values of ONE region: box_iou_by_sample [N], para_by_sample [N,5], batches
    of batch_sizes samples in order.  Returns (per-batch bbiou list, np.nanmean of it, np.nanmean(para, 0) with [4] in degrees)."""
    import warnings
    bb, at = [], 0
    for B in batch_sizes:
        s = 0
        for i in range(B):
            s += float(box_iou_by_sample[at + i])
        s /= B
        bb.append(s)
        at += B
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", category=RuntimeWarning)
        para = np.nanmean([np.asarray(p, np.float64) for p in para_by_sample], 0)
        para[4] *= 180.0 / 3.1415
        return bb, np.nanmean(bb), para


# ---- seeded inputs ----------------------------------------------------------------------------------------------------------------
# the fixture's cases: name -> (H, W, samples, batch size, seed); "a" holds a sample whose boxes all lie outside the canvas (NaN)
FIXTURE_CASES = {"a": (240, 320, 8, 4, 1), "b": (37, 53, 3, 3, 2)}
OFF_CANVAS = {"a": 5}          # that sample of the case


def _norm(el_px, H, W):
    with np.errstate(all="ignore"):
        return ofit.transform(np.asarray(el_px, np.float64), np.array([[2 / W, 0, -1], [0, 2 / H, -1], [0, 0, 1]])).astype(np.float32)


def _draw(rng, H, W, k):
    """A ground-truth pixel ellipse of region k (0 iris, 1 pupil), a prediction near it and what the class map shows."""
    s = min(H, W)
    ax = (0.28, 0.42) if k == 0 else (0.1, 0.2)
    gt = np.array([W * rng.uniform(0.35, 0.65), H * rng.uniform(0.35, 0.65), s * rng.uniform(*ax), s * rng.uniform(*ax), rng.uniform(-1.4, 1.4)])
    def near(e, c, r, t):
        return np.array([e[0] + s * rng.uniform(-c, c), e[1] + s * rng.uniform(-c, c), e[2] * rng.uniform(1 - r, 1 + r),
                         e[3] * rng.uniform(1 - r, 1 + r), e[4] + rng.uniform(-t, t)])
    return gt, near(gt, 0.03, 0.15, 0.3), near(gt, 0.02, 0.1, 0.2)


def inputs(H, W, N, seed, off_canvas=()):
    """dict(mask int64 [N,H,W], elPred float32 [N,10], elNorm float32 [N,2,5], cond float32 [N,2]).  Every ellipse is drawn again until
    no float64 box corner of its pixel form lies within NEAR_INT of an integer and no pixel's wtMat within NEAR_ZERO of zero.  Samples
    in ``off_canvas`` have both ellipses of both regions far outside the frame: box IoU 0 / 0."""
    rng = np.random.RandomState(1000 * seed + H * 7 + W)
    mask = np.zeros((N, H, W), np.int64)
    elPred, elNorm = np.zeros((N, 10), np.float32), np.zeros((N, 2, 5), np.float32)

    def ok(p):
        px = to_pixels(p, H, W)
        return (np.all(np.isfinite(px)) and not near_integer(px) and
                not np.any(np.abs(membership_margin(H, W, px)) < NEAR_ZERO))
    for i in range(N):
        for k in (0, 1):
            while True:
                gt, pred, shown = _draw(rng, H, W, k)
                if i in off_canvas:
                    gt[:2] += (6 * W, 5 * H)
                    pred[:2] += (6 * W, 5 * H)
                g, p = _norm(gt, H, W), _norm(pred, H, W)
                if ok(g) and ok(p):
                    break
            elNorm[i, k], elPred[i, 5 * k:5 * k + 5] = g, p
            mask[i][fc.render(H, W, shown)] = 1 + k
        sp = rng.rand(H, W) < 0.01
        mask[i][sp] = rng.randint(0, 3, size=int(sp.sum()))
    cond = np.zeros((N, 2), np.float32)
    cond[:, 0] = rng.rand(N) < 0.2
    cond[:, 1] = rng.rand(N) < 0.3
    return dict(mask=mask, elPred=elPred, elNorm=elNorm, cond=cond)


def fixture_inputs(name):
    H, W, N, B, seed = FIXTURE_CASES[name]
    return inputs(H, W, N, seed, off_canvas=(OFF_CANVAS[name],) if name in OFF_CANVAS else ())
