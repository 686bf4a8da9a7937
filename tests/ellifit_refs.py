"""NumPy restatement of csrc/ellifit.hip: boundary points of a class-map region, the draw generator, the reference's
ElliFit (helperfunctions.py:209-276) with its operations in the reference's order, an order-free RANSAC (:278-310), the mapping to
the search's coordinate convention, and dataprep.ellipse_targets.  tests/test_host_ellifit.py pins it to the outputs of the
reference itself (tests/golden/ellifit.npz); tests/test_gpu_ellifit.py compares the device against it."""
from fractions import Fraction

import numpy as np

DEFAULT_REGIONS = ((0b110, 1, 0), (0b100, 2, 0b001))


# ---- boundary points -----------------------------------------------------------------------------------------------------------
def _has_bit(mask, bits):
    m = np.asarray(mask).astype(np.int64)
    ok = (m >= 0) & (m < 32)
    return ok & (((int(bits) & 0xffffffff) >> np.where(ok, m, 0)) & 1).astype(bool)


def boundary_points(mask, class_bits, exclude_bits=0):
    """[N,2] int64 (x, y) = (column, row) in raster order: in the region, some 4-neighbour inside the image outside the region, no
    pixel of the 3x3 neighbourhood inside the image with its bit in exclude_bits."""
    region = _has_bit(mask, class_bits)
    excl = _has_bit(mask, exclude_bits)
    H, W = region.shape
    inside = np.pad(region, 1, constant_values=True)          # the frame edge contributes nothing
    edge = np.zeros_like(region)
    for dy, dx in ((-1, 0), (1, 0), (0, -1), (0, 1)):
        edge |= ~inside[1 + dy:1 + dy + H, 1 + dx:1 + dx + W]
    ex = np.pad(excl, 1, constant_values=False)
    near = np.zeros_like(region)
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            near |= ex[1 + dy:1 + dy + H, 1 + dx:1 + dx + W]
    r, c = np.nonzero(region & edge & ~near)                   # np.nonzero is row-major
    return np.stack([c, r], axis=1).astype(np.int64)


# ---- draws -----------------------------------------------------------------------------------------------------------------------
M32 = 0xffffffff
DRAW_ROUNDS = 4


def mix(x):
    x &= M32
    x ^= x >> 16
    x = (x * 0x7feb352d) & M32
    x ^= x >> 15
    x = (x * 0x846ca68b) & M32
    x ^= x >> 16
    return x


def draw_hash(seed, row, it, attempt):
    h = mix((seed + 0x9e3779b9) & M32)
    h = mix(h ^ (row & M32))
    h = mix(h ^ (it & M32))
    return mix(h ^ (attempt & M32))


def generated_draws(seed, row, N, n_min=15, iters=40, partial=False):
    """int32 [iters+1, n_min]: per iteration the attempts t = 0, 1, ... give index (hash * N) >> 32; an index already taken is
    skipped; at most 64 * DRAW_ROUNDS attempts.  None when some iteration runs out of attempts (status bit 0 on the device);
    with ``partial`` the table with -1 for such iterations, as the device writes it."""
    out = np.full((iters + 1, n_min), -1, dtype=np.int32)
    for it in range(iters + 1):
        got = []
        for t in range(64 * DRAW_ROUNDS):
            if len(got) == n_min:
                break
            # (the device tests a round of 64 attempts at once; taking them one by one in order is the same rule)
            idx = (draw_hash(seed, row, it, t) * N) >> 32
            if idx not in got:
                got.append(idx)
        if len(got) < n_min:
            if not partial:
                return None
            continue
        out[it] = got
    return out


# ---- Fit and the residual: the project's own statement, with the operation order that reproduces the reference's bits ---------------
def fit(points):
    """Unweighted ElliFit (helperfunctions.py:229-265): (Phi [5], model [5], valid).  The points are centred on their mean; the
    design matrix has the columns (x^2, 2xy, -2x, -2y, -1) and the target is -y^2; Phi = inverse(D'D) (D't), the inverse formed
    explicitly and both products left to matmul, which is the order that matters for the last bits.  Fewer than 7 points, a
    singular system or a non-finite entry: model = -1 five times and valid = False."""
    pts = np.asarray(points, dtype=np.float64)
    invalid = np.full(5, -1.0)
    if pts.size <= 12:
        return invalid.copy(), invalid.copy(), False
    mean_x, mean_y = np.mean(pts[:, 0]), np.mean(pts[:, 1])
    u, v = pts[:, 0] - mean_x, pts[:, 1] - mean_y
    design = np.empty((len(u), 5))
    design[:, 0] = u * u
    design[:, 1] = (2 * u) * v
    design[:, 2] = -2 * u
    design[:, 3] = -2 * v
    design[:, 4] = -1.0
    target = -(v * v)
    gram, moment = design.T @ design, design.T @ target
    try:
        Phi = np.linalg.inv(gram) @ moment
    except np.linalg.LinAlgError:
        return invalid.copy(), invalid.copy(), False
    model = model_of_phi(Phi, mean_x, mean_y)
    return (Phi, invalid.copy(), False) if model is None else (Phi, model, True)


def model_of_phi(Phi, mean_x, mean_y):
    """(cx, cy, a, b, theta) of the conic x^2 p0 + 2xy p1 - 2x p2 - 2y p3 - p4 = -y^2 in centred coordinates
    (helperfunctions.py:249-257); None for a model with a non-finite entry.  Squares of scalars go through ``** 2`` (pow), sums run
    left to right: both reproduce the reference's roundings."""
    p0, p1, p2, p3, p4 = (Phi[k] for k in range(5))
    with np.errstate(all="ignore"):
        den = p0 - p1 ** 2
        cx = (p2 - p3 * p1) / den
        cy = (p0 * p3 - p2 * p1) / den
        spread = np.sqrt((1 - p0) ** 2 + 4 * p1 ** 2)
        scale = p4 + cy ** 2 + (cx ** 2) * p0 + 2 * p1
        trace = 1 + p0
        semi_b = np.sqrt(2 * scale / (trace + spread))
        semi_a = np.sqrt(2 * scale / (trace - spread))
        tilt = 0.5 * np.arctan2(2 * p1, 1 - p0)
    model = np.array([cx + mean_x, cy + mean_y, semi_a, semi_b, -tilt], dtype=np.float64)
    return model if np.all(np.isfinite(model)) else None


def fit_error(model, points):
    """The residual RANSAC thresholds (helperfunctions.py:267-276): |(X/a)^2 + (Y/b)^2 - 1| with X = dx cos t - dy sin t and
    Y = dx sin t + dy cos t -- every product rounded on its own, 1/a^2 formed first."""
    pts = np.asarray(points, dtype=np.float64)
    cx, cy, a, b, t = (model[k] for k in range(5))
    with np.errstate(all="ignore"):
        cos_t, sin_t = np.cos(t), np.sin(t)
        dx, dy = pts[:, 0] - cx, pts[:, 1] - cy
        along = dx * cos_t - dy * sin_t
        across = dx * sin_t + dy * cos_t
        return np.abs((1 / a ** 2) * along ** 2 + (1 / b ** 2) * across ** 2 - 1)


def verify(model, pts):
    """my_ellipse(model).verify(pts) (helperfunctions.py:25-33, :140-149): mean of p^T M p, M's rotation is rotation_2d(-theta)."""
    pts = np.asarray(pts, dtype=np.float64)
    if len(pts) == 0:
        return np.inf
    c, s = np.cos(model[4]), np.sin(model[4])
    dx, dy = pts[:, 0] - model[0], pts[:, 1] - model[1]
    u, v = dx * c + dy * s, dy * c - dx * s
    return float(np.mean((u * u) / model[2] ** 2 + (v * v) / model[3] ** 2 - 1.0))


def exact_phi(pts):
    """The normal equations of ElliFit.fit solved in rational arithmetic; (Phi as floats, xm, ym as floats) or None if singular."""
    n = len(pts)
    xm = Fraction(int(pts[:, 0].sum()), n)
    ym = Fraction(int(pts[:, 1].sum()), n)
    rows, rhs = [], []
    for px, py in pts:
        x, y = Fraction(int(px)) - xm, Fraction(int(py)) - ym
        rows.append([x * x, 2 * x * y, -2 * x, -2 * y, Fraction(-1)])
        rhs.append(-y * y)
    A = [[sum(r[i] * r[j] for r in rows) for j in range(5)] + [sum(r[i] * v for r, v in zip(rows, rhs))] for i in range(5)]
    for c in range(5):
        p = next((r for r in range(c, 5) if A[r][c] != 0), None)
        if p is None:
            return None
        A[c], A[p] = A[p], A[c]
        for r in range(5):
            if r != c and A[r][c] != 0:
                f = A[r][c] / A[c][c]
                A[r] = [a - f * b for a, b in zip(A[r], A[c])]
    return np.array([float(A[i][5] / A[i][i]) for i in range(5)]), float(xm), float(ym)


# ---- RANSAC, order-free -----------------------------------------------------------------------------------------------------------
def ransac(pts, draws, n_min=15, iters=40, thres=5e-3, n_good=15):
    """Every iteration on its own, the result is the candidate with the smallest (error, iteration); the all-points fit is
    iteration -1; an invalid model has error +inf.  Returns a dict: model, valid, error, best_iter, n_inl, n_cand (candidates
    including -1), inliers (bool [N] of the best), gap_T (smallest |err - T| / T met), gap_best (relative gap between the two
    smallest errors; inf with one finite candidate)."""
    pts = np.asarray(pts, dtype=np.float64)
    N = len(pts)
    D = max(n_good, n_min)
    cands = []                       # (error, iteration, model, valid, inlier mask)

    def candidate(it, sel):
        _, model, valid = fit(pts[sel])
        err = float(np.mean(fit_error(model, pts[sel]))) if valid else np.inf
        if not np.isfinite(err):
            err = np.inf
        cands.append((err, it, model, valid, sel))

    gap_T = np.inf
    if N < 7:
        return dict(model=-np.ones(5), valid=False, error=np.inf, best_iter=-1, n_inl=0, n_cand=0, inliers=np.zeros(N, bool),
                    gap_T=np.inf, gap_best=np.inf)
    candidate(-1, np.ones(N, bool))
    if N > n_min and iters >= 0:
        for it in range(iters + 1):
            S = np.asarray(draws[it], dtype=np.int64)
            assert len(set(S.tolist())) == n_min and S.min() >= 0 and S.max() < N
            in_s = np.zeros(N, bool)
            in_s[S] = True
            _, pot, ok = fit(pts[in_s])
            if not ok:
                continue
            err = fit_error(pot, pts)
            rest = err[~in_s]
            if len(rest):
                gap_T = min(gap_T, float(np.min(np.abs(rest - thres) / thres)))
            sel = in_s | (err < thres)
            if int(sel.sum()) > D:
                candidate(it, sel)
    order = sorted(range(len(cands)), key=lambda k: (cands[k][0], cands[k][1]))
    best = cands[order[0]]
    finite = sorted(c[0] for c in cands if np.isfinite(c[0]))
    gap_best = (finite[1] - finite[0]) / finite[0] if len(finite) > 1 and finite[0] > 0 else np.inf
    valid = bool(best[3]) and np.isfinite(best[0])
    return dict(model=np.array(best[2], dtype=np.float64) if valid else -np.ones(5), valid=valid, error=best[0], best_iter=best[1],
                n_inl=int(best[4].sum()) if valid else 0, n_cand=len(cands), inliers=best[4], gap_T=gap_T, gap_best=gap_best)


# ---- the search's coordinate convention ------------------------------------------------------------------------------------------------
def to_search(model, H, W):
    """The fitted ellipse as the search reads it.  The model is the ellipse my_ellipse draws from it: a along
    (cos t, sin t), x = column, y = row (fit_error turns the other way; on drawn ellipses my_ellipse's reading is the drawn one).
    Second-moment form scaled by sx = W/(W-1), sy = H/(H-1); a' the semi-axis along theta' (calc_ell_iou)."""
    sx, sy = W / (W - 1), H / (H - 1)
    c, s = np.cos(model[4]), np.sin(model[4])
    a2, b2 = model[2] * model[2], model[3] * model[3]
    mxx = (a2 * (c * c) + b2 * (s * s)) * (sx * sx)
    myy = (a2 * (s * s) + b2 * (c * c)) * (sy * sy)
    mxy = ((a2 - b2) * (c * s)) * (sx * sy)
    d = mxx - myy
    rr = np.sqrt(d * d + 4.0 * mxy * mxy)
    return np.array([model[0] * sx, model[1] * sy, np.sqrt((mxx + myy + rr) / 2.0), np.sqrt(max((mxx + myy - rr) / 2.0, 0.0)),
                     0.5 * np.arctan2(2.0 * mxy, d)])


# ---- a whole call ----------------------------------------------------------------------------------------------------------------------
def ransac_from_mask(mask, regions=DEFAULT_REGIONS, n_min=15, iters=40, thres=5e-3, n_good=15, draws=None, seed=0, max_pts=4096):
    """What utils.ellipse_ransac_from_mask(..., return_stats=True) returns, as NumPy arrays, row R*f + r = region r of frame f
    (generated draws: one stream per region r, whatever the frame):
    dict(init, frame_of, cls, raw, stats_i, stats_f, status, points (list of [N,2]), draws [n, iters+1, n_min])."""
    mask = np.asarray(mask)
    F, H, W = mask.shape
    R = len(regions)
    n = F * R
    K1 = max(iters + 1, 0)
    out = dict(init=-np.ones((n, 5)), raw=-np.ones((n, 5)), frame_of=-np.ones(n, np.int32), cls=np.zeros(n, np.int32),
               stats_i=np.zeros((n, 4), np.int32), stats_f=np.full((n, 2), np.inf), status=0, points=[],
               draws=-np.ones((n, K1, n_min), np.int32))
    for i in range(n):
        f, reg = divmod(i, R)
        reg = tuple(regions[reg]) + (0,) * (3 - len(regions[reg]))
        out["cls"][i] = reg[1]
        pts = boundary_points(mask[f], reg[0], reg[2]) if reg[0] else np.zeros((0, 2), np.int64)
        out["stats_i"][i] = (len(pts), -1, 0, 0)
        if len(pts) > max_pts:
            out["status"] |= 2
            out["points"].append(pts[:max_pts])
            continue
        out["points"].append(pts)
        N = len(pts)
        if N < 7:
            continue
        d = None
        if N > n_min and iters >= 0:
            d = generated_draws(seed, i % R, N, n_min, iters) if draws is None else np.asarray(draws[i])
            bad = d is None or any(len(set(r.tolist())) != n_min or r.min() < 0 or r.max() >= N for r in d)
            if bad:
                out["status"] |= 1
                continue
            out["draws"][i] = d
        res = ransac(pts, d, n_min, iters, thres, n_good)
        out["stats_i"][i, 3] = res["n_cand"]
        if not res["valid"]:
            continue
        out["raw"][i] = res["model"]
        out["init"][i] = to_search(res["model"], H, W)
        out["frame_of"][i] = f
        out["stats_i"][i, 1:3] = (res["best_iter"], res["n_inl"])
        out["stats_f"][i] = (res["error"], verify(res["model"], pts))
    return out


# ---- dataprep.ellipse_targets ----------------------------------------------------------------------------------------------------------
def _rot(t):
    c, s = np.cos(t), np.sin(t)
    return np.array([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1]])


def _trans(cx, cy):
    return np.array([[1.0, 0.0, cx], [0.0, 1.0, cy], [0.0, 0.0, 1]])


def ellipse_info(param, H, W):
    """get_ellipse_info(param, H, cond=False)[1] (helperfunctions.py:488-518) with my_ellipse.transform (:124-129), mat2param
    (:50-63), recover_theta (:102-116) and recover_C (:118-122)."""
    cx, cy, a, b, theta = param
    Hn = np.array([[2 / W, 0, -1], [0, 2 / H, -1], [0, 0, 1]])
    Hr, Ht = _rot(-theta), _trans(-cx, -cy)
    Q = np.array([[1 / a ** 2, 0, 0], [0, 1 / b ** 2, 0], [0, 0, -1]])
    mat = Ht.T @ Hr.T @ Q @ Hr @ Ht
    Hi = np.linalg.inv(Hn)
    m = np.linalg.inv(Hn.T) @ mat @ Hi
    qa, qb, qc, qd, qe = m[0, 0], 2 * m[0, 1], m[1, 1], 2 * m[0, 2], 2 * m[1, 2]
    if abs(qb) <= 1e-40 and qa <= qc:
        th = 0.0
    elif abs(qb) <= 1e-40 and qa > qc:
        th = np.pi / 2
    else:
        th = 0.5 * np.arctan2(qb, (qa - qc))
    tx = (2 * qc * qd - qb * qe) / (qb ** 2 - 4 * qa * qc)
    ty = (2 * qa * qe - qb * qd) / (qb ** 2 - 4 * qa * qc)
    R2, T2 = _rot(th), _trans(tx, ty)
    mn = R2.T @ T2.T @ m @ T2 @ R2
    p = np.array([tx, ty, np.sqrt(1 / mn[0, 0]), np.sqrt(1 / mn[1, 1]), th])
    if p[2] > p[3]:
        p[[2, 3]] = p[[3, 2]]
        p[4] = 0.5 * np.pi + p[4]
    return p


def ellipse_targets(label, **ransac_args):
    """(pupil_center [B,2], iris_center [B,2], elNorm [B,2,5], cond [B,4]) float32, the batch contract of CurriculumLib.py:152-165,
    :189-193 from the labels alone: default regions (row 0 iris, row 1 pupil); a fit is accepted when |verify| < 0.05."""
    label = np.asarray(label)
    B, H, W = label.shape
    res = ransac_from_mask(label, DEFAULT_REGIONS, **ransac_args)
    pc, ic = -np.ones((B, 2)), -np.ones((B, 2))
    el = -np.ones((B, 2, 5))
    cond = np.zeros((B, 4))
    for b in range(B):
        ok = [res["frame_of"][2 * b + r] >= 0 and abs(res["stats_f"][2 * b + r, 1]) < 0.05 for r in (0, 1)]
        r, c = np.nonzero(label[b] == 2)
        if ok[1]:
            pc[b] = res["raw"][2 * b + 1, :2]
        elif len(r):
            pc[b] = (np.mean(c), np.mean(r))
        else:
            cond[b, 0] = 1
        cond[b, 1] = float(np.all(label[b] == 0))
        cond[b, 2] = float(not ok[1])
        cond[b, 3] = float(not ok[0])
        ic[b] = res["raw"][2 * b, :2] if ok[0] else pc[b]
        for r_ in (0, 1):
            if ok[r_]:
                el[b, r_] = ellipse_info(res["raw"][2 * b + r_], H, W)
    return pc.astype(np.float32), ic.astype(np.float32), el.astype(np.float32), cond.astype(np.float32)
