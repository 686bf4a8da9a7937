"""NumPy restatement of the prediction overlay grid (csrc/dispgrid.hip, egne_amd.dispgrid.image_grid; include/egne_hip.h states the
rules) and the seeded inputs shared by tests/test_host_dispgrid.py, tests/test_gpu_dispgrid.py and the fixture generator
tests/golden/make_golden_dispgrid.py.

    frame_u8 / equalize / grey            utils.py:270-274 around OpenCV's published equalizeHist rule
    pixel_ellipse / perimeter / outline   the transform of egne_ellipse_init_from_pred, evaluate._draw_ellipse's 720 samples, the clip
    make_grid                             torchvision.utils.make_grid(nrow, padding=2, pad_value=0) by its documented layout
    image_grid                            the whole call: (grid float32 [3,Hg,Wg], uint8 BGR [Hg,Wg,3], status int32 [n])
    inputs(B, H, W, seed, ...)            frames, class maps, ellipses, cond with the guards below

Every ellipse of the seeded inputs is drawn again while a float64 pixel parameter that gets truncated lies within NEAR of an integer,
or a sample coordinate within NEAR of a half-integer: device and host cos / sin differ in the last place there, and the rounding would
turn that into a whole pixel (the precaution of tests/ellipse_scores_refs.py).
"""
import hashlib

import numpy as np

import ellipse_scores_refs as ES

NEAR = 1e-6
ST_CONSTANT, ST_NONFINITE, ST_SKIP_IRIS, ST_SKIP_PUPIL, ST_SKIP_GT_IRIS, ST_SKIP_GT_PUPIL = 1, 2, 4, 8, 16, 32
F32 = np.float32


# ---- the frame -----------------------------------------------------------------------------------------------------------------------
def frame_u8(x):
    """np.uint8(255 * (x - x.min()) / (x - x.min()).max()) of utils.py:270-272 in float32; what NumPy leaves undefined is defined as
    the kernel defines it (NaN and negative quotients 0, quotients from 255 up 255).  Returns (u uint8 [H,W], status bits)."""
    x = np.asarray(x, F32)
    fin = np.isfinite(x)
    status = 0 if fin.all() else ST_NONFINITE
    if not fin.any():
        return np.zeros(x.shape, np.uint8), status
    mn, mx = x[fin].min(), x[fin].max()
    with np.errstate(all="ignore"):
        d = F32(mx - mn)
        t = F32(255) * (x - mn)
        q = t / d
    if d == 0:
        status |= ST_CONSTANT
    q = np.where(q >= 0, np.minimum(q, F32(255)), F32(0))          # (NaN >= 0 is False)
    return np.trunc(q).astype(np.uint8), status


def equalize_lut(hist):
    """OpenCV's published equalizeHist rule: the 256-entry table of a histogram."""
    hist = np.asarray(hist, np.int64)
    total = int(hist.sum())
    occ = np.flatnonzero(hist)
    if occ.size == 0:
        return np.zeros(256, np.uint8)
    i0 = int(occ[0])
    h0 = int(hist[i0])
    if h0 == total:
        return np.full(256, i0, np.uint8)
    scale = F32(255) / F32(total - h0)
    s = (np.cumsum(hist) - h0).astype(np.int32)
    r = np.rint(s.astype(F32) * scale)                              # float32 product, ties to even
    lut = np.clip(r, 0, 255).astype(np.uint8)
    lut[:i0 + 1] = 0
    return lut


def equalize(u):
    return equalize_lut(np.bincount(u.ravel(), minlength=256))[u]


def grey(e):
    """utils.py:273-274: e - e.min() in uint8, then float32(e / e.max()) (uint8 / uint8 is a float64 quotient); constant e: 0."""
    e = e - e.min()
    if e.max() == 0:
        return np.zeros(e.shape, F32)
    return (e / e.max()).astype(F32)


def grey_table(hist):
    """The kernel's 256-entry form of equalize + grey (entries of empty bins are defined, never read)."""
    hist = np.asarray(hist, np.int64)
    lut = equalize_lut(hist)
    occ = hist > 0
    if not occ.any():
        return lut, np.zeros(256, F32)
    emin, emax = lut[occ].min(), lut[occ].max()
    if emax == emin:
        return lut, np.zeros(256, F32)
    return lut, ((lut - emin).astype(np.uint8) / np.uint8(emax - emin)).astype(F32)


def grid_u8(g):
    """rint(255 * min(max(g, 0), 1)) in float32, channels reversed: [3,Hg,Wg] -> uint8 [Hg,Wg,3] BGR."""
    c = np.clip(np.asarray(g, F32), F32(0), F32(1))
    return np.ascontiguousarray(np.moveaxis(np.rint(F32(255) * c).astype(np.uint8)[::-1], 0, 2))


# ---- outlines --------------------------------------------------------------------------------------------------------------------------
def pixel_ellipse(el_norm, H, W):
    return ES.to_pixels(el_norm, H, W)


def drawn(el_px):
    el_px = np.asarray(el_px, np.float64)
    return bool(np.all(np.isfinite(el_px[:5])) and np.trunc(el_px[2]) >= 1 and np.trunc(el_px[3]) >= 1)


def _samples(cx, cy, a, b, ang):
    t = np.linspace(0, 2 * np.pi, 720, endpoint=False)              # evaluate._outline_table
    x = cx + a * np.cos(t) * np.cos(ang) - b * np.sin(t) * np.sin(ang)
    y = cy + a * np.cos(t) * np.sin(ang) + b * np.sin(t) * np.cos(ang)
    return x, y


def perimeter(r, c, r_radius, c_radius, orientation):
    """This project's outline pixels in the call form of skimage.draw.ellipse_perimeter: (rows, columns) of evaluate._draw_ellipse's 720
    samples, rounded to the nearest integer (ties to even), unclipped."""
    x, y = _samples(float(c), float(r), float(c_radius), float(r_radius), float(orientation))
    return np.rint(y).astype(np.int64), np.rint(x).astype(np.int64)


def ints_of(el_px):
    """What the reference hands to ellipse_perimeter: int(cy), int(cx), int(b), int(a)."""
    return int(el_px[1]), int(el_px[0]), int(el_px[3]), int(el_px[2])


def clip_rows_cols(rr, cc, H, W):
    """utils.py:344-347: ndarray.clip(6, size - 6) taken literally."""
    return np.minimum(np.maximum(rr, 6), H - 6), np.minimum(np.maximum(cc, 6), W - 6)


def outline(el_px, H, W, cos_sin_theta=None):
    """(rows, columns) of the outline of a pixel ellipse after the clip, or None if it is not drawn.  The clip is done in float64
    before the conversion (the same integers as clip_rows_cols for every coordinate an int64 holds; NaN: 6, then the upper bound)."""
    if not drawn(el_px):
        return None
    cx, cy, a, b = (float(np.trunc(v)) for v in el_px[:4])
    ca, sa = (np.cos(el_px[4]), np.sin(el_px[4])) if cos_sin_theta is None else cos_sin_theta
    t = np.linspace(0, 2 * np.pi, 720, endpoint=False)
    with np.errstate(all="ignore"):
        x = cx + a * np.cos(t) * ca - b * np.sin(t) * sa
        y = cy + a * np.cos(t) * sa + b * np.sin(t) * ca
        rr = np.fmin(np.fmax(np.rint(y), 6.0), float(H - 6)).astype(np.int64)
        cc = np.fmin(np.fmax(np.rint(x), 6.0), float(W - 6)).astype(np.int64)
    return rr, cc


def near_guard(el_norm, H, W):
    """True while the ellipse must be drawn again (module docstring)."""
    px = pixel_ellipse(el_norm, H, W)
    if not np.all(np.isfinite(px)):
        return True
    if np.any(np.abs(px[:4] - np.round(px[:4])) < NEAR):
        return True
    if not drawn(px):
        return False
    r, c, rb, ca = ints_of(px)
    x, y = _samples(float(c), float(r), float(ca), float(rb), float(px[4]))
    fr = np.concatenate([x, y])
    return bool(np.any(np.abs(np.abs(fr - np.floor(fr)) - 0.5) < NEAR))


# ---- the grid --------------------------------------------------------------------------------------------------------------------------
def grid_shape(n, nrow, H, W):
    if n == 1:
        return H, W
    xm = min(nrow, n)
    ym = -(-n // xm)
    return ym * (H + 2) + 2, xm * (W + 2) + 2


def grid_origin(k, n, nrow, H, W):
    if n == 1:
        return 0, 0
    xm = min(nrow, n)
    return (k // xm) * (H + 2) + 2, (k % xm) * (W + 2) + 2


def make_grid(frames, nrow=4):
    """frames [n,3,H,W] -> [3,Hg,Wg]: torchvision.utils.make_grid(frames, nrow=nrow, padding=2, pad_value=0) by its documented layout."""
    frames = np.asarray(frames)
    n, _, H, W = frames.shape
    Hg, Wg = grid_shape(n, nrow, H, W)
    g = np.zeros((3, Hg, Wg), frames.dtype)
    for k in range(n):
        r0, c0 = grid_origin(k, n, nrow, H, W)
        g[:, r0:r0 + H, c0:c0 + W] = frames[k]
    return g


def image_grid(img, mask, el, cond=None, el_gt=None, override=False, count=4, nrow=4, draw_gt=False):
    """The whole call on NumPy arrays: (grid float32 [3,Hg,Wg], uint8 BGR [Hg,Wg,3], status int32 [n])."""
    img, mask = np.asarray(img, F32), np.asarray(mask)
    B, H, W = img.shape
    n = min(count, B)
    frames, status = [], np.zeros(n, np.int32)
    for i in range(n):
        u, st = frame_u8(img[i])
        v = np.zeros((H, W), F32) if st & ST_CONSTANT else grey(equalize(u))
        im = np.stack([v, v, v], 0)
        if override or (cond is not None and cond[i, 1] == 0):
            im[:, mask[i] == 1] = np.array([0, 255, 0], F32)[:, None]
            im[:, mask[i] == 2] = np.array([255, 255, 0], F32)[:, None]
            todo = []
            if draw_gt:
                todo += [(el_gt[i, 0], (0, 102, 255), ST_SKIP_GT_IRIS), (el_gt[i, 1], (0, 102, 255), ST_SKIP_GT_PUPIL)]
            todo += [(el[i, 0], (0, 0, 255), ST_SKIP_IRIS), (el[i, 1], (255, 0, 0), ST_SKIP_PUPIL)]
            for e, colour, bit in todo:
                with np.errstate(all="ignore"):
                    px = pixel_ellipse(e, H, W)
                if not drawn(px):
                    st |= bit
                    continue
                rr, cc = clip_rows_cols(*perimeter(*ints_of(px), px[4]), H, W)
                im[:, rr, cc] = np.array(colour, F32)[:, None]
        status[i] = st
        frames.append(im)
    g = make_grid(np.stack(frames), nrow)
    return g, grid_u8(g), status


def sha(a):
    a = np.ascontiguousarray(a)
    return hashlib.sha256(a.tobytes()).hexdigest()


# ---- seeded inputs ---------------------------------------------------------------------------------------------------------------------
def _frame(rng, H, W):
    """A float32 frame like a z-scored eye image: smooth shading, a dark disc, noise in 4 x 4 blocks (the fixture compresses); negative
    minimum."""
    yy, xx = np.mgrid[0:H, 0:W]
    base = 0.8 * np.sin(xx / W * 3.0 + rng.uniform(0, 3)) + 0.6 * np.cos(yy / H * 2.0 + rng.uniform(0, 3))
    cy, cx, r = H * rng.uniform(0.3, 0.7), W * rng.uniform(0.3, 0.7), min(H, W) * rng.uniform(0.15, 0.3)
    base = base - 1.5 * (((yy - cy) ** 2 + (xx - cx) ** 2) < r * r)
    noise = np.kron(rng.randn(-(-H // 4), -(-W // 4)), np.ones((4, 4)))[:H, :W]
    return (base + 0.3 * noise).astype(F32)


def inputs(B, H, W, seed, leave_frame=()):
    """dict(img float32 [B,H,W], mask int64 [B,H,W], el, el_gt float32 [B,2,5], cond float32 [B,4]).  Samples in ``leave_frame`` have a
    pupil ellipse (predicted and ground truth) whose outline leaves the frame, so that the clip bites."""
    import fit_cases as fc
    rng = np.random.RandomState(7000 * seed + 13 * H + W)
    img = np.stack([_frame(rng, H, W) for _ in range(B)])
    mask = np.zeros((B, H, W), np.int64)
    el, el_gt = np.zeros((B, 2, 5), F32), np.zeros((B, 2, 5), F32)
    for i in range(B):
        for k in (0, 1):
            while True:
                gt, pred, shown = ES._draw(rng, H, W, k)
                if k == 1 and i in leave_frame:
                    shift = np.array([W * 0.45, H * 0.4])
                    gt[:2] += shift
                    pred[:2] += shift
                    shown[:2] += shift
                g, p = ES._norm(gt, H, W), ES._norm(pred, H, W)
                if not near_guard(g, H, W) and not near_guard(p, H, W):
                    break
            el_gt[i, k], el[i, k] = g, p
            mask[i][fc.render(H, W, shown)] = 1 + k
        sp = rng.rand(H, W) < 0.01
        mask[i][sp] = rng.randint(0, 3, size=int(sp.sum()))
    cond = np.zeros((B, 4), F32)
    cond[:, 0] = rng.rand(B) < 0.3
    cond[:, 1] = np.arange(B) % 2                 # mixed: every other frame carries no mask
    return dict(img=img, mask=mask, el=el, el_gt=el_gt, cond=cond)


# the fixture's cases: name -> (B, H, W, seed, override, frames whose pupil outline leaves the frame)
FIXTURE_CASES = {
    "five": (5, 48, 64, 1, True, ()),             # five frames, four drawn
    "odd": (2, 33, 47, 2, True, ()),
    "one": (1, 48, 64, 3, True, ()),              # no padding
    "big": (4, 240, 320, 4, True, ()),            # stored as the uint8 form and a hash of the float grid
    "cond": (4, 48, 64, 5, False, ()),            # override off, mixed cond[:,1]
    "clip": (2, 48, 64, 6, True, (0, 1)),         # the clip rule bites
}
HASHED = ("big",)


def fixture_inputs(name):
    B, H, W, seed, override, leave = FIXTURE_CASES[name]
    return inputs(B, H, W, seed, leave), override


# further seeded cases of the GPU test: name -> (B, H, W, seed, count, nrow)
SEEDED_CASES = {
    "tiny": (1, 13, 17, 11, 4, 4),
    "three_odd": (3, 33, 47, 12, 4, 4),
    "two_rows": (5, 48, 64, 13, 5, 4),
    "big_strided": (4, 240, 320, 14, 4, 4),
}
