"""NumPy restatement of the OpenCV branches of the reference's data_augment.augment (1 blur, 5 glint lines, 6 rotation): the
specification the device kernels of csrc/augment_cv.hip are held to, byte for byte.  TEST INFRASTRUCTURE ONLY.

What is pinned by the reference itself (tests/golden/augment_cv2.npz, recorded by tests/golden/make_golden_augment_cv2.py from the
reference's own augment() with recording stand-ins for the cv2 functions): the np.random draws, every argument handed to OpenCV, the
returned centre and ellipse parameters.  What is restated here from OpenCV's documentation: the pixels.  What stays UNPINNED against
OpenCV (it is not installed where this was written):
  * GaussianBlur: OpenCV filters 8-bit images with 8-bit fixed-point taps in two passes with this rounding, but whether its builds
    round the taps independently or diffuse the error so that they sum to 256 is unchecked (egne_amd.data_augment.gaussian_q8 is the
    one place that decides);
  * line: OpenCV fills a thick line as a fixed-point polygon with round caps; boundary pixels can differ from the exact capsule;
  * warpAffine: OpenCV holds the Lanczos weights as 15-bit integers and the coordinates in 10-bit fixed point; float64 here.  The
    expected difference of a grey level or two is unmeasured.

All arithmetic is integer or IEEE float64 in a fixed order (explicit loops over the taps, vectorised over pixels).  The host pieces
the product needs as well (tap tables, inverse matrix, segment clipping, draws, geometry) are imported from egne_amd.data_augment, so
product and restatement evaluate the same expressions."""
import hashlib

import numpy as np

from egne_amd import data_augment as DA
from oracle import data_augment as oaug


def rng_state_hash():
    """SHA-256 of the global np.random generator's state (key vector, position, cached normal)."""
    st = np.random.get_state()
    return hashlib.sha256(st[1].tobytes() + repr(tuple(st[2:])).encode()).hexdigest()


def reflect101(i, n):
    """BORDER_REFLECT_101 (gfedcb|abcdefgh|gfedcba), one reflection."""
    i = np.where(i < 0, -i, i)
    return np.where(i >= n, 2 * n - 2 - i, i)


def gaussian_blur(img, sigma):
    """cv2.GaussianBlur(img, (7, 7), sigma) on uint8 [H,W]: row pass r = sum q*src, column pass s = sum q*r, (s + 32768) >> 16."""
    img = np.asarray(img)
    H, W = img.shape
    if H < 4 or W < 4:
        raise ValueError("gaussian_blur: H, W >= 4 (one reflection)")
    q = DA.gaussian_q8(sigma).astype(np.int64)
    src = img.astype(np.int64)
    xs, ys = np.arange(W), np.arange(H)
    r = np.zeros((H, W), np.int64)
    for k in range(7):
        r = r + q[k] * src[:, reflect101(xs + k - 3, W)]
    s = np.zeros((H, W), np.int64)
    for k in range(7):
        s = s + q[k] * r[reflect101(ys + k - 3, H), :]
    return ((s + 32768) >> 16).astype(np.uint8)


def capsule_mask(shape, segs):
    """Pixels whose squared distance to one of the segments (x1, y1, x2, y2), float64, is <= 4.0; one operation per statement."""
    H, W = shape
    y, x = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    hit = np.zeros((H, W), bool)
    for ax, ay, bx, by in np.asarray(segs, np.float64).reshape(-1, 4):
        dx = bx - ax
        dy = by - ay
        dxx = dx * dx
        dyy = dy * dy
        len2 = dxx + dyy
        px = x - ax
        py = y - ay
        pdx = px * dx
        pdy = py * dy
        dot = pdx + pdy
        t = dot / len2 if len2 != 0.0 else np.zeros((H, W))
        t = np.where(t < 0.0, 0.0, np.where(t > 1.0, 1.0, t))
        cx = t * dx
        cy = t * dy
        ex = px - cx
        ey = py - cy
        exx = ex * ex
        eyy = ey * ey
        d2 = exx + eyy
        hit |= d2 <= DA.LINE_RADIUS2
    return hit


def draw_lines(img, lines, clip=True):
    """cv2.line(img, (x1, y1), (x2, y2), 255, 4) for every (x1, y1, x2, y2): capsules of radius 2.  ``clip``: through the host's
    Liang-Barsky clipping first, as the product does (False: the segments as given)."""
    img = np.asarray(img)
    if clip:
        n, segs = DA.clip_segments(lines, img.shape)
        segs = segs[:n]
    else:
        segs = np.asarray(lines, np.float64).reshape(-1, 4)
    out = img.copy()
    out[capsule_mask(img.shape, segs)] = 255
    return out


def _source_positions(shape, inv):
    H, W = shape
    y, x = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    i00, i01, i02, i10, i11, i12 = (float(v) for v in inv)
    X = ((i00 * x) + (i01 * y)) + i02
    Y = ((i10 * x) + (i11 * y)) + i12
    return X, Y


def warp_affine_lanczos4(img, M):
    """cv2.warpAffine(img, M, (W, H), flags=cv2.INTER_LANCZOS4), BORDER_CONSTANT 0, uint8 [H,W]."""
    img = np.asarray(img)
    H, W = img.shape
    X, Y = _source_positions((H, W), DA.invert_affine(M))
    ix = np.floor(32.0 * X + 0.5).astype(np.int64)
    iy = np.floor(32.0 * Y + 0.5).astype(np.int64)
    sx0, sy0 = (ix >> 5) - 3, (iy >> 5) - 3
    tab = DA.lanczos4_phase_table()
    wx, wy = tab[ix & 31], tab[iy & 31]                        # [H,W,8]
    src = np.zeros((H + 2, W + 2), np.float64)                 # a frame of zeros around the image: BORDER_CONSTANT
    src[1:-1, 1:-1] = img
    v = np.zeros((H, W), np.float64)
    for ky in range(8):
        sy = np.clip(sy0 + ky, -1, H) + 1
        t = np.zeros((H, W), np.float64)
        for kx in range(8):
            sx = np.clip(sx0 + kx, -1, W) + 1
            t = t + wx[:, :, kx] * src[sy, sx]
        v = v + wy[:, :, ky] * t
    return np.clip(np.rint(v), 0, 255).astype(np.uint8)


def warp_affine_nearest(lab, M):
    """cv2.warpAffine(lab, M, (W, H), flags=cv2.INTER_NEAREST): lab[floor(Y + 0.5), floor(X + 0.5)], 0 outside."""
    lab = np.asarray(lab)
    H, W = lab.shape
    X, Y = _source_positions((H, W), DA.invert_affine(M))
    nx = np.floor(X + 0.5).astype(np.int64)
    ny = np.floor(Y + 0.5).astype(np.int64)
    inside = (nx >= 0) & (nx < W) & (ny >= 0) & (ny < H)
    out = np.zeros_like(lab)
    out[inside] = lab[ny[inside], nx[inside]]
    return out


def rotate(img, lab, ang_deg):
    """Branch 6 for a given angle in degrees: (image, label)."""
    M = DA.rotation_matrix(DA.rotation_centre(np.shape(img)), np.deg2rad(ang_deg))
    return warp_affine_lanczos4(img, M), warp_affine_nearest(lab, M)


def augment(base, mask, pupil_c, elParam, choice=None):
    """The reference's augment() with every branch: 1, 5 and 6 as restated here (draws and geometry by the product's host functions,
    which tests/test_host_augment_cv2.py pins against the reference), the rest by oracle.data_augment.  Consumes np.random as the
    reference does."""
    k = choice
    if k is None:
        state = np.random.get_state()
        k = int(np.random.randint(0, 8))
        if k not in DA.CV2_CHOICES:
            np.random.set_state(state)
            return oaug.augment(base, mask, pupil_c, elParam, None)
    elif k not in DA.CV2_CHOICES:
        return oaug.augment(base, mask, pupil_c, elParam, k)
    cv = {}
    DA.draw(1, base.shape, [k], on_cv2="device", cv2_params=cv)
    pc = np.array(pupil_c, dtype=np.float64)
    pup, iri = np.array(elParam[0], dtype=np.float64), np.array(elParam[1], dtype=np.float64)
    img, lab = np.asarray(base), np.asarray(mask).astype(np.int64)
    if k == 1:
        img = gaussian_blur(base, cv["sigma"][0])
    elif k == 5:
        img = draw_lines(base, cv["lines"][0])
    else:
        img, lab = rotate(base, lab, cv["ang_deg"][0])
        pc, pup, iri = DA.rotate_geometry(pupil_c, elParam[0], elParam[1], cv["ang_rad"][0], cv["centre"])
    return img.astype(np.uint8), lab, pc, (pup, iri)
