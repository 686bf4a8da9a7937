"""data_augment.py of the reference (augment(), :12-130), batched on the device.

The reference augments ONE sample at a time on the host inside its Dataset (CurriculumLib.py:114-120).  Here a whole batch of
uint8 frames that already sits in HBM is augmented by one launch (csrc/dataprep.hip, egne_augment) plus, on request, a second one
for the OpenCV branches (csrc/augment_cv.hip, egne_augment_cv); the random draws stay on the host and consume ``np.random`` in
exactly the reference's order, so the same seed selects the same augmentation with the same parameters for every frame.

    choice  reference branch                         here
    0       flip left-right (:25-36)                 device, pinned against the reference (tests/golden/augment.npz)
    1       cv2.GaussianBlur (:38-42)                ``on_cv2="device"`` only: separable 7-tap filter, 8-bit fixed-point taps, reflect-101
    2       gamma through cv2.LUT (:44-49)           device; the 256-entry table is the reference's expression evaluated on the host,
                                                     cv2.LUT itself (a table look-up) is unpinned
    3       exposure +/- 25 (:51-56)                 device, pinned
    4       Gaussian noise (:58-65)                  device; pinned with the host-drawn noise field (``host_noise=True``); by default the
                                                     field is drawn on the device (same distribution, different stream)
    5       cv2.line glints (:67-79)                 ``on_cv2="device"`` only: capsules of radius 2 around the reference's segments
    6       cv2.warpAffine rotation (:100-119)       ``on_cv2="device"`` only: 8x8 Lanczos taps at 1/32-pixel phases (image), nearest
                                                     (label), the reference's geometry code for centre and ellipses
    >= 7    no change (:121-124)                     device (copy)

The OpenCV branches (1, 5, 6).  OpenCV is not installed where this was written, so by default (``on_cv2="raise"``) they raise and
with ``on_cv2="skip"`` the frame is left unchanged, as before.  ``on_cv2="device"`` builds them:
  * pinned by the reference itself (tests/golden/augment_cv2.npz, recorded by running the reference's augment() with recording
    stand-ins for the cv2 functions): order and count of the np.random draws, every argument handed to OpenCV (sigma, the lines'
    integer end points, colour, thickness, rotation centre / angle / scale, interpolation flags, dsize) and the returned centre and
    ellipse parameters, including that the (-1, -1) centre of an absent ellipse IS rotated while its angle stays -1;
  * restated from OpenCV's documentation (tests/augment_cv2_refs.py, the device kernels are byte-identical to it): the pixel
    arithmetic of GaussianBlur, line and warpAffine;
  * unpinned against OpenCV: which rule its builds use to round the 8-bit blur taps (``gaussian_q8`` holds the table, to be swapped
    if it differs), the boundary pixels of its fixed-point thick-line fill against the exact capsule, and its 15-bit Lanczos weights
    and 10-bit coordinates against float64 weights here (a grey level or two expected, unmeasured).

``augment`` keeps the reference's per-sample signature for NumPy callers; ``augment_batch`` is the path a device-side loader uses.
"""
import numpy as np
import torch

from . import _lib
from .engine import require_cuda
from .frame_io import device_table

CV2_CHOICES = (1, 5, 6)
GAMMAS = (0.6, 0.8, 1.2, 1.4)


def gamma_table(gamma):
    """data_augment.py:47 followed by the final astype(np.uint8) of :126 (cv2.LUT returns table[pixel])."""
    return (255.0 * (np.linspace(0, 1, 256) ** gamma)).astype(np.uint8)


# ---- host pieces of the OpenCV branches (shared with the restatement in tests/augment_cv2_refs.py) ---------------------------------
MAX_LINES = 9            # np.random.randint(1, 10)
LINE_RADIUS2 = 4.0       # thickness 4: a capsule of radius 2 (squared)
LINE_MARGIN = 4          # segments are clipped to [-4, W+3] x [-4, H+3]: nothing outside it reaches a pixel of the frame
INTER_BITS = 5           # OpenCV's interpolation tables hold 32 phases per pixel
_HOST_TABLES = {}


def gaussian_q8(sigma):
    """The 7 taps of cv2.GaussianBlur(.., (7, 7), sigma) as 8-bit fixed point (int32 [7], sum 256): OpenCV's documented
    getGaussianKernel formula k[i] = exp(-(i-3)^2 / (2 sigma^2)) / sum in float64, q = rint(256 k), and 256 - sum(q) added to the
    centre tap.  UNPINNED: OpenCV filters 8-bit images with 8-bit fixed-point taps too, but whether its builds round the taps
    independently or diffuse the rounding error so that they sum to 256 could not be checked (no OpenCV here).  This function is the
    only place that decides it."""
    sigma = int(sigma)
    if not 2 <= sigma <= 6:
        raise ValueError("gaussian_q8: sigma %d outside the reference's range 2..6" % sigma)
    k = [np.exp(-((i - 3) * (i - 3)) / (2.0 * sigma * sigma)) for i in range(7)]
    tot = 0.0
    for v in k:
        tot = tot + v
    q = [int(np.rint(256.0 * (v / tot))) for v in k]
    q[3] += 256 - sum(q)
    return np.array(q, np.int32)


def gaussian_q8_tables():
    """gaussian_q8 for sigma = 2..6, int32 [5,7]."""
    return np.stack([gaussian_q8(s) for s in range(2, 7)])


def lanczos4_phase_table():
    """The 1-D weights of the 8 Lanczos (a = 4) taps at -3..+4 around a source position for each of the 32 sub-pixel phases (float64
    [32,8], rows normalised): the expression of frame_io.lanczos4_table at frac = phase / 32."""
    if "lanczos" not in _HOST_TABLES:
        frac = np.arange(1 << INTER_BITS) / float(1 << INTER_BITS)
        taps = np.arange(-3, 5)
        x = frac[:, None] - taps[None, :]
        with np.errstate(invalid="ignore", divide="ignore"):
            wts = np.where(np.abs(x) < 1e-12, 1.0, np.sin(np.pi * x) * np.sin(np.pi * x / 4) / (np.pi * np.pi * x * x / 4))
        wts = np.where(np.abs(x) < 4, wts, 0.0)
        wts /= wts.sum(1, keepdims=True)
        _HOST_TABLES["lanczos"] = np.ascontiguousarray(wts)
    return _HOST_TABLES["lanczos"]


def rotation_centre(shape):
    """data_augment.py:103."""
    return (int(0.5 * shape[1]), int(0.5 * shape[0]))


def rotation_matrix(centre, ang_rad):
    """cv2.getRotationMatrix2D(centre, angle, 1.0) as documented, float64 [2,3]; ang_rad = angle * (pi / 180)."""
    a, b = np.cos(ang_rad), np.sin(ang_rad)
    cx, cy = float(centre[0]), float(centre[1])
    return np.array([[a, b, (1.0 - a) * cx - b * cy], [-b, a, b * cx + (1.0 - a) * cy]], np.float64)


def invert_affine(M):
    """Inverse of a 2x3 affine map (what cv2.warpAffine does without WARP_INVERSE_MAP), float64 [6] = i00 i01 i02 i10 i11 i12."""
    M = np.asarray(M, np.float64)
    D = 1.0 / (M[0, 0] * M[1, 1] - M[0, 1] * M[1, 0])
    i00, i01, i10, i11 = M[1, 1] * D, -M[0, 1] * D, -M[1, 0] * D, M[0, 0] * D
    i02 = -i00 * M[0, 2] - i01 * M[1, 2]
    i12 = -i10 * M[0, 2] - i11 * M[1, 2]
    return np.array([i00, i01, i02, i10, i11, i12], np.float64)


def rotate_geometry(pupil_c, pupil, iris, ang_rad, centre):
    """data_augment.py:111-120 with the reference's own NumPy calls: the centres rotate unconditionally (also the (-1, -1) of an
    absent ellipse), an angle only where its ellipse is not all -1.  ``pupil`` / ``iris`` are the [5] parameter vectors of the
    sample BEFORE the call; returns new arrays."""
    pc = np.array(pupil_c, dtype=np.float64)
    pup, iri = np.array(pupil, dtype=np.float64), np.array(iris, dtype=np.float64)
    bad_pup, bad_iri = bool(np.all(pup == -1)), bool(np.all(iri == -1))
    R = np.array([[np.cos(ang_rad), -np.sin(ang_rad)],
                  [np.sin(ang_rad), np.cos(ang_rad)]]).squeeze()
    R = R.T
    ctr = np.array(centre)
    pc = np.matmul(R, pc - ctr) + ctr
    pup[:2] = np.matmul(R, pup[:2] - ctr) + ctr
    pup[-1] = pup[-1] - ang_rad if not bad_pup else pup[-1]
    iri[:2] = np.matmul(R, iri[:2] - ctr) + ctr
    iri[-1] = iri[-1] - ang_rad if not bad_iri else iri[-1]
    return pc, pup, iri


def clip_segment(x1, y1, x2, y2, shape):
    """Liang-Barsky in float64: the part of the segment inside [-4, W+3] x [-4, H+3], or None.  (x1 - xc) * tan(theta) of
    getRandomLine is unbounded (1e16 and more); the clipped segment keeps the device arithmetic well conditioned and covers the same
    pixels of the frame, because the dropped parts are further than the radius from every pixel."""
    H, W = shape
    x1, y1, x2, y2 = float(x1), float(y1), float(x2), float(y2)
    dx, dy = x2 - x1, y2 - y1
    t0, t1 = 0.0, 1.0
    for p, q in ((-dx, x1 - (-LINE_MARGIN)), (dx, (W - 1 + LINE_MARGIN) - x1), (-dy, y1 - (-LINE_MARGIN)), (dy, (H - 1 + LINE_MARGIN) - y1)):
        if p == 0.0:
            if q < 0.0:
                return None
            continue
        r = q / p
        if p < 0.0:
            if r > t1:
                return None
            if r > t0:
                t0 = r
        else:
            if r < t0:
                return None
            if r < t1:
                t1 = r
    return (x1 + t0 * dx, y1 + t0 * dy, x1 + t1 * dx, y1 + t1 * dy)


def clip_segments(lines, shape):
    """(kept count, float64 [MAX_LINES, 4]) of up to MAX_LINES segments (x1, y1, x2, y2); the kept ones come first, in order."""
    segs = np.zeros((MAX_LINES, 4), np.float64)
    n = 0
    if len(lines) > MAX_LINES:
        raise ValueError("clip_segments: more than %d lines" % MAX_LINES)
    for ln in lines:
        c = clip_segment(ln[0], ln[1], ln[2], ln[3], shape)
        if c is not None:
            segs[n] = c
            n += 1
    return n, segs


def _draw_lines(shape):
    """The draws of branch 5 (:69-78, getRandomLine :132-137) in the reference's order; the integer end points it hands to cv2.line.
    (Scalars where the reference holds arrays of one element: the same draws and the same float64 operations, a quarter of the time.)"""
    rand = np.random.rand
    f = 0.3 + 0.4 * rand()
    yc, xc = f * shape[0], f * shape[1]
    lines = []
    for _ in range(np.random.randint(1, 10)):
        tan = np.tan(np.pi * rand())
        x1 = xc - 50 * rand() * (1 if rand() < 0.5 else -1)
        y1 = (x1 - xc) * tan + yc
        x2 = xc - (150 * rand() + 50) * (1 if rand() < 0.5 else -1)
        y2 = (x2 - xc) * tan + yc
        lines.append((int(x1), int(y1), int(x2), int(y2)))
    return lines


def draw(B, shape, choices=None, host_noise=False, on_cv2="raise", cv2_params=None):
    """The random draws of ``B`` consecutive augment() calls, in the reference's order per call: the branch index
    (np.random.randint(0, 8), :23), then the branch's own draws.  Returns (choice int32 [B], param float64 [B], lut uint8 [B,256],
    noise float64 [B,H,W] or None).  ``on_cv2``: "raise", "skip" (a frame that drew a cv2 branch is left unchanged) or "device"
    (the branch is kept and its draws are made).  With "device" the dict ``cv2_params``, if given, receives sigma int32 [B] (1),
    nlines int32 [B] and segs float64 [B,9,4] (5: segments clipped to the frame's neighbourhood, the kept ones first), rot float64
    [B,6] (6: inverse matrix i00 i01 i02 i10 i11 i12) and ang_rad float64 [B], plus what the reference hands to OpenCV before any of
    that: lines (per frame the list of integer end points x1 y1 x2 y2), ang_deg float64 [B] and centre (x, y)."""
    H, W = shape
    choice = np.zeros(B, np.int32)
    param = np.zeros(B, np.float64)
    lut = np.tile(np.arange(256, dtype=np.uint8), (B, 1))
    noise = None
    cv = dict(sigma=np.zeros(B, np.int32), nlines=np.zeros(B, np.int32), segs=np.zeros((B, MAX_LINES, 4), np.float64),
              rot=np.tile(np.array([1.0, 0.0, 0.0, 0.0, 1.0, 0.0]), (B, 1)), ang_rad=np.zeros(B, np.float64),
              ang_deg=np.zeros(B, np.float64), lines=[[] for _ in range(B)], centre=rotation_centre(shape))
    for b in range(B):
        c = int(np.random.randint(0, 8)) if choices is None else int(choices[b])
        if c in CV2_CHOICES and on_cv2 != "device":
            if on_cv2 != "skip":
                raise NotImplementedError("augment: branch %d needs OpenCV (blur / lines / rotate are only built as a restatement: "
                                          "pass on_cv2=\"device\", or \"skip\" to leave such frames unchanged)" % c)
            c = 7
        if c == 1:
            cv["sigma"][b] = np.random.randint(2, 7)
        elif c == 2:
            lut[b] = gamma_table(GAMMAS[np.random.randint(0, 4)])
        elif c == 3:
            param[b] = (50 * np.random.rand(1) - 25).item()
        elif c == 4:
            std = 14 * np.random.rand() + 2
            if host_noise:
                if noise is None:
                    noise = np.zeros((B, H, W), np.float64)
                noise[b] = np.random.normal(0.0, std, (H, W))      # already scaled: the launch multiplies by 1
                param[b] = 1.0
            else:
                param[b] = std
        elif c == 5:
            cv["lines"][b] = _draw_lines((H, W))
            cv["nlines"][b], cv["segs"][b] = clip_segments(cv["lines"][b], (H, W))
        elif c == 6:
            ang = 30 * 2 * (np.random.rand(1) - 0.5).item()
            cv["ang_deg"][b] = ang
            cv["ang_rad"][b] = np.deg2rad(ang)
            cv["rot"][b] = invert_affine(rotation_matrix(cv["centre"], cv["ang_rad"][b]))
        choice[b] = min(c, 7)
    if cv2_params is not None:
        cv2_params.update(cv)
    return choice, param, lut, noise


def augment_cv(img, label, oimg, olabel, choice, cv):
    """The second launch (csrc/augment_cv.hip): rewrites the frames of ``oimg`` / ``olabel`` (which hold egne_augment's copy) whose
    ``choice`` is 1, 5 or 6 from ``img`` / ``label``; ``cv`` as draw() fills it (NumPy arrays of B rows)."""
    B, H, W = img.shape
    dev = img.device
    frame = np.ascontiguousarray(np.stack([np.asarray(choice, np.int32), np.asarray(cv["sigma"], np.int32),
                                           np.asarray(cv["nlines"], np.int32)], axis=1))
    frame_d = torch.from_numpy(frame).to(dev)
    segs_d = torch.from_numpy(np.ascontiguousarray(cv["segs"], dtype=np.float64)).to(dev)
    rot_d = torch.from_numpy(np.ascontiguousarray(cv["rot"], dtype=np.float64)).to(dev)
    q8_d, phase_d = device_table("augment_cv", dev, lambda: (gaussian_q8_tables(), lanczos4_phase_table()))
    _lib.check(_lib.lib().egne_augment_cv(img.data_ptr(), label.data_ptr(), frame_d.data_ptr(), frame.ctypes.data, segs_d.data_ptr(),
                                          rot_d.data_ptr(), q8_d.data_ptr(), phase_d.data_ptr(), oimg.data_ptr(), olabel.data_ptr(),
                                          B, H, W, _lib.stream_ptr()), "augment_cv")


def augment_batch(img, label, pupil_c, elParam, choices=None, host_noise=False, on_cv2="raise"):
    """img uint8 [B,H,W] and label int64 [B,H,W] on the device; pupil_c [B,2] and elParam [B,2,5] (pixels, radians) on any device.
    Returns (img, label, pupil_c, elParam, choice) with the geometry of flipped frames mirrored as data_augment.py:29-36 does
    (entries equal to -1 everywhere mark an absent centre / ellipse and stay untouched) and, with ``on_cv2="device"``, the geometry
    of rotated frames as data_augment.py:111-120 does."""
    require_cuda(img, "img")
    require_cuda(label, "label")
    if img.dtype != torch.uint8 or img.dim() != 3 or label.dtype != torch.int64 or label.shape != img.shape:
        raise ValueError("augment_batch: img must be uint8 [B,H,W] and label int64 of the same shape")
    img, label = img.contiguous(), label.contiguous()
    B, H, W = img.shape
    dev = img.device
    cv = {}
    choice, param, lut, noise = draw(B, (H, W), choices, host_noise, on_cv2, cv2_params=cv)
    if (choice == 4).any() and noise is None:
        noise_d = torch.randn((B, H, W), dtype=torch.float64, device=dev)
    else:
        noise_d = torch.from_numpy(noise).to(dev) if noise is not None else None
    ch_d, p_d, lut_d = (torch.from_numpy(a).to(dev) for a in (choice, param, lut))
    oimg, olab = torch.empty_like(img), torch.empty_like(label)
    _lib.check(_lib.lib().egne_augment(img.data_ptr(), label.data_ptr(), ch_d.data_ptr(), p_d.data_ptr(), lut_d.data_ptr(),
                                       noise_d.data_ptr() if noise_d is not None else None, oimg.data_ptr(), olab.data_ptr(),
                                       B, H, W, _lib.stream_ptr()), "augment")
    if np.isin(choice, CV2_CHOICES).any():
        augment_cv(img, label, oimg, olab, choice, cv)
    pc = torch.as_tensor(pupil_c).clone()
    el = torch.as_tensor(elParam).clone()
    flip = torch.from_numpy(choice == 0).to(pc.device)
    if bool(flip.any()):
        ok_c = flip & ~(pc == -1).all(dim=1)
        pc[:, 0] = torch.where(ok_c, W - pc[:, 0], pc[:, 0])
        for k in range(2):
            ok = flip & ~(el[:, k] == -1).all(dim=1)
            el[:, k, 0] = torch.where(ok, W - el[:, k, 0], el[:, k, 0])
            el[:, k, 4] = torch.where(ok, -el[:, k, 4], el[:, k, 4])
    rotated = np.nonzero(choice == 6)[0]
    if len(rotated):
        pc_h, el_h = pc.detach().cpu().double().numpy().copy(), el.detach().cpu().double().numpy().copy()
        for b in rotated:
            pc_h[b], el_h[b, 0], el_h[b, 1] = rotate_geometry(pc_h[b], el_h[b, 0], el_h[b, 1], cv["ang_rad"][b], cv["centre"])
        pc, el = torch.from_numpy(pc_h).to(pc), torch.from_numpy(el_h).to(el)
    return oimg, olab, pc, el, choice


def augment(base, mask, pupil_c, elParam, choice=None, on_cv2="raise"):
    """The reference's signature (data_augment.py:12): one NumPy frame in, (uint8 image, int mask, centre, (pupil, iris)) out,
    computed on cuda:0 through ``augment_batch`` with the reference's random stream (host-drawn noise).  ``on_cv2`` as in draw()."""
    dev = torch.device("cuda", torch.cuda.current_device()) if torch.cuda.is_available() else None
    if dev is None:
        raise RuntimeError("augment: no GPU (this path has no CPU fallback)")
    img = torch.from_numpy(np.ascontiguousarray(base, dtype=np.uint8))[None].to(dev)
    lab = torch.from_numpy(np.ascontiguousarray(mask).astype(np.int64))[None].to(dev)
    pc = torch.from_numpy(np.asarray(pupil_c, dtype=np.float64).copy())[None]
    el = torch.from_numpy(np.stack([np.asarray(elParam[0], dtype=np.float64), np.asarray(elParam[1], dtype=np.float64)]))[None]
    oi, ol, pc, el, _ = augment_batch(img, lab, pc, el, None if choice is None else [choice], host_noise=True, on_cv2=on_cv2)
    return oi[0].cpu().numpy(), ol[0].cpu().numpy(), pc[0].numpy(), (el[0, 0].numpy(), el[0, 1].numpy())
