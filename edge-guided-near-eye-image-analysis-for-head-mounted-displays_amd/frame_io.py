"""Frame I/O of the video scripts: the NumPy restatement of cv2.resize, the host front end (preprocess_frame) and back end
(rescale_to_original, plot_segmap_ellpreds) of evaluate.py, and the same on the device (csrc/evalio.hip): preprocess_frames_device,
render_frames_device, with the small constant tables they upload once per device (device_table)."""
import sys

import numpy as np
import torch


def resize_lanczos4(img, dsize):
    """cv2.resize(img, dsize=(width, height), interpolation=cv2.INTER_LANCZOS4) restated in NumPy (evaluate.py:76): separable
    8-tap Lanczos (a = 4) at source coordinate (dst + 0.5) * scale - 0.5, replicated border, uint8 in -> rounded uint8 out.
    OpenCV is not installed here, so this is checked against properties only (parity unpinned): OpenCV quantises the tap
    weights to 1/32-pixel tables in fixed point, which this float restatement does not."""
    W2, H2 = int(dsize[0]), int(dsize[1])
    src = np.asarray(img)
    out = src.astype(np.float64)
    for axis, n2 in ((0, H2), (1, W2)):
        n1 = out.shape[axis]
        if n1 == n2:
            continue
        idx, wts = lanczos4_table(n1, n2)
        g = np.take(out, idx.reshape(-1), axis=axis)
        shp = list(out.shape)
        shp[axis:axis + 1] = [n2, 8]
        g = g.reshape(shp)
        wshape = [1] * g.ndim
        wshape[axis], wshape[axis + 1] = n2, 8
        out = (g * wts.reshape(wshape)).sum(axis + 1)
    if src.dtype == np.uint8:
        return np.clip(np.rint(out), 0, 255).astype(np.uint8)
    return out.astype(src.dtype)


def resize_nearest(img, dsize):
    """cv2.resize(..., interpolation=cv2.INTER_NEAREST): src index = floor(dst * scale) (evaluate.py:190-191)."""
    W2, H2 = int(dsize[0]), int(dsize[1])
    a = np.asarray(img)
    return a[nearest_table(a.shape[0], H2)][:, nearest_table(a.shape[1], W2)]


def nearest_table(n1, n2):
    """Source indices of resize_nearest for one axis resized from ``n1`` to ``n2`` samples (int64 [n2])."""
    return np.minimum((np.arange(n2) * (n1 / n2)).astype(np.int64), n1 - 1)


def preprocess_frame(img, op_shape, align_width=True):
    """evaluate.py:69-104: scale to the target WIDTH (Lanczos), pad or centre-crop the rows, z-score.  Returns the
    [1,H,W] float32 tensor and scale_shift = (scale, rows added (+) or removed (-)).  (The reference's crop branch
    indexes with floats and raises; the centre crop it intends is what runs here.)"""
    if not align_width:
        sys.exit('Height alignment not implemented! Exiting ...')
    scale_shift = (1, 0)
    if op_shape[1] != img.shape[1]:
        sc = op_shape[1] / img.shape[1]
        img = resize_lanczos4(img, (int(img.shape[1] * sc), int(img.shape[0] * sc)))
        scale_shift = (sc, 0)
    if op_shape[0] > img.shape[0]:
        pad = op_shape[0] - img.shape[0]
        img = np.pad(img, ((pad // 2, pad - pad // 2), (0, 0)))
        scale_shift = (scale_shift[0], pad)
    elif op_shape[0] < img.shape[0]:
        cut = img.shape[0] - op_shape[0]
        img = img[cut // 2: cut // 2 + op_shape[0]]
        scale_shift = (scale_shift[0], -cut)
    img = img.astype(np.float64)
    img = (img - img.mean()) / img.std()
    return torch.from_numpy(img).unsqueeze(0).to(torch.float32), scale_shift


def rescale_to_original(seg_map, pupil_ellipse, iris_ellipse, scale_shift, orig_shape, edge_map=None):
    """evaluate.py:169-192: ellipses back to the source frame (row shift, then 1/scale), class map (and edge map) un-padded /
    re-padded and resized to the source shape with nearest neighbour.  Returns (seg_map, pupil, iris[, edge_map])."""
    pupil_ellipse, iris_ellipse = np.array(pupil_ellipse, dtype=np.float64), np.array(iris_ellipse, dtype=np.float64)
    for e in (pupil_ellipse, iris_ellipse):
        e[1] = e[1] - np.floor(scale_shift[1] // 2)
        e[:-1] = e[:-1] * (1 / scale_shift[0])

    def fix(m):
        if m is None:
            return None
        if scale_shift[1] > 0:
            m = m[scale_shift[1] // 2: m.shape[0] - (scale_shift[1] - scale_shift[1] // 2)]
        elif scale_shift[1] < 0:
            m = np.pad(m, ((-scale_shift[1] // 2, -scale_shift[1] - (-scale_shift[1] // 2)), (0, 0)))
        return resize_nearest(m, (orig_shape[1], orig_shape[0])) if tuple(m.shape[:2]) != tuple(orig_shape[:2]) else m
    seg_map, edge_map = fix(seg_map), fix(edge_map)
    return (seg_map, pupil_ellipse, iris_ellipse) if edge_map is None else (seg_map, pupil_ellipse, iris_ellipse, edge_map)


def _draw_ellipse(img, el, colour):
    """Outline of the ellipse (cx, cy, a, b, theta) as cv2.ellipse(..., thickness 1) would put it (helperfunctions.py:606-609;
    integer centre / axes as there), without anti-aliasing: 720 boundary samples rounded to pixels."""
    if np.all(np.asarray(el) == -1) or not np.all(np.isfinite(el)):
        return
    cx, cy, a, b = (int(v) for v in el[:4])
    t = np.linspace(0, 2 * np.pi, 720, endpoint=False)
    ang = float(el[4])
    x = cx + a * np.cos(t) * np.cos(ang) - b * np.sin(t) * np.sin(ang)
    y = cy + a * np.cos(t) * np.sin(ang) + b * np.sin(t) * np.cos(ang)
    xi, yi = np.rint(x).astype(np.int64), np.rint(y).astype(np.int64)
    ok = (xi >= 0) & (xi < img.shape[1]) & (yi >= 0) & (yi < img.shape[0])
    img[yi[ok], xi[ok]] = colour


def plot_segmap_ellpreds(image, seg_map, pupil_ellipse, iris_ellipse):
    """helperfunctions.py:521-622: grey frame -> BGR, iris pixels (120,183,53), pupil pixels (36,231,253), iris ellipse in
    (255,0,0) and pupil ellipse in (0,0,255)."""
    out = np.stack([image] * 3, axis=2).astype(np.uint8)
    out[seg_map == 1] = np.array([120, 183, 53], np.uint8)
    out[seg_map == 2] = np.array([36, 231, 253], np.uint8)
    _draw_ellipse(out, iris_ellipse, np.array([255, 0, 0], np.uint8))
    _draw_ellipse(out, pupil_ellipse, np.array([0, 0, 255], np.uint8))
    return out


_LANCZOS_TABLES, _DEVICE_TABLES = {}, {}


def lanczos4_table(n1, n2):
    """Tap tables of resize_lanczos4 for one axis resized from ``n1`` to ``n2`` samples: (indices int32 [n2,8], clamped to the border,
    weights float64 [n2,8], normalised) -- the same expressions, hence the same bits, as resize_lanczos4 evaluates.  Cached."""
    key = (int(n1), int(n2))
    if key not in _LANCZOS_TABLES:
        n1, n2 = key
        pos = (np.arange(n2) + 0.5) * (n1 / n2) - 0.5
        base = np.floor(pos).astype(np.int64)
        frac = pos - base
        taps = np.arange(-3, 5)                                        # 8 taps around the source position
        x = frac[:, None] - taps[None, :]
        with np.errstate(invalid="ignore", divide="ignore"):
            wts = np.where(np.abs(x) < 1e-12, 1.0, np.sin(np.pi * x) * np.sin(np.pi * x / 4) / (np.pi * np.pi * x * x / 4))
        wts = np.where(np.abs(x) < 4, wts, 0.0)
        wts /= wts.sum(1, keepdims=True)
        idx = np.clip(base[:, None] + taps[None, :], 0, n1 - 1)        # BORDER_REPLICATE
        _LANCZOS_TABLES[key] = (np.ascontiguousarray(idx.astype(np.int32)), np.ascontiguousarray(wts))
    return _LANCZOS_TABLES[key]


def device_table(key, device, make):
    """Small constant tables of the device code, uploaded once per device (not inside a graph capture: the eager warm-up runs of
    GraphedFrames come first).  One cache for the package; ``key`` names the table: ("lanczos", n1, n2), ("nearest", ...), "outline"
    here, ("jpeg", quality) and ("jpeg_header", ...) in mjpeg.py, "augment_cv" in data_augment.py."""
    k = (key, str(device))
    if k not in _DEVICE_TABLES:
        _DEVICE_TABLES[k] = tuple(torch.from_numpy(a).to(device) for a in make())
    return _DEVICE_TABLES[k]


def outline_table():
    t = np.linspace(0, 2 * np.pi, 720, endpoint=False)      # _draw_ellipse's samples
    return (np.stack([np.cos(t), np.sin(t)]),)


def prep_geometry(src_hw, op_shape):
    """The shape arithmetic of preprocess_frame for an eye of ``src_hw`` = (rows, columns): returns (resized rows, resized columns,
    scale_shift)."""
    He, We = int(src_hw[0]), int(src_hw[1])
    Ho, Wo = int(op_shape[0]), int(op_shape[1])
    Hr, Wr, scale_shift = He, We, (1, 0)
    if Wo != We:
        sc = Wo / We
        Wr, Hr = int(We * sc), int(He * sc)
        scale_shift = (sc, 0)
    if Ho > Hr:
        scale_shift = (scale_shift[0], Ho - Hr)
    elif Ho < Hr:
        scale_shift = (scale_shift[0], -(Hr - Ho))
    return Hr, Wr, scale_shift


def _check_frames(frames_u8, eyes, eye_width):
    from egne_amd.engine import require_cuda
    require_cuda(frames_u8, "frames_u8")
    if frames_u8.dtype != torch.uint8 or frames_u8.dim() != 3:
        raise ValueError("frames_u8 must be a uint8 [N,H,W] tensor")
    if eyes < 1 or eye_width < 1 or eyes * eye_width > frames_u8.shape[2]:
        raise ValueError("%d eyes of %d columns do not fit frames of %d columns" % (eyes, eye_width, frames_u8.shape[2]))
    return frames_u8.contiguous()


def preprocess_frames_device(frames_u8, op_shape, eyes=2, eye_width=320, return_u8=False):
    """preprocess_frame(grey, op_shape, align_width=True) of every eye of a batch of video frames, on the device (egne_eval_prep):
    ``frames_u8`` uint8 [N,Hs,Ws] on the GPU, eye i of a frame = columns [i*eye_width, (i+1)*eye_width).  Returns (x float32
    [N*eyes,1,Ho,Wo], frame-major then eye -- bit-identical to the stacked host results --, scale_shift); with ``return_u8`` also the
    uint8 image [N*eyes,Ho,Wo] after resize / pad / crop, before the z-score.  Queues on the current stream, no synchronisation."""
    from egne_amd import _lib
    f = _check_frames(frames_u8, eyes, eye_width)
    N, Hs, Ws = f.shape
    Ho, Wo = int(op_shape[0]), int(op_shape[1])
    Hr, Wr, scale_shift = prep_geometry((Hs, eye_width), (Ho, Wo))
    if Wr != Wo or Hr < 1:
        raise ValueError("eyes of %dx%d resize to %dx%d, not to the target width %d" % (Hs, eye_width, Hr, Wr, Wo))
    L = _lib.lib()
    rows = device_table(("lanczos", Hs, Hr), f.device, lambda: lanczos4_table(Hs, Hr)) if Hr != Hs else (None, None)
    cols = device_table(("lanczos", eye_width, Wr), f.device, lambda: lanczos4_table(eye_width, Wr)) if Wr != eye_width else (None, None)
    resize = int(rows[0] is not None or cols[0] is not None)
    x = torch.empty((N * eyes, 1, Ho, Wo), dtype=torch.float32, device=f.device)
    u8 = torch.empty((N * eyes, Ho, Wo), dtype=torch.uint8, device=f.device) if return_u8 else None
    ws = torch.empty(int(L.egne_eval_prep_workspace_bytes(N, eyes, Hr, Wr, resize)), dtype=torch.uint8, device=f.device)
    ptr = lambda t: None if t is None else t.data_ptr()       # noqa: E731
    _lib.check(L.egne_eval_prep(f.data_ptr(), N, Hs, Ws, eyes, eye_width, Hr, Wr, ptr(rows[0]), ptr(rows[1]), ptr(cols[0]), ptr(cols[1]),
                                Ho, Wo, x.data_ptr(), ptr(u8), ws.data_ptr(), _lib.stream_ptr()), "eval_prep")
    return (x, scale_shift, u8) if return_u8 else (x, scale_shift)


def render_frames_device(frames_u8, edge, seg, fit, scale_shift, eyes=2, eye_width=320):
    """The back end of draw() on the device (egne_eval_render): ``frames_u8`` uint8 [N,Hs,Ws] (the frames the maps were computed
    from), ``edge`` float32 [N*eyes,Ho,Wo], ``seg`` int64 [N*eyes,Ho,Wo] (model.predictions()), ``fit`` float64 [N*eyes,2,5] (iris,
    pupil) as fit_ellipses_from_pred leaves it, ``scale_shift`` from preprocess_frames_device.  Returns device tensors (overlay uint8
    [N,Hs,Ws,3] BGR, edge frame uint8 [N,Hs,Ws,3], ellipses float64 [N*eyes,2,5] at source geometry) -- byte for byte what
    rescale_to_original + plot_segmap_ellpreds + the edge-frame expression give per eye.  No synchronisation."""
    from egne_amd import _lib
    from egne_amd.engine import require_cuda
    f = _check_frames(frames_u8, eyes, eye_width)
    N, Hs, Ws = f.shape
    E = N * eyes
    for t, what in ((edge, "edge"), (seg, "seg"), (fit, "fit")):
        require_cuda(t, what)
    if seg.dtype != torch.int64 or seg.dim() != 3 or seg.shape[0] != E:
        raise ValueError("seg must be an int64 [%d,Ho,Wo] tensor" % E)
    if edge.dtype != torch.float32 or tuple(edge.shape) != tuple(seg.shape):
        raise ValueError("edge must be a float32 tensor of the class maps' shape %s" % (tuple(seg.shape),))
    if fit.dtype != torch.float64 or tuple(fit.shape) != (E, 2, 5):
        raise ValueError("fit must be a float64 [%d,2,5] tensor" % E)
    Ho, Wo = int(seg.shape[1]), int(seg.shape[2])
    scale, shift = scale_shift
    if int(shift) != shift or shift >= Ho or not scale > 0:
        raise ValueError("scale_shift %r does not belong to maps of %d rows" % (scale_shift, Ho))
    cs, = device_table("outline", f.device, outline_table)
    overlay = torch.empty((N, Hs, Ws, 3), dtype=torch.uint8, device=f.device)
    edge_frame = torch.empty_like(overlay)
    ell = torch.empty((E, 2, 5), dtype=torch.float64, device=f.device)
    edge, seg, fit = edge.contiguous(), seg.contiguous(), fit.contiguous()
    _lib.check(_lib.lib().egne_eval_render(f.data_ptr(), N, Hs, Ws, eyes, eye_width, seg.data_ptr(), edge.data_ptr(), fit.data_ptr(), Ho, Wo,
                                           1 / scale, int(shift), cs.data_ptr(), overlay.data_ptr(), edge_frame.data_ptr(), ell.data_ptr(),
                                           _lib.stream_ptr()), "eval_render")
    return overlay, edge_frame, ell
