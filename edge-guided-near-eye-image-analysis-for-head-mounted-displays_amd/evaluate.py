#!/usr/bin/env python3
"""Video / frame inference entry point -- the reference's evaluate.py (edge -> seg -> ellipse fit).

The per-image path (evaluate.py:105-166) runs on the HIP kernels; the two ellipses of a frame are fitted
by one device launch.  OpenCV is not available in this image: MJPEG .avi files (the format of
videos/example1.avi) are decoded with PIL, results go to <video>_ellipses.npy instead of an overlay video.

    python evaluate.py --path2data videos [--max_frames 20]
    python evaluate.py --synthetic 4
    python evaluate.py --path2data videos --low_latency 1 --device_io 1     (frame prep and overlay rendering on the device)
    python evaluate.py --path2data videos --device_io 1 --device_jpeg 1     (frame number and Motion-JPEG encoding on the device too)
    python evaluate.py --path2data videos --device_io 1 --device_jpeg 1 --device_decode 1     (and the input's Motion-JPEG decoding)
    python evaluate.py --path2data videos --ellipse_seed mask     (ellipse seeds from the class map instead of the regression head)
    python evaluate.py --path2data videos --ellipse_seed ransac   (seeds from the reference's ElliFit + RANSAC on the class map's boundaries)
    python evaluate.py --path2data videos --clean_mask 1          (the class map cleaned on the device before anything reads it)
"""
import argparse
import glob
import io
import os
import re
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import egne_amd  # noqa: E402,F401
from egne_amd import _entry  # noqa: E402

import numpy as np  # noqa: E402
import torch  # noqa: E402

from egne_amd.utils import fit_ellipses_from_mask, fit_ellipses_from_pred  # noqa: E402


def parse_args(argv=None):
    p = argparse.ArgumentParser()                               # evaluate.py:33-65
    p.add_argument('--vid_ext', type=str, default='avi')
    p.add_argument('--path2data', type=str, default='videos')
    p.add_argument('--align_width', type=int, default=1)
    p.add_argument('--method', type=str, default='baseline')
    p.add_argument('--model', type=str, default='ritnet_v2')                            # evaluate.py:37,362-367: 'ritnet_v2' | 'deepvog'
    p.add_argument('--loadfile', type=str, default='logs/baseline_edge_16.pkl')        # evaluate.py:357
    p.add_argument('--setting', type=str, default='configs/baseline_edge.yaml')        # evaluate.py:359
    p.add_argument('--max_frames', type=int, default=0)
    p.add_argument('--synthetic', type=int, default=0)
    p.add_argument('--low_latency', type=int, default=0)          # 1: the two eyes of a frame per call, results before the next frame
    p.add_argument('--eye_width', type=int, default=320)          # columns per eye of a video frame (two eyes side by side; evaluate.py:235-249: 320)
    p.add_argument('--device_io', type=int, default=0, choices=(0, 1))   # 1: frame prep and overlay rendering on the device (csrc/evalio.hip)
    p.add_argument('--device_jpeg', type=int, default=0, choices=(0, 1))  # 1: frame number and JPEG encoding on the device too (csrc/jpeg.hip); needs --device_io 1
    p.add_argument('--device_decode', type=int, default=0, choices=(0, 1))  # 1: the input's JPEG decoding on the device (csrc/jpeg_decode.hip); needs --device_io 1
    p.add_argument('--ellipse_seed', type=str, default='pred', choices=('pred', 'mask', 'ransac'))   # mask: the searches are seeded from the class map (csrc/mask_seed.hip); ransac: from ElliFit + RANSAC on its boundaries (csrc/ellifit.hip)
    p.add_argument('--clean_mask', type=int, default=0, choices=(0, 1))   # 1: the class map is cleaned on the device before anything reads it (csrc/cleanup.hip): 3x3 opening, largest blob, holes filled
    a = p.parse_args(argv)
    if a.device_jpeg and not a.device_io:
        p.error('--device_jpeg 1 encodes the frames that --device_io 1 renders on the device: it needs --device_io 1')
    if a.device_decode and not a.device_io:
        p.error('--device_decode 1 decodes into the frames that --device_io 1 prepares on the device: it needs --device_io 1')
    a.prec = torch.float32
    return a


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


SEED_REGIONS = {'ritnet_v2': None,                          # utils.DEFAULT_SEED_REGIONS: iris = classes 1 | 2 scored against 1, pupil = class 2
                'deepvog': ((0, 1), (0b010, 1))}            # class map {0, 1 = pupil}: no iris row, the pupil seeded from and scored against class 1


RANSAC_REGIONS = {'ritnet_v2': None,                        # utils.DEFAULT_RANSAC_REGIONS: iris boundary of classes 1 | 2, pupil boundary away from class 0
                  'deepvog': ((0, 1), (0b010, 1, 0))}


CLEAN_LAYERS = {'ritnet_v2': None,                         # utils.DEFAULT_CLEAN_LAYERS: the iris blob of classes 1 | 2, the pupil blob painted over it
                'deepvog': ((0b010, 1, 3),)}               # class map {0, 1 = pupil}: the pupil blob alone


def clean_of(args):
    """The ``clean`` keyword of _seg_and_fit for --clean_mask / --model: None (the raw argmax, as ever) or the layers of
    utils.clean_class_maps."""
    if args is None or not getattr(args, 'clean_mask', 0):
        return None
    from egne_amd.utils import DEFAULT_CLEAN_LAYERS
    return CLEAN_LAYERS.get(getattr(args, 'model', 'ritnet_v2')) or DEFAULT_CLEAN_LAYERS


def seed_of(args):
    """(seed, regions) of --ellipse_seed / --model: ('pred', None) unless the flag asks for the class map (mask: second moments of the
    largest component; ransac: ElliFit + RANSAC on the region's boundary, generated draws with seed 0 -- the same for every call)."""
    kind = 'pred' if args is None else getattr(args, 'ellipse_seed', 'pred')
    if kind == 'mask':
        return 'mask', SEED_REGIONS.get(getattr(args, 'model', 'ritnet_v2'))
    if kind == 'ransac':
        return 'ransac', RANSAC_REGIONS.get(getattr(args, 'model', 'ritnet_v2'))
    return 'pred', None


def _fit(mask, elPred, seed, regions):
    if seed == 'ransac':
        return fit_ellipses_from_mask(mask, regions, seed_kind='ransac')
    if seed == 'mask':
        return fit_ellipses_from_mask(mask, regions)
    return fit_ellipses_from_pred(mask, elPred)


def evaluate_ellseg_on_image(frames, model, edge_model, args=None):
    """evaluate.py:112-166 for a batch of frames [N,1,H,W] (the reference loops one frame at a time).
    Returns edge maps [N,H,W], class maps [N,H,W], pupil ellipses [N,5], iris ellipses [N,5] (pixels).  ``args``: where the seeds of
    the searches come from (seed_of)."""
    seed, regions = seed_of(args)
    from egne_amd.utils import calc_edge
    assert frames.dim() == 4, 'Frame must be [N,1,H,W]'
    ns = argparse.Namespace(prec=torch.float32, edge_thres=0)
    for attempt in (0, 1, 2):
        with torch.no_grad():
            edge = calc_edge(ns, frames, edge_model, frames.device)
        # a frame beyond the head-room of the calibrated f16 pre-scales (engine.Plan.overflowed): a plan re-calibrates on its next call, so
        # the frames simply run again.  The edge network's word is read BEFORE its map is fed on (a NaN map must not reach the model plan's
        # own calibration pass)
        if _overflowed(edge_model):
            continue
        res = _to_host(_seg_and_fit(frames, model, seed=seed, regions=regions, clean=clean_of(args))(edge))
        if not _overflowed(model):
            return res
    raise RuntimeError("non-finite activations after re-calibration: the input frames themselves are not finite")


def _overflowed(net):
    return bool(net.overflowed()) if hasattr(net, "overflowed") else False


def _seg_and_fit(frames, model, wfit=None, then=None, seed='pred', regions=None, clean=None):
    """Second stage of a batch (evaluate.py:117-166): ESF-Net on the frames and their edge maps, argmax mask, both ellipses
    fitted on the device.  Returns a callable of the edge maps (egne_amd.pipeline.TwoStagePipeline runs it on its second stream).
    ``wfit`` (egne_amd.pipeline.WindowedFit): the searches go to its stream and are released in the next batch's launch window; the
    third result is then a handle (``_to_host`` waits for it); ``then(edge, mask, fit)`` is queued on the searches' stream right behind
    them (the device-side rendering of --device_io 1).  ``seed`` / ``regions``: seed_of(args).  ``clean`` (clean_of(args)): layers
    of utils.clean_class_maps -- the class map is cleaned right behind model.predictions(), on the same stream, and seeds, search,
    renderers and the returned map all read the cleaned tensor (a fresh one per call: it lives as long as whoever holds it)."""
    dev = frames.device
    N, _, H, W = frames.shape

    def run(edge):
        with torch.no_grad():
            labels = torch.zeros((N, H, W), device=dev)
            labels[..., 0, 2] = 1                                  # evaluate.py:118-120: make all 3 classes present
            labels[..., 2, 2] = 2
            z = lambda *s: torch.zeros(s, device=dev)              # noqa: E731
            out = model(frames, edge, labels.long(), z(N, 2), z(N, 2, 5), z(N, H, W), z(N, 3, H, W), z(N, 4),
                        torch.zeros(N, dtype=torch.long, device=dev), 0)
            if clean is not None:
                from egne_amd.utils import clean_class_maps
                m = clean_class_maps(model.predictions(), clean)          # (the closure of WindowedFit.submit keeps it until its searches ran)
                if wfit is not None:
                    e = edge[:, 0].clone()
                    return e, m, wfit.submit(m, out[1], then=None if then is None else (lambda fit: then(e, m, fit)),
                                             seed=seed, regions=regions)
                return edge[:, 0].clone(), m, _fit(m, out[1], seed, regions)
            if wfit is not None:
                e, m = edge[:, 0].clone(), model.predictions().clone()
                return e, m, wfit.submit(model.predictions(), out[1], then=None if then is None else (lambda fit: then(e, m, fit)),
                                         seed=seed, regions=regions)
            fit = _fit(model.predictions(), out[1], seed, regions)        # [N,2,5] on the device: (iris, pupil)
            return edge[:, 0].clone(), model.predictions().clone(), fit
    return run


def graphed_runner(warmup_frames, model, edge_model, seed='pred', regions=None, clean=None):
    """edge -> seg -> fit of a fixed small batch as one hipGraph replay (egne_amd.pipeline.GraphedFrames): the per-eye loop of
    evaluate.py:235-249 at one or two frames per call.  ``runner(frames)`` returns the same device tensors as the eager path (edge maps
    [N,H,W], class maps [N,H,W], fitted ellipses [N,2,5]); results are bit-identical to it."""
    from egne_amd.pipeline import GraphedFrames
    from egne_amd.utils import calc_edge
    ns = argparse.Namespace(prec=torch.float32, edge_thres=0)

    def stage(x):
        return _seg_and_fit(x, model, seed=seed, regions=regions, clean=clean)(calc_edge(ns, x, edge_model, x.device))
    return GraphedFrames(stage, warmup_frames)


def graphed_runner_io(warmup_u8, model, edge_model, op_shape=(240, 320), eyes=2, eye_width=320, seed='pred', regions=None, clean=None):
    """graphed_runner with the device front and back end INSIDE the captured graph: uint8 frames [N,Hs,Ws] in, (overlay, edge frame,
    ellipses at source geometry) out -- prep, edge, seg, fit and rendering are one replay.  Capture allows it: shapes are fixed, the
    tap tables are uploaded by the eager warm-up runs, nothing in the two stages synchronises."""
    from egne_amd.pipeline import GraphedFrames
    from egne_amd.utils import calc_edge
    ns = argparse.Namespace(prec=torch.float32, edge_thres=0)

    def stage(fu):
        x, ss = preprocess_frames_device(fu, op_shape, eyes, eye_width)
        edge, seg, fit = _seg_and_fit(x, model, seed=seed, regions=regions, clean=clean)(calc_edge(ns, x, edge_model, x.device))
        return render_frames_device(fu, edge, seg, fit, ss, eyes, eye_width)
    return GraphedFrames(stage, warmup_u8)


def evaluate_frames_device_io(frames_u8, model, edge_model, op_shape=(240, 320), eyes=2, eye_width=320, seed='pred', regions=None,
                              clean=None):
    """evaluate_ellseg_on_image from uint8 device frames to rendered device frames (eager; the redo path of --device_io 1): the same
    re-calibration retries, nothing crosses to the host but the plans' overflow words."""
    from egne_amd.utils import calc_edge
    ns = argparse.Namespace(prec=torch.float32, edge_thres=0)
    x, ss = preprocess_frames_device(frames_u8, op_shape, eyes, eye_width)
    for attempt in (0, 1, 2):
        with torch.no_grad():
            edge = calc_edge(ns, x, edge_model, x.device)
        if _overflowed(edge_model):
            continue
        e, m, fit = _seg_and_fit(x, model, seed=seed, regions=regions, clean=clean)(edge)
        if not _overflowed(model):
            return render_frames_device(frames_u8, e, m, fit, ss, eyes, eye_width)
    raise RuntimeError("non-finite activations after re-calibration: the input frames themselves are not finite")


def _upload_u8(frames, device):
    """The only host -> device copy of --device_io 1: the decoded frames as they are, uint8 [N,Hs,Ws]."""
    return torch.from_numpy(np.ascontiguousarray(frames)).to(device)


def _download(t):
    """The only device -> host copies of --device_io 1 go through here: two uint8 BGR frames and 20 doubles per eye (with
    --device_jpeg 1: the streams' lengths and flags, their used bytes in one buffer, and 20 doubles per eye)."""
    return t.cpu().numpy()


def _encode_rendered(batch):
    """--device_jpeg 1, right behind the rendering on its stream: the frame numbers go into a copy of the overlay (a frame whose
    stream does not fit is drawn by the host from the untouched one), both stacks are encoded."""
    overlay, edge_frame, _ = batch.rendered
    stamped = _stamp_masks_device(overlay.clone(), batch.masks)
    batch.encoded = encode_jpeg_device(stamped) + encode_jpeg_device(edge_frame)


class _Batch(list):
    """Frames of a batch whose results are still on the device; with --device_io 1 also their uint8 device copy (kept for the
    rendering and for a redo) and the rendered tensors once the fit's stream has queued them; with --device_jpeg 1 also the frame
    numbers' masks on the device and the encoded streams; with --device_decode 1 the decoder's flags (int32 [N], on the device)."""
    fu = None
    dflags = None
    rendered = None
    masks = None
    encoded = None


def _to_host(res):
    edge, mask, fit = res
    if not torch.is_tensor(fit):       # WindowedFit.Handle: the searches may still be waiting for their window
        fit.synchronize()
        fit = fit.result
    fit = fit.cpu().numpy()
    return edge.cpu().numpy(), mask.cpu().numpy(), fit[:, 1], fit[:, 0]


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
        taps = np.arange(-3, 5)
        x = frac[:, None] - taps[None, :]
        with np.errstate(invalid="ignore", divide="ignore"):
            wts = np.where(np.abs(x) < 1e-12, 1.0, np.sin(np.pi * x) * np.sin(np.pi * x / 4) / (np.pi * np.pi * x * x / 4))
        wts = np.where(np.abs(x) < 4, wts, 0.0)
        wts /= wts.sum(1, keepdims=True)
        idx = np.clip(base[:, None] + taps[None, :], 0, n1 - 1)
        _LANCZOS_TABLES[key] = (np.ascontiguousarray(idx.astype(np.int32)), np.ascontiguousarray(wts))
    return _LANCZOS_TABLES[key]


def _device_table(key, device, make):
    """Small constant tables of the device front / back end, uploaded once per device (not inside a graph capture: the eager
    warm-up runs of GraphedFrames come first)."""
    k = (key, str(device))
    if k not in _DEVICE_TABLES:
        _DEVICE_TABLES[k] = tuple(torch.from_numpy(a).to(device) for a in make())
    return _DEVICE_TABLES[k]


def _outline_table():
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
    rows = _device_table(("lanczos", Hs, Hr), f.device, lambda: lanczos4_table(Hs, Hr)) if Hr != Hs else (None, None)
    cols = _device_table(("lanczos", eye_width, Wr), f.device, lambda: lanczos4_table(eye_width, Wr)) if Wr != eye_width else (None, None)
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
    cs, = _device_table("outline", f.device, _outline_table)
    overlay = torch.empty((N, Hs, Ws, 3), dtype=torch.uint8, device=f.device)
    edge_frame = torch.empty_like(overlay)
    ell = torch.empty((E, 2, 5), dtype=torch.float64, device=f.device)
    edge, seg, fit = edge.contiguous(), seg.contiguous(), fit.contiguous()
    _lib.check(_lib.lib().egne_eval_render(f.data_ptr(), N, Hs, Ws, eyes, eye_width, seg.data_ptr(), edge.data_ptr(), fit.data_ptr(), Ho, Wo,
                                           1 / scale, int(shift), cs.data_ptr(), overlay.data_ptr(), edge_frame.data_ptr(), ell.data_ptr(),
                                           _lib.stream_ptr()), "eval_render")
    return overlay, edge_frame, ell


# ---- Motion-JPEG on the device (--device_jpeg 1; csrc/jpeg.hip) -- ITU-T T.81 baseline in a JFIF wrapper, tables of its Annex K ---------
JPEG_RESTART_MCUS = 4          # MCUs (16 x 16 pixels) per restart interval = per wave of the entropy coder: 150 intervals in a 640 x 240 frame
_JPEG_ZIGZAG = (0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28,
                35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63)
_JPEG_LUMA_Q = (16, 11, 10, 16, 24, 40, 51, 61,             # table K.1, rows = vertical frequency
                12, 12, 14, 19, 26, 58, 60, 55,
                14, 13, 16, 24, 40, 57, 69, 56,
                14, 17, 22, 29, 51, 87, 80, 62,
                18, 22, 37, 56, 68, 109, 103, 77,
                24, 35, 55, 64, 81, 104, 113, 92,
                49, 64, 78, 87, 103, 121, 120, 101,
                72, 92, 95, 98, 112, 100, 103, 99)
_JPEG_CHROMA_Q = (17, 18, 24, 47, 99, 99, 99, 99,           # table K.2
                  18, 21, 26, 66, 99, 99, 99, 99,
                  24, 26, 56, 99, 99, 99, 99, 99,
                  47, 66, 99, 99, 99, 99, 99, 99) + (99,) * 32
# tables K.3 - K.6: (number of codes of length 1..16, symbols in code order); an AC symbol is run << 4 | category
_JPEG_HUFF = (
    ((0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0), tuple(range(12))),                                   # DC luminance
    ((0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 125),                                                    # AC luminance
     (0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71,
      0x14, 0x32, 0x81, 0x91, 0xa1, 0x08, 0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72,
      0x82, 0x09, 0x0a, 0x16, 0x17, 0x18, 0x19, 0x1a, 0x25, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x34, 0x35, 0x36, 0x37,
      0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59,
      0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x83,
      0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3,
      0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3,
      0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2,
      0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa)),
    ((0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0), tuple(range(12))),                                   # DC chrominance
    ((0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 119),                                                    # AC chrominance
     (0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22,
      0x32, 0x81, 0x08, 0x14, 0x42, 0x91, 0xa1, 0xb1, 0xc1, 0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1,
      0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25, 0xf1, 0x17, 0x18, 0x19, 0x1a, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x35, 0x36,
      0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58,
      0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a,
      0x82, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a,
      0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba,
      0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda,
      0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa)),
)
_JPEG_TABLES, _JPEG_HEADERS = {}, {}


def jpeg_tables(quality):
    """The tables egne_jpeg_encode takes (include/egne_hip.h), as NumPy arrays: (qt uint8 [2,64], the luminance / chrominance divisors
    in zigzag order -- libjpeg's quality scaling of tables K.1 / K.2 --, huff uint32 [544], (code length << 16) | code of the four
    Annex K code tables, dct int32 [8,8], T[u][x] = rint(8192 a(u) cos((2x+1) u pi / 16)) computed in float64).  Cached."""
    quality = int(quality)
    if not 1 <= quality <= 100:
        raise ValueError("JPEG quality %d outside 1..100" % quality)
    if quality not in _JPEG_TABLES:
        scale = 5000 // quality if quality < 50 else 200 - 2 * quality
        qt = np.array([[min(max((base[n] * scale + 50) // 100, 1), 255) for n in _JPEG_ZIGZAG] for base in (_JPEG_LUMA_Q, _JPEG_CHROMA_Q)], np.uint8)
        huff = np.zeros(544, np.uint32)
        for (counts, symbols), first in zip(_JPEG_HUFF, (0, 32, 16, 288)):
            code, k = 0, 0
            for length in range(1, 17):                     # T.81 Annex C: codes of one length are consecutive, then a zero bit is appended
                for _ in range(counts[length - 1]):
                    huff[first + symbols[k]] = length << 16 | code
                    code, k = code + 1, k + 1
                code <<= 1
        u, x = np.arange(8, dtype=np.float64)[:, None], np.arange(8, dtype=np.float64)[None, :]
        a = np.where(u == 0, np.sqrt(1.0 / 8.0), np.sqrt(2.0 / 8.0))
        dct = np.rint(8192.0 * a * np.cos((2 * x + 1) * u * np.pi / 16)).astype(np.int32)
        _JPEG_TABLES[quality] = (qt, huff, np.ascontiguousarray(dct))
    return _JPEG_TABLES[quality]


def jpeg_header(W, H, quality, restart_mcus=JPEG_RESTART_MCUS):
    """Everything of a frame's JPEG file in front of the entropy-coded scan: SOI, APP0 (JFIF 1.1), two DQT, SOF0 (8 bit, H x W, Y 2x2,
    Cb 1x1, Cr 1x1), the four DHT, DRI, SOS.  ``restart_mcus`` 1..8: what egne_jpeg_encode's LDS staging is sized for.  Cached."""
    W, H, quality, restart_mcus = int(W), int(H), int(quality), int(restart_mcus)
    if not (1 <= W <= 65535 and 1 <= H <= 65535 and 1 <= restart_mcus <= 8):
        raise ValueError("JPEG frame %dx%d / restart interval %d out of range (1..65535, 1..8 MCUs)" % (W, H, restart_mcus))
    key = (W, H, quality, restart_mcus)
    if key not in _JPEG_HEADERS:
        _JPEG_HEADERS[key] = _build_jpeg_header(*key)
    return _JPEG_HEADERS[key]


def _build_jpeg_header(W, H, quality, restart_mcus):
    qt = jpeg_tables(quality)[0]

    def seg(marker, body):
        return bytes((0xFF, marker)) + (len(body) + 2).to_bytes(2, 'big') + body
    h = b'\xff\xd8' + seg(0xE0, b'JFIF\x00\x01\x01\x00\x00\x01\x00\x01\x00\x00')
    h += seg(0xDB, b'\x00' + qt[0].tobytes()) + seg(0xDB, b'\x01' + qt[1].tobytes())
    h += seg(0xC0, b'\x08' + H.to_bytes(2, 'big') + W.to_bytes(2, 'big') + bytes((3, 1, 0x22, 0, 2, 0x11, 1, 3, 0x11, 1)))
    for (counts, symbols), tc_th in zip(_JPEG_HUFF, (0x00, 0x10, 0x01, 0x11)):
        h += seg(0xC4, bytes((tc_th,)) + bytes(counts) + bytes(symbols))
    h += seg(0xDD, restart_mcus.to_bytes(2, 'big'))
    return h + seg(0xDA, bytes((3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0)))


def encode_jpeg_device(frames_bgr_u8, quality=90, cap=None):
    """Baseline JPEG files of a stack of uint8 BGR device frames [N,H,W,3] (egne_jpeg_encode): returns device tensors (out uint8
    [N,cap], frame n's file in out[n, :lengths[n]]; lengths int32 [N]; flags int32 [N], 1 where the file did not fit ``cap`` bytes --
    its length is then 0).  ``cap`` defaults to the header plus 1.5 bytes per pixel of the frame padded to multiples of 16.  Queues on
    the current stream, no synchronisation."""
    from egne_amd import _lib
    from egne_amd.engine import require_cuda
    f = frames_bgr_u8
    require_cuda(f, "frames_bgr_u8")
    if f.dtype != torch.uint8 or f.dim() != 4 or f.shape[3] != 3 or min(f.shape) < 1:
        raise ValueError("frames_bgr_u8 must be a uint8 [N,H,W,3] tensor")
    f = f.contiguous()
    N, H, W = int(f.shape[0]), int(f.shape[1]), int(f.shape[2])
    header = jpeg_header(W, H, quality, JPEG_RESTART_MCUS)
    if cap is None:
        cap = len(header) + (-(-H // 16) * 16) * (-(-W // 16) * 16) * 3 // 2
    cap = int(cap)
    if cap < 1:
        raise ValueError("cap must be positive")
    qt, huff, dct = _device_table(("jpeg", int(quality)), f.device, lambda: jpeg_tables(quality))
    hd, = _device_table(("jpeg_header", W, H, int(quality)), f.device, lambda: (np.frombuffer(header, np.uint8).copy(),))
    L = _lib.lib()
    out = torch.empty((N, cap), dtype=torch.uint8, device=f.device)
    lengths = torch.empty(N, dtype=torch.int32, device=f.device)
    flags = torch.empty(N, dtype=torch.int32, device=f.device)
    ws = torch.empty(int(L.egne_jpeg_workspace_bytes(N, H, W)), dtype=torch.uint8, device=f.device)
    _lib.check(L.egne_jpeg_encode(f.data_ptr(), N, H, W, qt.data_ptr(), huff.data_ptr(), dct.data_ptr(), hd.data_ptr(), len(header),
                                  JPEG_RESTART_MCUS, out.data_ptr(), cap, lengths.data_ptr(), flags.data_ptr(), ws.data_ptr(),
                                  _lib.stream_ptr()), "jpeg_encode")
    return out, lengths, flags


_STAMP_PATCH = (16, 64, 8, 10)         # rows, columns, x0, y0 of the patch that holds the frame number: asserted per number below


def frame_number_mask(j, ph=_STAMP_PATCH[0], pw=_STAMP_PATCH[1], x0=_STAMP_PATCH[2], y0=_STAMP_PATCH[3]):
    """The coverage mask of _put_frame_number's text: str(j) in white on a black 'L' canvas at (10, 12), same default font; returns
    the uint8 [ph,pw] patch at origin (x0, y0), which must hold everything PIL draws (asserted)."""
    from PIL import Image, ImageDraw
    canvas = Image.new('L', (max(x0 + pw, 0) + 128, max(y0 + ph, 0) + 64), 0)
    ImageDraw.Draw(canvas).text((10, 12), str(j), fill=255)
    box = canvas.getbbox()
    if box is not None and not (x0 <= box[0] and y0 <= box[1] and box[2] <= x0 + pw and box[3] <= y0 + ph and
                                box[2] < canvas.size[0] and box[3] < canvas.size[1]):
        raise AssertionError("frame number %r covers %r, outside the %dx%d patch at (%d, %d)" % (j, box, pw, ph, x0, y0))
    full = np.asarray(canvas)
    patch = np.zeros((ph, pw), np.uint8)
    ys, xs = max(y0, 0), max(x0, 0)
    patch[ys - y0:, xs - x0:] = full[ys: y0 + ph, xs: x0 + pw]
    return patch


def stamp_numbers_device(frames, numbers):
    """_put_frame_number(frames[n], numbers[n]) on the device, in place (egne_stamp_mask): ``frames`` uint8 [N,H,W,3] BGR on the GPU.
    The host only draws the numbers' small coverage masks.  Current stream, no synchronisation of the device work."""
    masks = torch.from_numpy(np.stack([frame_number_mask(j) for j in numbers]))
    return _stamp_masks_device(frames, masks.to(frames.device))


def _stamp_masks_device(frames, masks):
    from egne_amd import _lib
    from egne_amd.engine import require_cuda
    require_cuda(frames, "frames")
    if frames.dtype != torch.uint8 or frames.dim() != 4 or frames.shape[3] != 3 or not frames.is_contiguous():
        raise ValueError("frames must be a contiguous uint8 [N,H,W,3] tensor")
    if masks.dtype != torch.uint8 or masks.dim() != 3 or masks.shape[0] != frames.shape[0]:
        raise ValueError("one uint8 mask per frame")
    N, H, W = (int(v) for v in frames.shape[:3])
    masks = masks.contiguous()
    _lib.check(_lib.lib().egne_stamp_mask(frames.data_ptr(), N, H, W, masks.data_ptr(), int(masks.shape[1]), int(masks.shape[2]),
                                          _STAMP_PATCH[2], _STAMP_PATCH[3], 0, 0, 255, _lib.stream_ptr()), "stamp_mask")
    return frames


class MJPEGWriter:
    """Minimal AVI (RIFF) writer with Motion-JPEG frames encoded by PIL -- stands in for cv2.VideoWriter (evaluate.py:219-221;
    the reference writes mp4v, for which there is no encoder in this image).  Frames are BGR uint8 arrays as OpenCV's are."""

    def __init__(self, path, fps, size):
        self.path, self.fps, self.size, self.frames = path, max(int(fps), 1), (int(size[0]), int(size[1])), []

    def write(self, frame_bgr):
        from PIL import Image
        buf = io.BytesIO()
        Image.fromarray(np.ascontiguousarray(frame_bgr[..., ::-1])).save(buf, format='JPEG', quality=90)
        self.frames.append(buf.getvalue())

    def write_jpeg(self, data):
        """Append a frame that is a complete JPEG file already (encode_jpeg_device)."""
        self.frames.append(bytes(data))

    def release(self):
        import struct
        W, H, n = self.size[0], self.size[1], len(self.frames)
        chunks, idx, off = [], [], 4
        for f in self.frames:
            pad = len(f) & 1
            chunks.append(b'00dc' + struct.pack('<I', len(f)) + f + b'\0' * pad)
            idx.append(b'00dc' + struct.pack('<III', 0x10, off, len(f)))
            off += 8 + len(f) + pad
        movi = b'movi' + b''.join(chunks)
        biggest = max((len(f) for f in self.frames), default=0)
        avih = struct.pack('<IIIIIIIIIIIIII', 1000000 // self.fps, biggest * self.fps, 0, 0x10, n, 0, 1, biggest, W, H, 0, 0, 0, 0)
        strh = b'vids' + b'MJPG' + struct.pack('<IHHIIIIIIIIhhhh', 0, 0, 0, 0, 1, self.fps, 0, n, biggest, 0xffffffff, 0, 0, 0, W, H)
        strf = struct.pack('<IiiHHIIiiII', 40, W, H, 1, 24, 0x47504a4d, W * H * 3, 0, 0, 0, 0)

        def ck(tag, data):
            return tag + struct.pack('<I', len(data)) + data + (b'\0' if len(data) & 1 else b'')

        def lst(tag, data):
            return b'LIST' + struct.pack('<I', len(data) + 4) + tag + data
        hdrl = lst(b'hdrl', ck(b'avih', avih) + lst(b'strl', ck(b'strh', strh) + ck(b'strf', strf)))
        body = b'AVI ' + hdrl + b'LIST' + struct.pack('<I', len(movi)) + movi + ck(b'idx1', b''.join(idx))
        with open(self.path, 'wb') as f:
            f.write(b'RIFF' + struct.pack('<I', len(body)) + body)


def mjpeg_frames(path):
    """Yield grey frames of an MJPEG .avi by scanning for JPEG SOI/EOI markers (no OpenCV)."""
    from PIL import Image
    data = open(path, 'rb').read()
    pos = 0
    while True:
        a = data.find(b'\xff\xd8\xff', pos)
        if a < 0:
            return
        b = data.find(b'\xff\xd9', a)
        if b < 0:
            return
        pos = b + 2
        try:
            yield np.asarray(Image.open(io.BytesIO(data[a:b + 2])).convert('L'))
        except Exception:
            continue


def mjpeg_chunks(path):
    """Yield the JPEG files of an MJPEG .avi as byte strings: the SOI/EOI scan of mjpeg_frames, nothing decoded."""
    data = open(path, 'rb').read()
    pos = 0
    while True:
        a = data.find(b'\xff\xd8\xff', pos)
        if a < 0:
            return
        b = data.find(b'\xff\xd9', a)
        if b < 0:
            return
        pos = b + 2
        yield data[a:b + 2]


def _decode_host(data):
    """The host path of a frame: PIL, as mjpeg_frames; None where PIL cannot decode it."""
    from PIL import Image
    try:
        return np.array(Image.open(io.BytesIO(data)).convert('L'))
    except Exception:
        return None


# ---- Motion-JPEG decoding on the device (--device_decode 1; csrc/jpeg_decode.hip) ------------------------------------------------------
JPEG_GREY, JPEG_444, JPEG_422, JPEG_420 = 0, 1, 2, 3          # `sampling` of egne_jpeg_decode
JPEG_DESC_BYTES = 1408                                        # one frame's record of egne_jpeg_decode (include/egne_hip.h)
_JPEG_FOREIGN_MARKER = re.compile(b'\xff[^\x00\xd0-\xd7]')     # in a scan: anything but stuffing and RSTm (a second scan, fill bytes, ...)
_PARSED_HEADER = [None, None]                                 # the last header jpeg_parse walked, and what it found there


def _parse_header(data):
    """The marker segments of a JPEG file up to and including SOS: a dictionary (see jpeg_parse; 'scan_off' = where the scan starts,
    'record' = the frame's descriptor without its scan), or None."""
    n = len(data)
    if n < 4 or data[:2] != b'\xff\xd8':
        return None
    p, qt, huff, restart, sof = 2, {}, {}, 0, None
    while True:
        if p + 4 > n or data[p] != 0xFF:
            return None
        m = data[p + 1]
        L = int.from_bytes(data[p + 2: p + 4], 'big')
        if m in (0x01, 0xD8, 0xD9, 0xFF) or 0xD0 <= m <= 0xD7 or L < 2 or p + 2 + L > n:
            return None
        b = data[p + 4: p + 2 + L]
        if m == 0xDB:
            for k in range(0, len(b), 65):
                if b[k] > 3 or k + 65 > len(b):                # 16-bit divisors (Pq = 1), a table number above 3, a short segment
                    return None
                qt[b[k]] = b[k + 1: k + 65]
        elif m == 0xC4:
            k = 0
            while k < len(b):
                if k + 17 > len(b):
                    return None
                counts = b[k + 1: k + 17]
                nsym, code = sum(counts), 0
                for length in range(16):                       # the codes must fit their lengths (T.81 Annex C)
                    code = (code + counts[length]) << 1
                    if code > 2 << (length + 1):
                        return None
                if b[k] not in (0x00, 0x01, 0x10, 0x11) or nsym > 256 or k + 17 + nsym > len(b):
                    return None
                huff[b[k]] = (bytes(counts), bytes(b[k + 17: k + 17 + nsym]))
                k += 17 + nsym
        elif m == 0xC0:
            if sof is not None or len(b) < 6 or b[0] != 8 or len(b) != 6 + 3 * b[5]:
                return None
            sof = (int.from_bytes(b[1:3], 'big'), int.from_bytes(b[3:5], 'big'),
                   [(b[6 + 3 * i], b[7 + 3 * i] >> 4, b[7 + 3 * i] & 15, b[8 + 3 * i]) for i in range(b[5])])
        elif 0xC1 <= m <= 0xCF:                                # every other frame type: extended, progressive, lossless, arithmetic
            return None
        elif m == 0xDD:
            if len(b) != 2:
                return None
            restart = int.from_bytes(b, 'big')
        elif m == 0xEE and b[:5] == b'Adobe' and len(b) >= 12 and b[11] != 1:
            return None                                        # Adobe transform 0 / 2: the components are RGB or YCCK, not YCbCr
        elif m == 0xDA:
            break
        p += 2 + L
    if sof is None:
        return None
    H, W, comps = sof
    shape = [(h, v) for _, h, v, _ in comps]
    sampling = {((1, 1),): JPEG_GREY, ((1, 1),) * 3: JPEG_444, ((2, 1), (1, 1), (1, 1)): JPEG_422,
                ((2, 2), (1, 1), (1, 1)): JPEG_420}.get(tuple(shape))
    if sampling is None or H < 1 or W < 1:
        return None
    if len(comps) == 3 and [c[0] for c in comps] != [1, 2, 3]:   # libjpeg takes other identifiers ('R', 'G', 'B', ...) for other colour spaces
        return None
    if sampling in (JPEG_422, JPEG_420) and (W + 1) // 2 <= 2:          # libjpeg replicates chroma planes this narrow
        return None
    if len(b) != 4 + 2 * len(comps) or b[0] != len(comps) or tuple(b[-3:]) != (0, 63, 0):
        return None
    if not huff:                                               # AVI Motion-JPEG convention: no DHT = the tables of Annex K
        huff = {ident: (bytes(c), bytes(sy)) for ident, (c, sy) in zip((0x00, 0x10, 0x01, 0x11), _JPEG_HUFF)}
    sel = []
    for i, (ident, _, _, tq) in enumerate(comps):
        td, ta = b[2 + 2 * i] >> 4, b[2 + 2 * i] & 15
        if b[1 + 2 * i] != ident or td > 1 or ta > 1 or td not in huff or 0x10 | ta not in huff or tq not in qt:
            return None
        sel.append((tq, td, ta))
    record = np.zeros(JPEG_DESC_BYTES, np.uint8)
    words = record[:32].view(np.int32)
    words[2] = restart
    for k in range(3):
        words[3 + k] = sum(sl[k] << (8 * c) for c, sl in enumerate(sel))
    for t, body in qt.items():
        record[32 + 64 * t: 96 + 64 * t] = np.frombuffer(body, np.uint8)
    tables = []
    for t, ident in enumerate((0x00, 0x01, 0x10, 0x11)):
        tables.append(huff.get(ident))
        if ident in huff:
            counts, symbols = huff[ident]
            record[288 + 272 * t: 304 + 272 * t] = np.frombuffer(counts, np.uint8)
            record[304 + 272 * t: 304 + 272 * t + len(symbols)] = np.frombuffer(symbols, np.uint8)
    return dict(H=H, W=W, sampling=sampling, components=[(h, v) + sl for (_, h, v, _), sl in zip(comps, sel)],
                qt={t: bytes(body) for t, body in qt.items()}, huff=tables, restart=restart, scan_off=p + 2 + L, record=record)


def jpeg_parse(data):
    """What egne_jpeg_decode needs of one JPEG file, or None for a file the device decoder does not take (anything but SOF0, 8 bit,
    one scan, grey or three components at 4:4:4 / 4:2:2 / 4:2:0, 8-bit quantisation tables; fill bytes or foreign markers inside the
    scan; subsampled chroma planes of one or two columns; three components that are not YCbCr: an Adobe segment with a transform
    other than 1, or identifiers other than 1, 2, 3).  Walks the marker segments only -- byte-level work, nothing per Huffman
    symbol.  Returns a dictionary: H, W, sampling (JPEG_GREY / JPEG_444 / JPEG_422 / JPEG_420), components [(h, v, tq, td, ta)],
    qt {table: 64 bytes in file (zigzag) order}, huff [DC 0, DC 1, AC 0, AC 1] as (16 counts, symbols) or None (a file without DHT
    gets the tables of Annex K), restart (MCUs, 0 = none), scan_off, scan_len (the entropy-coded scan: up to EOI), record."""
    hdr, info = _PARSED_HEADER
    if hdr is None or not data.startswith(hdr):                # (a video's frames mostly share their header byte for byte)
        info = _parse_header(data)
        if info is None:
            return None
        _PARSED_HEADER[:] = [bytes(data[:info['scan_off']]), info]
    off = info['scan_off']
    end = data.find(b'\xff\xd9', off)
    if end < 0 or _JPEG_FOREIGN_MARKER.search(data, off, end) or data[end - 1: end] == b'\xff':
        return None
    return dict(info, scan_len=end - off)


def decode_jpeg_device(datas, device=None, sub_bits=1024, mode=1, out=None, parsed=None):
    """Grey frames of a list of baseline JPEG files (byte strings) decoded on the device (egne_jpeg_decode): returns (grey uint8
    [N,H,W] on the device -- byte for byte np.asarray(Image.open(...).convert('L')) of every file --, flags int32 [N], non-zero where
    the scan turned out invalid: that frame's row is then unspecified).  All files share H, W and sampling (ValueError otherwise, and
    for a file jpeg_parse refuses).  ``mode`` 1: self-synchronising subsequences of ``sub_bits`` bits; 0: one lane per restart
    interval.  ``out``: the uint8 [N,H,W] device tensor to decode into; ``parsed``: the files' jpeg_parse results, if the caller has
    them.  One upload of the concatenated scans and one of the descriptor table; queues on the current stream, no synchronisation."""
    from egne_amd import _lib
    datas = list(datas)
    infos = [jpeg_parse(d) for d in datas] if parsed is None else list(parsed)
    if not datas or len(infos) != len(datas):
        raise ValueError("decode_jpeg_device needs at least one JPEG file (and one jpeg_parse result per file)")
    for n, info in enumerate(infos):
        if info is None:
            raise ValueError("file %d is not a JPEG stream the device decoder takes (jpeg_parse)" % n)
    H, W, sampling = infos[0]['H'], infos[0]['W'], infos[0]['sampling']
    for n, info in enumerate(infos):
        if (info['H'], info['W'], info['sampling']) != (H, W, sampling):
            raise ValueError("file %d is %dx%d with sampling %d, file 0 %dx%d with sampling %d: one call, one geometry"
                             % (n, info['H'], info['W'], info['sampling'], H, W, sampling))
    N = len(datas)
    desc = np.stack([info['record'] for info in infos])
    words = desc[:, :32].view(np.int32)
    parts, at = [], 0
    for n, (d, info) in enumerate(zip(datas, infos)):
        scan = d[info['scan_off']: info['scan_off'] + info['scan_len']]
        words[n, 0], words[n, 1] = at, len(scan)
        parts += [scan, b'\0' * (-len(scan) % 4)]
        at += len(scan) + (-len(scan) % 4)
    nbytes = max(at, 4)
    device = torch.device('cuda' if device is None else device)
    streams = torch.from_numpy(np.frombuffer(b''.join(parts).ljust(nbytes, b'\0'), np.uint8).copy()).to(device)
    desc = torch.from_numpy(desc).to(device)
    if out is None:
        out = torch.empty((N, H, W), dtype=torch.uint8, device=device)
    elif out.dtype != torch.uint8 or tuple(out.shape) != (N, H, W) or not out.is_contiguous() or out.device.type != 'cuda':
        raise ValueError("out must be a contiguous uint8 [%d,%d,%d] tensor on the device" % (N, H, W))
    L = _lib.lib()
    flags = torch.empty(N, dtype=torch.int32, device=device)
    ws = torch.empty(int(L.egne_jpeg_decode_workspace_bytes(N, H, W, sampling, nbytes, int(sub_bits), 1)), dtype=torch.uint8, device=device)
    _lib.check(L.egne_jpeg_decode(streams.data_ptr(), nbytes, desc.data_ptr(), N, H, W, sampling, int(sub_bits), int(mode), out.data_ptr(),
                                  None, flags.data_ptr(), None, ws.data_ptr(), _lib.stream_ptr()), "jpeg_decode")
    return out, flags


def _decode_batch(batch, device):
    """--device_decode 1: the frames of a batch into one uint8 [N,H,W] device tensor -- those jpeg_parse took by the device decoder
    (straight into the tensor when that is all of them), the others from the host's decode.  Returns (frames, flags int32 [N])."""
    first = next((x[1] for _, fr, x in batch if fr is None), None)
    shape = (first['H'], first['W']) if first is not None else batch[0][1].shape[:2]
    on_dev = [n for n, (_, fr, _) in enumerate(batch) if fr is None]
    fu = torch.empty((len(batch),) + tuple(shape), dtype=torch.uint8, device=device)
    flags = torch.zeros(len(batch), dtype=torch.int32, device=device)
    if on_dev:
        whole = len(on_dev) == len(batch)
        grey, fl = decode_jpeg_device([batch[n][2][0] for n in on_dev], device, out=fu if whole else None,
                                      parsed=[batch[n][2][1] for n in on_dev])
        if whole:
            return fu, fl
        at = torch.tensor(on_dev, device=device)
        fu[at] = grey
        flags[at] = fl
    for n, (_, fr, _) in enumerate(batch):
        if fr is not None:
            fu[n] = _upload_u8(fr, device)
    return fu, flags


def evaluate_ellseg_per_video(path_vid, args, model, edge_model, device):
    """evaluate.py:195-308: every frame of the video holds two eyes side by side (320 columns each): per eye preprocess ->
    edge -> seg -> fitted ellipses -> back to the source geometry; writes <name>_result_<method>.avi (overlay: class colours,
    both ellipses, frame number) and <name>_edge_<method>.avi (255 - 255*edge), both Motion-JPEG, and the ellipse dictionary
    <name>_pred2_<method>.npy {frame: (iris, pupil)} -- eyes are batched 32 at a time instead of one by one."""
    from egne_amd.pipeline import TwoStagePipeline, WindowedFit
    stem = os.path.splitext(path_vid)[0]
    out, pending = {}, []
    vid_out = edge_out = None
    # the edge network of batch i+1 runs next to ESF-Net + fit of batch i (two HIP streams), and the host draws / encodes batch
    # i-1 meanwhile: results come back one batch late
    pipe = TwoStagePipeline(argparse.Namespace(prec=torch.float32, edge_thres=0), edge_model, torch.device(device))
    queued = []                                  # frames of the batches whose results are still on the device
    # the ellipse searches of batch i are released where ESF-Net of batch i+1 reaches its low-resolution levels (WindowedFit): a
    # batch is drawn once the NEXT batch's second stage has been queued, i.e. two batches behind the decoder
    wfit = WindowedFit(torch.device(device))
    ready = []

    redo = [False]
    io = bool(getattr(args, 'device_io', 0))        # frame prep and rendering on the device: uint8 frames up, uint8 frames + ellipses down
    ew = int(getattr(args, 'eye_width', 320))
    live = bool(getattr(args, 'low_latency', 0))    # head-mounted-display use: a frame's ellipses before the next frame arrives
    dj = bool(getattr(args, 'device_jpeg', 0))      # frame number and JPEG encoding on the device: only the streams' bytes come down
    if dj and not io:
        sys.exit('evaluate.py: --device_jpeg 1 needs --device_io 1')
    dd = bool(getattr(args, 'device_decode', 0))    # the input's JPEG decoding on the device: compressed bytes up instead of frames
    if dd and not io:
        sys.exit('evaluate.py: --device_decode 1 needs --device_io 1')
    runner = [None]
    seed, regions = seed_of(args)                   # --ellipse_seed mask: every path below seeds the searches from the class map
    clean = clean_of(args)                          # --clean_mask 1: every path below reads the cleaned class map

    def flush():
        if not pending:
            return
        if io:
            return flush_io()
        eyes = [e for fr in pending for e in fr[2]]
        x = torch.stack([e[0] for e in eyes]).to(device)
        if live:
            # one hipGraph replay per frame pair (egne_amd.pipeline.GraphedFrames, captured on the first frame): no batching, no
            # pipelining across frames -- 4.3-4.7 ms per call on MI355X instead of a batch of 32 every ~20 ms
            if runner[0] is None or tuple(runner[0].x.shape) != tuple(x.shape):
                runner[0] = graphed_runner(x, model, edge_model, seed, regions, clean)
            res = [t.clone() for t in runner[0](x)]
            if _overflowed(model) | _overflowed(edge_model):
                # beyond the head-room of the scales baked into the captured launches: capture again (its eager warm-up runs re-calibrate)
                runner[0] = graphed_runner(x, model, edge_model, seed, regions, clean)
                res = [t.clone() for t in runner[0](x)]
                if _overflowed(model) | _overflowed(edge_model):
                    raise RuntimeError("non-finite activations after re-calibration: the input frames themselves are not finite")
            done = torch.cuda.Event()
            done.record()
            frames_now = list(pending)
            pending.clear()
            draw(frames_now, (tuple(res), done))
            return
        queued.append(list(pending))
        pending.clear()
        r = pipe.submit(x, _seg_and_fit(x, model, wfit, seed=seed, regions=regions, clean=clean))
        if r is not None:
            ready.append((queued.pop(0), r))
        while len(ready) > 1:
            draw(*ready.pop(0))

    def fix_flagged(batch):
        """--device_decode 1: the decoder's flags come down; a flagged frame is decoded by the host into its row.  True if there was one."""
        bad = np.flatnonzero(_download(batch.dflags))
        for n in bad:
            fr = _decode_host(batch[n][2][0])
            if fr is None or tuple(fr.shape) != tuple(batch.fu.shape[1:]):
                sys.exit('evaluate.py: frame %d of %s is a JPEG stream that neither the device decoder nor the host decodes; '
                         'run with --device_decode 0, which skips such frames' % (batch[n][0], path_vid))
            torch.cuda.synchronize()
            batch.fu[n] = _upload_u8(fr, device)
        if len(bad):
            batch.dflags.zero_()
        return len(bad) > 0

    def flush_io():
        batch = _Batch(pending)
        pending.clear()
        if dd:
            # eager launches on this stream, in front of prep (and of the graph replay): stream lengths vary, so nothing is captured
            batch.fu, batch.dflags = _decode_batch(batch, device)
        else:
            batch.fu = _upload_u8(np.stack([fr for _, fr, _ in batch]), device)
        if dj:
            batch.masks = torch.from_numpy(np.stack([frame_number_mask(j) for j, _, _ in batch])).to(device)
        if live:
            # prep and rendering are part of the replay: one graph from the uint8 frame to the two uint8 frames
            # (--device_decode 1: a capture calibrates on its frames, so it never sees a flagged frame's unspecified row; a replay may,
            # and what such a row does to the network is either an overflow, answered here, or nothing, answered at draw time)
            if runner[0] is None or tuple(runner[0].x.shape) != tuple(batch.fu.shape):
                if dd:
                    fix_flagged(batch)
                runner[0] = graphed_runner_io(batch.fu, model, edge_model, (240, 320), 2, ew, seed, regions, clean)
            res = runner[0](batch.fu)
            if _overflowed(model) | _overflowed(edge_model):
                if dd:
                    fix_flagged(batch)
                runner[0] = graphed_runner_io(batch.fu, model, edge_model, (240, 320), 2, ew, seed, regions, clean)
                res = runner[0](batch.fu)
                if _overflowed(model) | _overflowed(edge_model):
                    raise RuntimeError("non-finite activations after re-calibration: the input frames themselves are not finite")
            batch.rendered = tuple(res)
            if dj:
                _encode_rendered(batch)           # eager launches on the same stream, right behind the replay
            done = torch.cuda.Event()
            done.record()
            draw_io(batch, (None, done))
            return
        x, ss = preprocess_frames_device(batch.fu, (240, 320), 2, ew)

        def then(e, m, fit):                  # on the searches' stream, right behind them (WindowedFit.submit)
            batch.rendered = render_frames_device(batch.fu, e, m, fit, ss, 2, ew)
            if dj:
                _encode_rendered(batch)
        queued.append(batch)
        r = pipe.submit(x, _seg_and_fit(x, model, wfit, then, seed, regions, clean))
        if r is not None:
            ready.append((queued.pop(0), r))
        while len(ready) > 1:
            draw_io(*ready.pop(0))

    def draw_io(batch, r):
        nonlocal vid_out, edge_out
        res, done = r
        done.synchronize()
        if res is not None:
            res[2].synchronize()        # WindowedFit.Handle: queues the searches (and the rendering behind them) if their window never opened
        again = redo[0] or _overflowed(model) | _overflowed(edge_model)
        if again:
            redo[0] = not redo[0]
        if dd and fix_flagged(batch):
            # the decoder's flags come down with the results: a flagged frame is decoded by the host, and the batch is done again
            again = True
        if again:
            # as draw(): this batch and the one queued behind it again, from the retained uint8 device frames, rendered again
            torch.cuda.synchronize()
            batch.rendered = evaluate_frames_device_io(batch.fu, model, edge_model, (240, 320), 2, ew, seed, regions, clean)
            if dj:
                _encode_rendered(batch)
        if dj:
            # the lengths and flags of the batch's streams come down, then their used bytes packed into one buffer, then the ellipses
            out_o, len_o, flag_o, out_e, len_e, flag_e = batch.encoded
            meta = _download(torch.stack([len_o, flag_o, len_e, flag_e]))
            packed = _download(torch.cat([o[n, :int(meta[k, n])] for n in range(len(batch)) for k, o in ((0, out_o), (2, out_e))])).tobytes()
            ell, at = _download(batch.rendered[2]), 0
        else:
            overlay, edge_frame, ell = (_download(t) for t in batch.rendered)
        for n, (j, fr, _) in enumerate(batch):
            for i in range(2):
                q, p = ell[2 * n + i, 0].copy(), ell[2 * n + i, 1].copy()
                out[j] = (q, p)
                out[(j, i)] = (q, p)
            if not dj:
                _put_frame_number(overlay[n], j)
            if vid_out is None:
                Hh, Ww = (int(v) for v in batch.fu.shape[1:]) if dd else fr.shape[:2]      # (--device_decode 1: from the parsed header)
                vid_out = MJPEGWriter(stem + '_result_' + args.method + '.avi', 30, (Ww, Hh))
                edge_out = MJPEGWriter(stem + '_edge_' + args.method + '.avi', 30, (Ww, Hh))
            if not dj:
                vid_out.write(overlay[n])
                edge_out.write(edge_frame[n])
                continue
            for k, w, frames in ((0, vid_out, batch.rendered[0]), (2, edge_out, batch.rendered[1])):
                if meta[k + 1, n]:                     # the stream did not fit its slot: the frame itself comes down and PIL encodes it
                    frame = _download(frames[n])
                    if k == 0:
                        _put_frame_number(frame, j)
                    w.write(frame)
                else:
                    w.write_jpeg(packed[at: at + int(meta[k, n])])
                    at += int(meta[k, n])

    def drain():
        r = pipe.flush()
        if r is not None and queued:
            ready.append((queued.pop(0), r))
        while ready:
            (draw_io if io else draw)(*ready.pop(0))

    def draw(frames_of_batch, r):
        nonlocal vid_out, edge_out
        res, done = r
        done.synchronize()
        edge, seg, pup, iri = _to_host(res)
        if redo[0] or _overflowed(model) | _overflowed(edge_model):
            # invalid results (engine.Plan.overflowed): this batch again, back to back, on the re-calibrated plans -- and the batch
            # queued behind it too, whose edge maps were computed with the old scales
            redo[0] = not redo[0]
            torch.cuda.synchronize()    # the edge network of the NEXT batch is in flight on the pipeline's stream and owns the same plan buffers
            x = torch.stack([e[0] for _, _, fe in frames_of_batch for e in fe]).to(device)
            edge, seg, pup, iri = evaluate_ellseg_on_image(x, model, edge_model, args)
        k = 0
        for j, frame_bgr, fe in frames_of_batch:
            overlay, edge_frame = frame_bgr.copy(), frame_bgr.copy()
            for i, (_, ss, grey) in enumerate(fe):
                em = 255.0 - 255.0 * edge[k]                                         # evaluate.py:263-264
                sm, p, q, em = rescale_to_original(seg[k], pup[k], iri[k], ss, grey.shape, edge_map=em)
                out[j] = (q, p)                                                      # evaluate.py:269 (the second eye overwrites the first)
                out[(j, i)] = (q, p)
                overlay[:, ew * i: ew * (i + 1)] = plot_segmap_ellpreds(grey, sm, p, q)
                edge_frame[:, ew * i: ew * (i + 1)] = np.clip(em, 0, 255).astype(np.uint8)[..., None]
                k += 1
            _put_frame_number(overlay, j)
            if vid_out is None:
                Hh, Ww = frame_bgr.shape[:2]
                vid_out = MJPEGWriter(stem + '_result_' + args.method + '.avi', 30, (Ww, Hh))
                edge_out = MJPEGWriter(stem + '_edge_' + args.method + '.avi', 30, (Ww, Hh))
            vid_out.write(overlay)
            edge_out.write(edge_frame)

    def frames_or_chunks():
        """--device_decode 1: (None, (file, jpeg_parse's result)) for a frame the device decodes, (host-decoded frame, (file, None)) for
        one it does not take (or whose geometry is not the video's first device frame's); a file PIL cannot decode either is skipped,
        as mjpeg_frames skips it, so both paths number the frames alike."""
        if not dd:
            yield from mjpeg_frames(path_vid)
            return
        key = None
        for chunk in mjpeg_chunks(path_vid):
            info = jpeg_parse(chunk)
            if info is not None:
                key = key or (info['H'], info['W'], info['sampling'])
                if (info['H'], info['W'], info['sampling']) == key:
                    yield None, (chunk, info)
                    continue
            fr = _decode_host(chunk)
            if fr is not None:
                yield fr, (chunk, None)

    for j, fr in enumerate(frames_or_chunks()):
        if args.max_frames and j >= args.max_frames:
            break
        if io:
            if not args.align_width:
                sys.exit('Height alignment not implemented! Exiting ...')
            # the decoded frame as it is (--device_decode 1: the compressed one): prep and rendering run on the device
            pending.append((j,) + fr if dd else (j, fr, None))
        else:
            frame_bgr = np.stack([fr] * 3, axis=2)
            eyes = []
            for i in range(2):
                grey = fr[:, ew * i: ew * (i + 1)]
                t, ss = preprocess_frame(grey, (240, 320), args.align_width)
                eyes.append((t, ss, grey))
            pending.append((j, frame_bgr, eyes))
        if len(pending) >= (1 if live else 16):
            flush()
    flush()
    drain()
    assert not queued
    for w in (vid_out, edge_out):
        if w is not None:
            w.release()
    np.save(stem + '_pred2_' + args.method + '.npy', out, allow_pickle=True)
    return out


def _put_frame_number(img, j):
    """cv2.putText(frame, str(j), (10, 30), FONT_HERSHEY_PLAIN, 2.0, (0, 0, 255), 2) -- PIL's default font instead of Hershey."""
    from PIL import Image, ImageDraw
    im = Image.fromarray(np.ascontiguousarray(img[..., ::-1]))
    ImageDraw.Draw(im).text((10, 12), str(j), fill=(255, 0, 0))
    img[...] = np.asarray(im)[..., ::-1]


def main(argv=None):
    args = parse_args(argv)
    device = torch.device('cuda')
    setting = _entry.load_setting(args.setting)
    if args.model not in ('ritnet_v2', 'deepvog'):
        sys.exit('evaluate.py: illegal model %r (evaluate.py:362-367 knows ritnet_v2 and deepvog)' % args.model)
    if args.synthetic:
        edge_net, model = _entry.seeded_networks(setting)
        if args.model == 'deepvog':
            from egne_amd import synth
            from egne_amd.modelSummary import get_model
            model = get_model('deepvog', None)
            model.load_state_dict(synth.seeded_state_dict(model.state_dict(), seed=1, kind='esf'))
    else:
        for need in (args.loadfile, 'gen_00000016.pt'):        # the reference dies in torch.load (evaluate.py:360-371)
            if not os.path.exists(need):
                sys.exit('evaluate.py: weights file %r not found (use --synthetic N for seeded random weights)' % need)
        from egne_amd.bdcn_new import BDCN
        from egne_amd.modelSummary import get_model
        edge_net = BDCN()
        edge_net.load_state_dict(torch.load('gen_00000016.pt', map_location='cpu')['a'])
        model = get_model(args.model, setting)
        model.load_state_dict(torch.load(args.loadfile, map_location='cpu')['state_dict'], strict=True)
    edge_net, model = edge_net.to(device).eval(), model.to(device).eval()
    if args.synthetic:
        from egne_amd import synth
        x = synth.make_batch(args.synthetic, seed=5)['img'].to(device)
        edge, seg, pup, iri = evaluate_ellseg_on_image(x, model, edge_net, args)
        print('pupil ellipses:\n', pup, '\niris ellipses:\n', iri)
        return pup, iri
    res = None
    for v in sorted(glob.glob(os.path.join(args.path2data, '*.' + args.vid_ext))):
        print('evaluate {}...'.format(os.path.basename(v)))
        res = evaluate_ellseg_per_video(v, args, model, edge_net, device)
    return res


if __name__ == '__main__':
    main()
