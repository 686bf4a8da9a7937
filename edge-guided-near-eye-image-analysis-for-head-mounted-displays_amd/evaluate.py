#!/usr/bin/env python3
"""Video / frame inference entry point -- the reference's evaluate.py (edge -> seg -> ellipse fit).

The per-image path (evaluate.py:105-166) runs on the HIP kernels; the two ellipses of a frame are fitted
by one device launch.  OpenCV is not available in this image: MJPEG .avi files (the format of
videos/example1.avi) are decoded with PIL (or on the device), and per video the script writes <name>_result_<method>.avi (the
overlay: class colours, both ellipses, frame number), <name>_edge_<method>.avi (the edge maps), both Motion-JPEG, and
<name>_pred2_<method>.npy (the ellipse dictionary {frame: (iris, pupil), (frame, eye): (iris, pupil)}).

This file holds the arguments, the seed / clean-up policy tables, the stages and the video loop; the resize restatement and the host
and device front and back ends live in frame_io.py, the JPEG / AVI code in mjpeg.py.  Their names are imported back below: the loop
looks them up here, in this module's globals, at call time.

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
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import egne_amd  # noqa: E402,F401
from egne_amd import _entry  # noqa: E402

import numpy as np  # noqa: E402
import torch  # noqa: E402

from egne_amd.utils import fit_ellipses_from_mask, fit_ellipses_from_pred  # noqa: E402
from egne_amd.frame_io import (  # noqa: E402,F401
    _check_frames, _draw_ellipse, device_table, lanczos4_table, nearest_table, outline_table, plot_segmap_ellpreds, prep_geometry,
    preprocess_frame, preprocess_frames_device, render_frames_device, rescale_to_original, resize_lanczos4, resize_nearest)
from egne_amd.mjpeg import (  # noqa: E402,F401
    JPEG_420, JPEG_422, JPEG_444, JPEG_DESC_BYTES, JPEG_GREY, JPEG_RESTART_MCUS, MJPEGWriter, _JPEG_CHROMA_Q, _JPEG_HUFF, _JPEG_LUMA_Q,
    _JPEG_ZIGZAG, _STAMP_PATCH, _decode_host, _parse_header, _put_frame_number, _stamp_masks_device, decode_jpeg_device,
    encode_jpeg_device, frame_number_mask, jpeg_header, jpeg_parse, jpeg_tables, mjpeg_chunks, mjpeg_frames, stamp_numbers_device)

_device_table, _outline_table = device_table, outline_table      # the names they had while they lived here
BATCH_FRAMES = 16          # video frames per batch of the batched loop (read when evaluate_ellseg_per_video is called)


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
        if len(pending) >= (1 if live else BATCH_FRAMES):
            flush()
    flush()
    drain()
    assert not queued
    for w in (vid_out, edge_out):
        if w is not None:
            w.release()
    np.save(stem + '_pred2_' + args.method + '.npy', out, allow_pickle=True)
    return out


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
