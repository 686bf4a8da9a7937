"""Measurement of evaluate.py --device_io: per frame wall time of (a) front end, (b) back end, (c) the whole
--low_latency 1 loop without JPEG encode, with --device_io 0 and 1, interleaved in one process.  Writes profiles/eval_device_io.txt."""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch

import egne_amd  # noqa: F401
from egne_amd import evaluate as E
from common import bdcn_module, esf_module, gold

WARM, STEPS = 20, 200
dev = torch.device("cuda:0")
bd, net = bdcn_module().to(dev), esf_module("baseline_edge").to(dev).eval()
eyes = gold("evaluate_real_frames")["eyes"]


def clip(big):
    fr = []
    for k in range(WARM + STEPS):
        a, b = eyes[(2 * (k % 2))], eyes[2 * (k % 2) + 1]
        f = np.concatenate([np.roll(a, k % 17 - 8, 1), np.roll(b, 8 - k % 17, 1)], axis=1)
        fr.append(np.kron(f, np.ones((2, 2), np.uint8)) if big else f)
    return fr


def stats(ts):
    t = np.asarray(ts[WARM:]) * 1e3
    return "%8.3f %8.3f %8.3f" % (np.median(t), t.mean(), np.percentile(t, 90))


lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


say("evaluate.py --device_io: wall time per frame pair in ms (median, mean, 90th percentile) over %d frames after %d warm-up frames" % (STEPS, WARM))
say("MI355X, one process, --device_io 0 and 1 interleaved (two rounds each); host = the parent commit's NumPy path")
for big in (False, True):
    frames = clip(big)
    Hs, Ws = frames[0].shape
    ew = Ws // 2
    say("")
    say("clip %d x %d (eye %d x %d -> 240 x 320%s)" % (Ws, Hs, ew, Hs, ", Lanczos resize" if big else ", no resize"))
    # ---- (a) front end: decoded uint8 frame -> network input on the device --------------------------------------------------
    for rnd in range(2):
        for io in (0, 1):
            ts = []
            for fr in frames:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                if io:
                    x, ss = E.preprocess_frames_device(E._upload_u8(fr[None], dev), (240, 320), 2, ew)
                else:
                    x = torch.stack([E.preprocess_frame(fr[:, ew * i: ew * (i + 1)], (240, 320))[0] for i in range(2)]).to(dev)
                torch.cuda.synchronize()
                ts.append(time.perf_counter() - t0)
            say("(a) front end           device_io %d round %d: %s" % (io, rnd, stats(ts)))
    # ---- (b) back end: fit result on the device -> two uint8 host frames ----------------------------------------------------
    fu = E._upload_u8(np.stack(frames[:1]), dev)
    x, ss = E.preprocess_frames_device(fu, (240, 320), 2, ew)
    from egne_amd.utils import calc_edge
    import argparse
    ns = argparse.Namespace(prec=torch.float32, edge_thres=0)
    res = E._seg_and_fit(x, net)(calc_edge(ns, x, bd, dev))
    res = tuple(t.clone() for t in res)
    torch.cuda.synchronize()
    fr = frames[0]
    for rnd in range(2):
        for io in (0, 1):
            ts = []
            for _ in range(WARM + STEPS):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                if io:
                    ov, ef, ell = (E._download(t) for t in E.render_frames_device(fu, res[0], res[1], res[2], ss, 2, ew))
                else:
                    edge, seg, pup, iri = E._to_host(res)
                    bgr = np.stack([fr] * 3, axis=2)
                    ov, ef = bgr.copy(), bgr.copy()
                    for i in range(2):
                        grey = fr[:, ew * i: ew * (i + 1)]
                        em = 255.0 - 255.0 * edge[i]
                        sm, p, q, em = E.rescale_to_original(seg[i], pup[i], iri[i], ss, grey.shape, edge_map=em)
                        ov[:, ew * i: ew * (i + 1)] = E.plot_segmap_ellpreds(grey, sm, p, q)
                        ef[:, ew * i: ew * (i + 1)] = np.clip(em, 0, 255).astype(np.uint8)[..., None]
                ts.append(time.perf_counter() - t0)
            say("(b) back end            device_io %d round %d: %s" % (io, rnd, stats(ts)))
    # GPU time of the two stages alone (device events around 200 back-to-back calls)
    for name, fn in (("prep", lambda: E.preprocess_frames_device(fu, (240, 320), 2, ew)),
                     ("render", lambda: E.render_frames_device(fu, res[0], res[1], res[2], ss, 2, ew))):
        for _ in range(WARM):
            fn()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        for _ in range(STEPS):
            fn()
        b.record()
        torch.cuda.synchronize()
        say("    %-6s on the device, %d eager calls back to back (device events, launch-bound): %.1f us per call" % (name, STEPS, a.elapsed_time(b) * 1e3 / STEPS))
    # ---- (c) the whole --low_latency 1 loop, no JPEG encode -----------------------------------------------------------------
    stamps = []
    E.mjpeg_frames = lambda path, _f=frames: iter(_f)

    def write(self, frame):
        if "_edge_" in self.path:
            stamps.append(time.perf_counter())
    E.MJPEGWriter.write = write
    E.MJPEGWriter.release = lambda self: None
    import tempfile
    tmpdir = tempfile.mkdtemp()
    for rnd in range(2):
        for io in (0, 1):
            del stamps[:]
            args = E.parse_args(["--low_latency", "1", "--device_io", str(io), "--eye_width", str(ew), "--method", "m%d" % io])
            t0 = time.perf_counter()
            E.evaluate_ellseg_per_video(os.path.join(tmpdir, "clip.avi"), args, net, bd, dev)
            ts = np.diff(np.asarray([t0] + stamps))
            say("(c) --low_latency 1 loop device_io %d round %d: %s" % (io, rnd, stats(list(ts))))
os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
with open(os.path.join(ROOT, "profiles", "eval_device_io.txt"), "w") as f:
    f.write("\n".join(lines) + "\n")
