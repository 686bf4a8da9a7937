"""Measurement of evaluate.py --device_jpeg: per frame pair wall time of the whole --low_latency 1 loop INCLUDING
the two JPEG encodes and the AVI writers' write / write_jpeg, with --device_io 1 (host PIL encoding, the parent behaviour) and
--device_io 1 --device_jpeg 1, interleaved in one process; the encoder alone by device events; PIL's encoder on this host.  Writes
profiles/eval_device_jpeg.txt."""
import os
import sys
import tempfile
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


say("evaluate.py --device_jpeg: wall time per frame pair in ms (median, mean, 90th percentile) over %d frames after %d warm-up frames" % (STEPS, WARM))
say("MI355X, one process, --device_io 1 (PIL encodes on the host: the parent commit) and --device_io 1 --device_jpeg 1 interleaved, two rounds each")
say("restart interval %d MCUs, quality 90" % E.JPEG_RESTART_MCUS)
real_write, real_jpeg = E.MJPEGWriter.write, E.MJPEGWriter.write_jpeg
for big in (False, True):
    frames = clip(big)
    Hs, Ws = frames[0].shape
    ew = Ws // 2
    say("")
    say("clip %d x %d (eye %d x %d -> 240 x 320%s)" % (Ws, Hs, ew, Hs, ", Lanczos resize" if big else ", no resize"))
    # ---- (a) the whole --low_latency 1 loop, JPEG encoding and the writers included --------------------------------------------------
    stamps, sizes = [], []
    E.mjpeg_frames = lambda path, _f=frames: iter(_f)

    def write(self, frame):
        real_write(self, frame)
        sizes.append(len(self.frames.pop()))           # (the stream is dropped: 220 frames per run need not be kept)
        if "_edge_" in self.path:
            stamps.append(time.perf_counter())

    def write_jpeg(self, data):
        real_jpeg(self, data)
        sizes.append(len(self.frames.pop()))
        if "_edge_" in self.path:
            stamps.append(time.perf_counter())
    E.MJPEGWriter.write, E.MJPEGWriter.write_jpeg = write, write_jpeg
    E.MJPEGWriter.release = lambda self: None
    tmpdir = tempfile.mkdtemp()
    for rnd in range(2):
        for dj in (0, 1):
            del stamps[:], sizes[:]
            args = E.parse_args(["--low_latency", "1", "--device_io", "1", "--device_jpeg", str(dj), "--eye_width", str(ew), "--method", "m%d" % dj])
            t0 = time.perf_counter()
            E.evaluate_ellseg_per_video(os.path.join(tmpdir, "clip.avi"), args, net, bd, dev)
            ts = np.diff(np.asarray([t0] + stamps))
            say("(a) --low_latency 1 loop with encoding, device_jpeg %d round %d: %s   (mean stream %.1f KB)"
                % (dj, rnd, stats(list(ts)), np.mean(sizes[2 * WARM:]) / 1e3))
    E.MJPEGWriter.write, E.MJPEGWriter.write_jpeg = real_write, real_jpeg
    # ---- (b) PIL's encoder on this host, the two frames of a pair (a rendered-like BGR frame and a grey one) ----------------------------
    bgr = np.stack([frames[0]] * 3, axis=2)
    bgr[60:120, 100:200] = (120, 183, 53)
    w = E.MJPEGWriter(os.path.join(tmpdir, "x.avi"), 30, (Ws, Hs))
    ts = []
    for _ in range(WARM + STEPS):
        t0 = time.perf_counter()
        w.write(bgr)
        ts.append(time.perf_counter() - t0)
        del w.frames[:]
    say("(b) MJPEGWriter.write (PIL, quality 90) of one frame on this host: %s" % stats(ts))
    # ---- (c) the Python surface: device events around back-to-back eager calls (an upper bound of the device time at 2 frames: each call
    # also allocates four tensors on the host side) ------------------------------------------------------------------------------------
    for n, calls in ((2, 4000), (32, 1000)):
        stack = torch.from_numpy(np.stack([np.stack([frames[k]] * 3, axis=2) for k in range(n)])).to(dev)
        for _ in range(WARM):
            out, lengths, flags = E.encode_jpeg_device(stack)
        for rnd in range(2):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            a.record()
            for _ in range(calls):
                out, lengths, flags = E.encode_jpeg_device(stack)
            b.record()
            torch.cuda.synchronize()
            assert not flags.any().item()
            say("(c) encode_jpeg_device, %2d frames, %d eager calls back to back (device events) round %d: %.1f us per call, %.1f us per frame, %.1f KB per frame"
                % (n, calls, rnd, a.elapsed_time(b) * 1e3 / calls, a.elapsed_time(b) * 1e3 / calls / n, lengths.float().mean().item() / 1e3))
        # the same four launches on preallocated buffers, nothing but the C call per iteration: what is left of (c) without the Python wrapper
        # (header, table look-ups, four allocations per call)
        from egne_amd import _lib
        L = _lib.lib()
        header = E.jpeg_header(Ws, Hs, 90)
        qt, huff, dct = E._device_table(("jpeg", 90), dev, lambda: E.jpeg_tables(90))
        hd, = E._device_table(("jpeg_header", Ws, Hs, 90), dev, lambda: (np.frombuffer(header, np.uint8).copy(),))
        cap = int(out.shape[1])
        ws = torch.empty(int(L.egne_jpeg_workspace_bytes(n, Hs, Ws)), dtype=torch.uint8, device=dev)
        argv = (stack.data_ptr(), n, Hs, Ws, qt.data_ptr(), huff.data_ptr(), dct.data_ptr(), hd.data_ptr(), len(header), E.JPEG_RESTART_MCUS,
                out.data_ptr(), cap, lengths.data_ptr(), flags.data_ptr(), ws.data_ptr(), _lib.stream_ptr())
        for rnd in range(2):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            a.record()
            for _ in range(calls):
                L.egne_jpeg_encode(*argv)
            b.record()
            torch.cuda.synchronize()
            assert not flags.any().item()
            say("(d) egne_jpeg_encode alone, %2d frames, %d calls on preallocated buffers (device events) round %d: %.1f us per call, %.1f us per frame"
                % (n, calls, rnd, a.elapsed_time(b) * 1e3 / calls, a.elapsed_time(b) * 1e3 / calls / n))
os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
with open(os.path.join(ROOT, "profiles", "eval_device_jpeg.txt"), "w") as f:
    f.write("\n".join(lines) + "\n")
