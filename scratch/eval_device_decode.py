"""Measurement of evaluate.py --device_decode, against --device_io 1 --device_jpeg 1 (PIL decodes on the host: the
parent behaviour), interleaved in one process, two rounds each: frames per second of the batched loop, wall time per frame pair of the
--low_latency 1 loop, the decode launches alone by device events (one frame, 16 frames, mode 0 against mode 1) next to PIL's decoder on
this host.  Clips of 640 x 240 and 1280 x 480, written as Motion-JPEG by MJPEGWriter (PIL, quality 90), and the five frames of the
example video's format in tests/golden/mjpeg_example_frames.npz.  Writes profiles/eval_device_decode.txt."""
import io
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch
from PIL import Image

import egne_amd  # noqa: F401
from egne_amd import _lib, evaluate as E
from common import bdcn_module, esf_module, gold

WARM, STEPS, BATCHED = 20, 200, 480
dev = torch.device("cuda:0")
bd, net = bdcn_module().to(dev), esf_module("baseline_edge").to(dev).eval()
eyes = gold("evaluate_real_frames")["eyes"]
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


def clip(big, n):
    fr = []
    for k in range(n):
        a, b = eyes[(2 * (k % 2))], eyes[2 * (k % 2) + 1]
        f = np.concatenate([np.roll(a, k % 17 - 8, 1), np.roll(b, 8 - k % 17, 1)], axis=1)
        fr.append(np.kron(f, np.ones((2, 2), np.uint8)) if big else f)
    return fr


def stats(ts):
    t = np.asarray(ts[WARM:]) * 1e3
    return "%8.3f %8.3f %8.3f" % (np.median(t), t.mean(), np.percentile(t, 90))


def events(fn, calls):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / calls


def pil_ms(files):
    ts = []
    for k in range(WARM + STEPS):
        t0 = time.perf_counter()
        np.asarray(Image.open(io.BytesIO(files[k % len(files)])).convert("L"))
        ts.append(time.perf_counter() - t0)
    return stats(ts)


def c_call(files, sub_bits, mode):
    """egne_jpeg_decode on preallocated buffers: nothing but the C call per iteration."""
    L = _lib.lib()
    infos = [E.jpeg_parse(f) for f in files]
    N, H, W, sampling = len(files), infos[0]["H"], infos[0]["W"], infos[0]["sampling"]
    desc = np.stack([i["record"] for i in infos])
    parts, at = [], 0
    for n, (f, i) in enumerate(zip(files, infos)):
        scan = f[i["scan_off"]: i["scan_off"] + i["scan_len"]]
        desc[n, :8].view(np.int32)[:] = (at, len(scan))
        parts.append(scan + b"\0" * (-len(scan) % 4))
        at += len(parts[-1])
    streams = torch.from_numpy(np.frombuffer(b"".join(parts), np.uint8).copy()).to(dev)
    d = torch.from_numpy(desc).to(dev)
    out = torch.empty((N, H, W), dtype=torch.uint8, device=dev)
    flags = torch.empty(N, dtype=torch.int32, device=dev)
    st = torch.zeros((N, 2), dtype=torch.int32, device=dev)
    ws = torch.empty(int(L.egne_jpeg_decode_workspace_bytes(N, H, W, sampling, at, sub_bits, 1)), dtype=torch.uint8, device=dev)
    argv = (streams.data_ptr(), at, d.data_ptr(), N, H, W, sampling, sub_bits, mode, out.data_ptr(), None, flags.data_ptr(), st.data_ptr(), ws.data_ptr(),
            _lib.stream_ptr())

    def call():
        assert L.egne_jpeg_decode(*argv) == 0
    call()
    torch.cuda.synchronize()
    assert not flags.any().item()
    return call, (streams, d, out, flags, ws), st.cpu().numpy()


say("evaluate.py --device_decode on MI355X, one process; --device_io 1 --device_jpeg 1 (PIL decodes on the host: the parent commit) and the")
say("same with --device_decode 1 interleaved, two rounds each; times in ms as (median, mean, 90th percentile) after %d warm-up frames" % WARM)
real_release = E.MJPEGWriter.release
tmpdir = tempfile.mkdtemp()
for big in (False, True):
    Hs, Ws = (480, 1280) if big else (240, 640)
    ew = Ws // 2
    frames = clip(big, BATCHED)
    vid = os.path.join(tmpdir, "clip%d.avi" % big)
    w = E.MJPEGWriter(vid, 30, (Ws, Hs))
    for f in frames:
        w.write(np.stack([f] * 3, axis=2))
    w.release()
    files = list(E.mjpeg_chunks(vid))
    say("")
    say("clip %d x %d, %d frames, mean %.1f KB per frame (eye %d x %d -> 240 x 320%s)"
        % (Ws, Hs, len(files), np.mean([len(f) for f in files]) / 1e3, ew, Hs, ", Lanczos resize" if big else ", no resize"))
    E.MJPEGWriter.release = lambda self: None              # (the output videos are not kept)
    # ---- (a) the batched loop: frames per second of the whole call, decoding, encoding and the writers included ---------------------------
    for rnd in range(2):
        for dd in (0, 1):
            args = E.parse_args(["--device_io", "1", "--device_jpeg", "1", "--device_decode", str(dd), "--eye_width", str(ew), "--method", "b%d" % dd])
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            E.evaluate_ellseg_per_video(vid, args, net, bd, dev)
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            say("(a) batched loop, device_decode %d round %d: %7.1f frames/s (%d frames in %.3f s)" % (dd, rnd, len(files) / dt, len(files), dt))
    # ---- (b) the --low_latency 1 loop: wall time per frame pair, from one written edge frame to the next --------------------------------
    stamps = []
    real_write, real_jpeg = E.MJPEGWriter.write, E.MJPEGWriter.write_jpeg

    def write(self, frame):
        real_write(self, frame)
        del self.frames[:]
        if "_edge_" in self.path:
            stamps.append(time.perf_counter())

    def write_jpeg(self, data):
        if "_edge_" in self.path:
            stamps.append(time.perf_counter())
    E.MJPEGWriter.write, E.MJPEGWriter.write_jpeg = write, write_jpeg
    for rnd in range(2):
        for dd in (0, 1):
            del stamps[:]
            args = E.parse_args(["--low_latency", "1", "--device_io", "1", "--device_jpeg", "1", "--device_decode", str(dd), "--eye_width", str(ew),
                                 "--method", "l%d" % dd, "--max_frames", str(WARM + STEPS)])
            t0 = time.perf_counter()
            E.evaluate_ellseg_per_video(vid, args, net, bd, dev)
            say("(b) --low_latency 1 loop, device_decode %d round %d: %s ms per frame pair" % (dd, rnd, stats(list(np.diff(np.asarray([t0] + stamps))))))
    E.MJPEGWriter.write, E.MJPEGWriter.write_jpeg, E.MJPEGWriter.release = real_write, real_jpeg, real_release
    # ---- (c) the decode alone ------------------------------------------------------------------------------------------------------------
    sets = [("this clip", files)]
    if not big:
        with np.load(os.path.join(ROOT, "tests", "golden", "mjpeg_example_frames.npz")) as g:
            sets.append(("example video format (Lavc tables)", [g[k].tobytes() for k in g.files]))
    for what, fs in sets:
        say("(c) %s, %.1f KB per frame: PIL decode + convert('L') on this host: %s ms per frame" % (what, np.mean([len(f) for f in fs]) / 1e3, pil_ms(fs)))
        for rnd in range(2):
            for n, calls in ((1, 200), (16, 50)):
                batch = [fs[k % len(fs)] for k in range(n)]
                us = events(lambda: E.decode_jpeg_device(batch, dev), calls)
                say("(c) %s: decode_jpeg_device (parse, two uploads, launches), %2d frames, %d eager calls back to back (device events) round %d: "
                    "%.1f us per call, %.1f us per frame" % (what, n, calls, rnd, us, us / n))
            for n, mode, sub_bits in ((1, 0, 1024), (1, 1, 1024), (1, 1, 512), (1, 1, 2048), (16, 0, 1024), (16, 1, 1024)):
                call, keep, st = c_call([fs[k % len(fs)] for k in range(n)], sub_bits, mode)
                us = events(call, 200 if n == 1 else 50)
                say("(d) %s: egne_jpeg_decode alone on preallocated buffers, %2d frames, mode %d, sub_bits %4d (device events) round %d: "
                    "%.1f us per call, %.1f us per frame; at most %d rounds, %d ranges in a frame" % (what, n, mode, sub_bits, rnd, us, us / n, st[:, 0].max(), st[:, 1].max()))
os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
with open(os.path.join(ROOT, "profiles", "eval_device_decode.txt"), "w") as f:
    f.write("\n".join(lines) + "\n")
