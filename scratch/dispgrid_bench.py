"""Measurement of the prediction overlay grid (egne_amd.dispgrid, csrc/dispgrid.hip).  Writes profiles/dispgrid.txt (or the path given
as the first argument).

(a) the call alone (image_grid with the uint8 image: five launches) at 240 x 320 for 4 frames and for count = 64,
    device events around back-to-back calls; beside it save_grid (JPEG encoding and the copy down) by a host clock, and the NumPy
    restatement of tests/dispgrid_refs.py on one host core of the same box.
(b) test.py's loop (calc_acc) over 512 synthetic frames in batches of 64 with --disp 0 and --disp 1: one process, the same loader and
    networks, taking turns, three times each after a warm round; frames / s from a host clock around the call.
(c) train.py, 512 synthetic frames in batches of 64: seconds from one epoch's validation pass to the next one's with --disp 0 and
    --disp 1, taking turns, the first interval of every run left out.  --disp 0 runs the code the parent commit runs: the flag adds
    nothing to it.
The weights are seeded random numbers: the pictures mean nothing, only their agreement with the restatement does (tests).
"""
import contextlib
import io
import os
import sys
import tempfile
import time
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch

import egne_amd  # noqa: F401
from egne_amd import _entry, dispgrid

OUT = os.path.abspath(sys.argv[1]) if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "dispgrid.txt")
PARTS = sys.argv[2] if len(sys.argv) > 2 else "abc"
dev = torch.device("cuda:0")
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


def spread(v):
    return "%.1f (%.1f .. %.1f)" % (float(np.median(v)), min(v), max(v))


def timed(fn, reps):
    us = []
    for r in range(6):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        a.record()
        for _ in range(reps):
            fn()
        b.record()
        host = (time.perf_counter() - t0) * 1e6 / reps
        torch.cuda.synchronize()
        if r:
            us.append(a.elapsed_time(b) * 1e3 / reps)
    return us, host


def part_a():
    import dispgrid_refs as R
    H, W = 240, 320
    say("(a) 240 x 320, seeded frames, maps and ellipses (tests/dispgrid_refs.inputs, 4 frames repeated); us per call on the device, "
        "median (min .. max) of 5 rounds of 20 calls after a warm one; host = time to queue one call")
    base = R.inputs(4, H, W, 31)
    for n in (4, 64):
        d = {k: torch.from_numpy(np.concatenate([v] * (n // 4))).to(dev) for k, v in base.items()}

        def call():
            return dispgrid.image_grid(d["img"], d["mask"], d["el"], None, d["cond"], d["el_gt"], override=True, count=n, nrow=8 if n > 4 else 4,
                                       return_u8=True)
        us, host = timed(call, 20)
        g, u8 = call()
        say("    %2d frames, grid %4d x %4d: image_grid (float grid + uint8 image)   %s us   (host %.0f us)" % (n, g.shape[1], g.shape[2], spread(us), host))
        with tempfile.TemporaryDirectory() as tmp:
            ts = []
            for r in range(6):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                dispgrid.save_grid(os.path.join(tmp, "g.jpg"), u8)
                ts.append((time.perf_counter() - t0) * 1e6)
            say("               save_grid (device JPEG, copy down, file), host clock           %s us, %d bytes"
                % (spread(ts[1:]), os.path.getsize(os.path.join(tmp, "g.jpg"))))
    ts = []
    for r in range(4):
        t0 = time.perf_counter()
        R.image_grid(base["img"], base["mask"], base["el"], base["cond"], base["el_gt"], override=True)
        ts.append((time.perf_counter() - t0) * 1e3)
    say("     4 frames: the NumPy restatement on one host core                      %s ms" % spread(ts[1:]))


def part_b():
    from torch.utils.data import DataLoader
    from egne_amd import test as T
    setting = _entry.load_setting(os.path.join(os.path.dirname(T.__file__), "configs", "baseline_edge.yaml"))
    N, B = 512, 64
    data = _entry.SyntheticEyes(N)
    edge_net, model = _entry.seeded_networks(setting, "ritnet_v2")
    edge_net, model = edge_net.to(dev).eval(), model.to(dev)
    loader = DataLoader(data, batch_size=B, shuffle=False, num_workers=0, drop_last=True)
    say("(b) test.py's loop, --synthetic %d --batchsize %d, baseline_edge, seeded weights; host clock around calc_acc; runs take turns" % (N, B))
    res, out = {0: [], 1: []}, {}
    for r in range(4):
        for disp in (0, 1):
            args = types.SimpleNamespace(prec=torch.float32, edge_thres=0, test_normal=0, device_loader=0, device_metrics=0, record_iou=0,
                                         ellipse_metrics=0, ellipse_search=0, model="ritnet_v2", batchsize=B, curObj=None, method="baseline",
                                         disp=disp)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            with contextlib.redirect_stdout(io.StringIO()):
                out[disp] = T.calc_acc(args, loader, model, edge_net, dev)
            torch.cuda.synchronize()
            if r:
                res[disp].append(N / (time.perf_counter() - t0))
    for disp in (0, 1):
        say("    --disp %d: %s frames/s   (three runs after a warm one: %s)" % (disp, spread(res[disp]), ", ".join("%.1f" % v for v in res[disp])))
    ms = lambda d: 1e3 * B / float(np.median(res[d]))      # noqa: E731
    widest = max(1e3 * B / min(v) - 1e3 * B / max(v) for v in res.values())
    say("    per batch of %d, from the medians: %.2f ms without, %+.2f ms with the grid and its file; runs of ONE setting spread over up to "
        "%.2f ms, so a difference below that is not resolved by this loop (see (a))" % (B, ms(0), ms(1) - ms(0), widest))
    same = all(np.array_equal(np.float64(a), np.float64(b), equal_nan=True) for a, b in zip(out[0], out[1]))
    say("    return values of the two settings equal bit for bit: %s; files written: %d" % (same, len(os.listdir(os.path.join("img", "synthetic_baseline_disp")))))


def part_c():
    from egne_amd import train as TR
    N, B, E = 512, 64, 4
    say("(c) train.py --synthetic %d --batchsize %d --epochs %d, baseline_edge: seconds from one epoch's validation pass to the next one's "
        "(validation, checkpoint, %d training steps, the grid and its file), host clock, the first interval of every run left out; runs "
        "take turns" % (N, B, E, N // B))
    res = {0: [], 1: []}
    orig = TR.lossandaccuracy
    for r in range(2):
        for disp in (0, 1):
            stamps = []

            def spy(*a, **k):
                torch.cuda.synchronize()
                stamps.append(time.perf_counter())
                return orig(*a, **k)
            TR.lossandaccuracy = spy
            with contextlib.redirect_stdout(io.StringIO()):
                TR.main(["--synthetic", str(N), "--batchsize", str(B), "--epochs", str(E), "--setting", "configs/baseline_edge.yaml",
                         "--expname", "bench%d%d" % (disp, r), "--disp", str(disp)])
            TR.lossandaccuracy = orig
            res[disp] += list(np.diff(stamps))[1:]
    for disp in (0, 1):
        say("    --disp %d: %s s per epoch   (%s)" % (disp, "%.2f (%.2f .. %.2f)" % (float(np.median(res[disp])), min(res[disp]), max(res[disp])),
                                                    ", ".join("%.2f" % v for v in res[disp])))
    say("    the draw adds one image_grid and one save_grid per epoch (part (a)); epochs of ONE setting spread over %.2f s"
        % max(max(v) - min(v) for v in res.values()))


say("Prediction overlay grid (csrc/dispgrid.hip, egne_amd.dispgrid) on MI355X, one process.")
work = tempfile.mkdtemp()
os.chdir(work)
if "a" in PARTS:
    part_a()
if "b" in PARTS:
    part_b()
if "c" in PARTS:
    part_c()
os.makedirs(os.path.dirname(OUT), exist_ok=True)
with open(OUT, "w") as f:
    f.write("\n".join(lines) + "\n")
