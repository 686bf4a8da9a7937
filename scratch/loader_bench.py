"""Measurement of the device-side training loader (egne_amd.loader.device_batch): device-event time and host
wall time of a whole call at B = 64 and B = 256 for 240 x 320 batches, augmentation on / off, without scaling (raw frames of 240 x 320
and smaller) and with it (raw 480 x 640, scale 0.5); the per-stage split of the same work; next to it the README's training rate and
the one-core time of the host restatement of the item path (tests/loader_refs.py) on four frames.  Writes profiles/loader.txt (or
the path given as the first argument)."""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch

import egne_amd  # noqa: F401
from egne_amd import data_augment as DA, dataprep, loader
import loader_refs as R

OUT = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "loader.txt")
TRAIN_RATE = 1790.0          # README.md: bf16-storage training at 256 per GPU, 1781-1800 frames/s
dev = torch.device("cuda:0")
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


def timed(fn, calls, rounds=5):
    """(device ms, host ms) per call: `calls` back to back between two device events and two host stamps that end in a synchronise;
    medians over `rounds` after one warm round, with the extremes of the device time."""
    d, h = [], []
    for r in range(rounds + 1):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        a.record()
        for _ in range(calls):
            fn()
        b.record()
        torch.cuda.synchronize()
        if r:
            d.append(a.elapsed_time(b) / calls)
            h.append((time.perf_counter() - t0) * 1e3 / calls)
    return float(np.median(d)), min(d), max(d), float(np.median(h))


_SETS = {}


def raw_batch(B, sizes, target):
    if target not in _SETS:
        _SETS[target] = loader.SyntheticRawEyes(8, seed=100, sizes=sizes, target=target)
    return loader.collate_raw([_SETS[target][i % 8] for i in range(B)])


def one_setting(B, scale, augment):
    target, sizes = ((480, 640), [(480, 640), (472, 632)]) if scale else ((240, 320), [(240, 320), (232, 312)])
    raw = raw_batch(B, sizes, target)
    np.random.seed(1)
    call = lambda: loader.device_batch(raw, size=target, scale=scale, augment=augment, on_cv2="device")      # noqa: E731
    calls = 10 if B == 64 else 4
    d, lo, hi, h = timed(call, calls)
    step = B / TRAIN_RATE * 1e3
    say("B %3d  scale %-4s augment %-3s  device_batch %7.2f ms (%.2f .. %.2f) on the device, %7.2f ms of host wall time per call; the step "
        "that consumes it: %.1f ms at %d frames/s  -> %.1f %% of it" % (B, scale or "no", "on" if augment else "off", d, lo, hi, h, step, TRAIN_RATE, 100 * d / step))
    # the same work stage by stage, inputs already on the device
    img_d, lab_d = torch.from_numpy(raw.images).to(dev), torch.from_numpy(raw.labels).to(dev)
    el, pc = loader.stage_geometry(raw.elParam, raw.pupil_center, raw.src_hw, target, scale)
    si, sl = loader.stage(img_d, lab_d, raw.src_hw, target, scale)
    ai, al = si, sl
    parts = [("host-to-device copy of the raw batch", lambda: (torch.from_numpy(raw.images).to(dev), torch.from_numpy(raw.labels).to(dev))),
             ("stage (egne_loader_stage)", lambda: loader.stage(img_d, lab_d, raw.src_hw, target, scale))]
    if augment:
        parts.append(("augment_batch (draws on the host, 1-2 launches)", lambda: DA.augment_batch(si, sl, pc, el, on_cv2="device")))
        ai, al = DA.augment_batch(si, sl, pc, el, on_cv2="device")[:2]
    x, fl = loader.finish(ai, al)
    cond = torch.from_numpy(raw.cond).to(dev)
    el_d = el.to(dev)
    parts += [("finish (egne_loader_finish)", lambda: loader.finish(ai, al)),
              ("spatial_weights", lambda: dataprep.spatial_weights(fl)),
              ("dist_maps", lambda: dataprep.dist_maps(fl)),
              ("geometry on the host (pad shift, scale)", lambda: loader.stage_geometry(raw.elParam, raw.pupil_center, raw.src_hw, target, scale)),
              ("ellipse normalisation (torch, float64)", lambda: dataprep._ellipse_info(el_d, fl.shape[1], fl.shape[2]))]
    for name, fn in parts:
        pd, plo, phi, ph = timed(fn, calls, rounds=3)
        say("        %-52s %8.3f ms device (%.3f .. %.3f)  %8.3f ms host" % (name, pd, plo, phi, ph))


say("egne_amd.loader.device_batch on MI355X, one process; eager calls back to back between two device events (and two host stamps that end")
say("in a synchronise), median (min .. max) of 5 rounds after a warm round; the batch it returns is 240 x 320.  'no' scaling: raw frames of")
say("240 x 320 and 232 x 312; scale 0.5: raw frames of 480 x 640 and 472 x 632.  Augmentation: the reference's draw per frame, on_cv2=\"device\".")
say("")
for B in (64, 256):
    for scale in (False, 0.5):
        for augment in (False, True):
            one_setting(B, scale, augment)
    say("")

samples = [R.raw_case(7 + i, 240, 320) for i in range(4)]
torch.set_num_threads(1)
t = []
for rnd in range(3):
    t0 = time.perf_counter()
    for s in samples:
        R.item(s, (240, 320))
    t.append((time.perf_counter() - t0) / 4 * 1e3)
say("host restatement of the item path (tests/loader_refs.py: pad, remap, Canny / dilate restatement, three distance transforms, z-score,")
say("ellipse normalisation; no augmentation, NumPy / SciPy on one core), four 240 x 320 frames: %.1f ms per frame (best of 3 rounds: %.1f) = %.0f "
    "frames/s per core" % (float(np.median(t)), min(t), 1e3 / min(t)))
os.makedirs(os.path.dirname(OUT), exist_ok=True)
with open(OUT, "w") as f:
    f.write("\n".join(lines) + "\n")
