"""Measurement of the label maps from TEyeD annotations (csrc/annot.hip, egne_amd.dataprep.labels_from_annotations).  Writes
profiles/annot.txt (or the path given as the first argument).

(a) the call alone (three launches) at 480 x 640 for B = 1, 64 and 256, both maps and Masks_noSkin only, device events around
    back-to-back calls.  Beside it, on the same box and the same buffers, a plain fill of the same bytes (torch.zero_), and the time
    the bytes written would take at 6.3 TB/s, the achievable HBM rate MI355X_MICROARCH gives.
(b) loader.device_batch (augment=False, size 480 x 640, scale 0.5) from an AnnotBatch against a RawBatch of the same frames, at
    B = 64 and 256, taking turns; a host clock around the call up to a device synchronise, because the upload is host work.  The
    RawBatch path is the code the parent commit runs.
The annotations and frames are seeded (tests/annot_refs.seeded_annotations / seeded_frames).
"""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch

import annot_refs as R
import egne_amd  # noqa: F401
from egne_amd import dataprep, loader

OUT = os.path.abspath(sys.argv[1]) if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "annot.txt")
PARTS = sys.argv[2] if len(sys.argv) > 2 else "ab"
dev = torch.device("cuda:0")
lines = []
HBM = 6.3e12


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
        a.record()
        for _ in range(reps):
            fn()
        b.record()
        torch.cuda.synchronize()
        if r:
            us.append(a.elapsed_time(b) * 1e3 / reps)
    return us


def records(B, seed):
    base = dataprep.pack_annotations(*R.seeded_annotations(min(B, 64), seed))
    return np.concatenate([base] * ((B + len(base) - 1) // len(base)))[:B]


def part_a():
    Rr, C = 480, 640
    say("(a) 480 x 640, seeded annotations (34-point lids); us per call on the device, median (min .. max) of 5 rounds after a warm one")
    for B in (1, 64, 256):
        rec = torch.from_numpy(records(B, 90)).to(dev)
        bufs = [torch.empty((B, Rr, C), dtype=torch.int8, device=dev) for _ in range(2)]
        reps = 200 if B == 1 else 50
        for skin in (True, False):
            out = bufs if skin else bufs[0]
            us = timed(lambda: dataprep.labels_from_annotations(rec, (Rr, C), with_skin=skin, out=out), reps)
            fill = timed((lambda: (bufs[0].zero_(), bufs[1].zero_())) if skin else (lambda: bufs[0].zero_()), reps)
            nbytes = B * Rr * C * (2 if skin else 1)
            floor = nbytes / HBM * 1e6
            say("    B %3d, %-17s labels_from_annotations %s us   torch.zero_ of the same %5.1f MB %s us   ratio %.2f   bytes / 6.3 TB/s %.1f us (x %.1f)"
                % (B, "both maps:" if skin else "Masks_noSkin only:", spread(us), nbytes / 1e6, spread(fill), np.median(us) / np.median(fill), floor,
                   np.median(us) / floor))
        (ns, sk), st = dataprep.labels_from_annotations(rec, (Rr, C), return_status=True)
        say("           class shares of Masks_noSkin %s, of Masks %s; status words all zero: %s"
            % (np.round(torch.bincount(ns.flatten().long(), minlength=4).cpu().numpy() / ns.numel(), 3).tolist(),
               np.round(torch.bincount(sk.flatten().long(), minlength=4).cpu().numpy() / sk.numel(), 3).tolist(), not bool(st.any())))


def part_b():
    Rr, C = 480, 640
    say("(b) loader.device_batch(size=(480, 640), scale=0.5, augment=False), ms per batch by a host clock up to a device synchronise; the two "
        "kinds take turns, median (min .. max) of 7 rounds after a warm one")
    for B in (64, 256):
        ball, iris, pupil, lid = R.seeded_annotations(64, 91)
        idx = np.arange(B) % 64
        rec = dataprep.pack_annotations(ball[idx], iris[idx], pupil[idx], lid[idx])
        frames = R.seeded_frames(8, Rr, C, 92)[np.arange(B) % 8]
        loc, fp, fi = dataprep.annotation_fits(iris[idx], pupil[idx])
        el = np.stack([fi, fp], axis=1)
        hw = np.tile(np.array([[Rr, C]], np.int32), (B, 1))
        labels = dataprep.labels_from_annotations(rec, (Rr, C), with_skin=False).cpu().numpy()
        cond = np.zeros((B, 4), bool)
        info = np.zeros((B, 3), np.int64)
        rb = loader.RawBatch(frames, labels, hw, el, loc, cond, info)
        ab = loader.AnnotBatch(frames, rec, hw, el, loc, cond, info)
        res = {"raw": [], "annot": []}
        outs = {}
        for r in range(8):
            for name, batch in (("raw", rb), ("annot", ab)):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                outs[name] = loader.device_batch(batch, size=(Rr, C), scale=0.5, augment=False)
                torch.cuda.synchronize()
                if r:
                    res[name].append((time.perf_counter() - t0) * 1e3)
        same = all(torch.equal(x, y) for x, y in zip(outs["raw"], outs["annot"]))
        widest = max(max(v) - min(v) for v in res.values())
        diff = float(np.median(res["annot"]) - np.median(res["raw"]))
        say("    B %3d: RawBatch (uploads %5.1f MB of labels) %s ms   AnnotBatch (uploads %5.1f KB of records, paints) %s ms   difference of the medians %+.2f ms, "
            "rounds of one kind spread over %.2f ms: %s; the nine tensors equal bit for bit: %s"
            % (B, labels.nbytes / 1e6, spread(res["raw"]), rec.nbytes / 1e3, spread(res["annot"]), diff, widest,
               "resolved" if abs(diff) > widest else "not resolved", same))


say("Label maps from TEyeD annotations (csrc/annot.hip, egne_amd.dataprep.labels_from_annotations) on MI355X, one process.")
if "a" in PARTS:
    part_a()
if "b" in PARTS:
    part_b()
os.makedirs(os.path.dirname(OUT), exist_ok=True)
with open(OUT, "w") as f:
    f.write("\n".join(lines) + "\n")
