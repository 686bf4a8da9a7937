"""Measurement of the ellipse scores against ground truth (egne_amd.scores.EllipseLedger, csrc/ellipse_scores.hip).  Writes
profiles/ellipse_scores.txt (or the path given as the first argument).

(a) the scoring launch alone (egne_ellipse_pair_scores through EllipseLedger.append with fit=, so that nothing else is queued) at
    1, 64 and 256 samples of 240 x 320, device events around back-to-back calls; beside it the two launches it follows in test.py:
    the pixel forms of elPred (egne_ellipse_init_from_pred) and the search (utils.fit_ellipses_from_pred, which exists already).
(b) test.py's loop (calc_acc) over 512 synthetic frames in batches of 64 with --device_metrics 1 and --ellipse_metrics 0, 1, and 1 with
    --ellipse_search 1: one process, the same loader and networks, taking turns, three times each after a warm round; frames / s from
    a host clock around the call (it ends in a copy down).
The weights are seeded random numbers: the metric VALUES mean nothing, only their agreement with the restatement does (tests).
"""
import contextlib
import io
import os
import sys
import time
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch

import egne_amd  # noqa: F401
from egne_amd import _entry, scores, utils

OUT = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "ellipse_scores.txt")
PARTS = sys.argv[2] if len(sys.argv) > 2 else "ab"
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
    import ellipse_scores_refs as R
    H, W = 240, 320
    say("(a) 240 x 320, seeded maps and ellipses (tests/ellipse_scores_refs.inputs, 8 samples repeated); us per call on the device, "
        "median (min .. max) of 5 rounds of 20 calls after a warm one; host = time to queue one call")
    base = R.inputs(H, W, 8, seed=11)
    for B in (1, 64, 256):
        d = {k: torch.from_numpy(np.concatenate([v] * (-(-B // 8)))[:B]).to(dev) for k, v in base.items()}
        led = scores.EllipseLedger(B, dev)
        fit = utils.ellipse_seeds_from_pred(d["elPred"], H, W)[0].view(B, 2, 5)

        def score():
            led.n = led.batches = 0          # (the same rows again: no fill of the buffer between the calls)
            led.append(d["mask"], None, d["elNorm"], d["cond"], fit=fit)
        us, host = timed(score, 20)
        say("    B = %3d: egne_ellipse_pair_scores            %s us   (host %.0f us)" % (B, spread(us), host))
        us, host = timed(lambda: utils.ellipse_seeds_from_pred(d["elPred"], H, W), 20)
        say("             egne_ellipse_init_from_pred         %s us   (host %.0f us)" % (spread(us), host))
        us, host = timed(lambda: utils.fit_ellipses_from_pred(d["mask"], d["elPred"]), 20)
        say("             seeds + egne_ellipse_fit (search)   %s us   (host %.0f us)" % (spread(us), host))


def part_b():
    from torch.utils.data import DataLoader
    from egne_amd import test as T
    setting = _entry.load_setting(os.path.join(os.path.dirname(T.__file__), "configs", "baseline_edge.yaml"))
    N, B = 512, 64
    data = _entry.SyntheticEyes(N)
    edge_net, model = _entry.seeded_networks(setting, "ritnet_v2")
    edge_net, model = edge_net.to(dev).eval(), model.to(dev)
    loader = DataLoader(data, batch_size=B, shuffle=False, num_workers=0, drop_last=True)
    say("(b) test.py's loop, --synthetic %d --batchsize %d --device_metrics 1, baseline_edge, seeded weights; host clock around calc_acc; "
        "runs take turns" % (N, B))
    kinds = (("--ellipse_metrics 0", 0, 0), ("--ellipse_metrics 1", 1, 0), ("--ellipse_metrics 1 --ellipse_search 1", 1, 1))
    res = {k[0]: [] for k in kinds}
    out, summ = {}, {}
    for r in range(4):
        for name, em, es in kinds:
            args = types.SimpleNamespace(prec=torch.float32, edge_thres=0, test_normal=0, device_loader=0, device_metrics=1, record_iou=0,
                                         ellipse_metrics=em, ellipse_search=es, model="ritnet_v2", batchsize=B, curObj=None, method="baseline")
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            with contextlib.redirect_stdout(io.StringIO()):
                out[name] = T.calc_acc(args, loader, model, edge_net, dev)
            torch.cuda.synchronize()
            summ[name] = T.calc_acc.last_ellipse_summary
            if r:
                res[name].append(N / (time.perf_counter() - t0))
    for name, _, _ in kinds:
        say("    %-40s %s frames/s   (three runs after a warm one: %s)" % (name + ":", spread(res[name]), ", ".join("%.1f" % v for v in res[name])))
    med = {k: float(np.median(v)) for k, v in res.items()}
    k0, k1, k2 = (k[0] for k in kinds)
    ms = lambda k: 1e3 * N / med[k] / (N // B)      # noqa: E731
    widest = max(1e3 * N / min(v) / (N // B) - 1e3 * N / max(v) / (N // B) for v in res.values())
    say("    per batch of %d, from the medians: %.2f ms without, %+.2f ms with the scoring launch, %+.2f ms more with the search launch; "
        "runs of ONE setting spread over up to %.2f ms, so differences below that are not resolved by this loop (see (a) for the launches)"
        % (B, ms(k0), ms(k1) - ms(k0), ms(k2) - ms(k1), widest))
    same = all(np.array_equal(np.float64(a), np.float64(b), equal_nan=True) for k in (k1, k2) for a, b in zip(out[k0], out[k]))
    say("    return values of the three settings equal bit for bit: %s; summary without the flag: %s" % (same, summ[k0]))
    say("    (random weights: box IoU iris %.4f pupil %.4f, searched %.4f / %.4f -- numbers without meaning)"
        % (summ[k1]["bbiou_iris"], summ[k1]["bbiou_pupil"], summ[k2]["bbiou_iris"], summ[k2]["bbiou_pupil"]))


say("Ellipse scores against ground truth (csrc/ellipse_scores.hip, egne_amd.scores.EllipseLedger) on MI355X, one process.")
if "a" in PARTS:
    part_a()
if "b" in PARTS:
    part_b()
os.makedirs(os.path.dirname(OUT), exist_ok=True)
with open(OUT, "w") as f:
    f.write("\n".join(lines) + "\n")
