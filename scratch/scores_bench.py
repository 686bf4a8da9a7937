"""Measurement of the device-side score tracking (egne_amd.scores).  Writes profiles/scores.txt (or the path
given as the first argument).

(a) the counts call (memset + counts kernel) at 64 and 256 frames of 240 x 320, device events around back-to-back calls that walk a
    ring of map pairs larger than the 256 MB Infinity Cache (every call reads its maps from HBM), beside its algorithmic bytes
    (16 per pixel) and the 6.3 TB/s a streaming read achieves on this chip; the row launch beside it.
(b) test.py's loop (calc_acc) over 512 synthetic frames in batches of 64 with --device_metrics 0 and 1, one process, the same
    loader and networks, taking turns, three times each: frames / s from a host clock around the call (it ends in a copy down).
(c) a train.py step at 64 frames (frozen edge network, forward, backward, fused Adam; the batch already on the device) without and
    with the ledger's append behind optimizer.step(), taking turns, three times each: device events around 10 steps.
"""
import os
import sys
import time
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

import egne_amd  # noqa: F401
from egne_amd import _entry, scores
from egne_amd.utils import calc_edge

OUT = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "scores.txt")
PARTS = sys.argv[2] if len(sys.argv) > 2 else "abc"
HBM = 6.3e12            # MI355X_MICROARCH: achievable streaming rate (8 TB/s on paper)
dev = torch.device("cuda:0")
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


def spread(v):
    return "%.1f (%.1f .. %.1f)" % (float(np.median(v)), min(v), max(v))


def part_a():
    H, W = 240, 320
    say("(a) egne_seg_confusion_counts, 240 x 320 int64 maps with classes 0..2, ring of map pairs > 512 MB; median (min .. max) of 5 rounds after a warm one")
    for B in (64, 256):
        nbytes = 16 * B * H * W
        ring = max(2, -(-(512 << 20) // nbytes))
        pairs = []
        for _ in range(ring):
            yt = torch.randint(0, 3, (B, H, W), device=dev)
            pairs.append((yt, torch.where(torch.rand(B, H, W, device=dev) < 0.8, yt, torch.randint(0, 3, (B, H, W), device=dev))))
        reps = max(1, 24 // ring)
        us = []
        for r in range(6):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            a.record()
            for _ in range(reps):
                for yt, yp in pairs:
                    scores.seg_confusion_counts(yt, yp)
            b.record()
            torch.cuda.synchronize()
            if r:
                us.append(a.elapsed_time(b) * 1e3 / (reps * ring))
        med = float(np.median(us))
        say("    B = %3d: %s us per call, %.1f MB read -> %.2f TB/s = %.0f %% of 6.3 TB/s   (%d pairs in the ring, %d calls per round)"
            % (B, spread(us), nbytes / 1e6, nbytes / med / 1e6, 100 * nbytes / (med * 1e-6) / HBM, ring, reps * ring))
        # the row launch with everything else of an append (host checks, small copies), maps from the same ring
        vec = [torch.rand(B, 10, device=dev), torch.rand(B, 10, device=dev), torch.rand(B, 2, device=dev) * 200, torch.rand(B, 2, device=dev) * 200,
               torch.rand(B, 2, 5, device=dev), torch.rand(B, 4, device=dev) < 0.2]
        led = scores.ScoreLedger(B * reps * ring, dev)
        us = []
        for r in range(6):
            led.reset()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            a.record()
            for _ in range(reps):
                for yt, yp in pairs:
                    led.append(yt, yp, *vec)
            b.record()
            host = (time.perf_counter() - t0) * 1e6 / (reps * ring)
            torch.cuda.synchronize()
            if r:
                us.append(a.elapsed_time(b) * 1e3 / (reps * ring))
        say("             ScoreLedger.append (counts + rows): %s us per call on the device, %.0f us of host time to queue it" % (spread(us), host))
        del pairs


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
    res = {0: [], 1: []}
    out = {}
    for r in range(4):
        for flag in (0, 1):
            args = types.SimpleNamespace(prec=torch.float32, edge_thres=0, test_normal=0, device_loader=0, device_metrics=flag, record_iou=0,
                                         model="ritnet_v2", batchsize=B, curObj=None, method="baseline")
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out[flag] = T.calc_acc(args, loader, model, edge_net, dev)
            torch.cuda.synchronize()
            if r:
                res[flag].append(N / (time.perf_counter() - t0))
    same = all(np.array_equal(np.float64(a), np.float64(b), equal_nan=True) for a, b in zip(out[0], out[1]))
    for flag in (0, 1):
        say("    --device_metrics %d: %s frames/s   (three runs after a warm one: %s)" % (flag, spread(res[flag]), ", ".join("%.1f" % v for v in res[flag])))
    say("    return values of the two settings equal bit for bit: %s" % same)
    # what the host pass costs by itself: the per-batch copies and NumPy work of --device_metrics 0 on one batch
    from egne_amd.utils import getSeg_metrics
    lab = torch.randint(0, 3, (B, 240, 320), device=dev)
    msk = torch.randint(0, 3, (B, 240, 320), device=dev)
    t = []
    for r in range(4):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        getSeg_metrics(lab.cpu().numpy(), msk.cpu().numpy(), np.zeros(B, np.float32))
        t.append((time.perf_counter() - t0) * 1e3)
    say("    the host pass alone on one batch of %d (two copies down + getSeg_metrics): %s ms" % (B, spread(t[1:])))


def part_c():
    from egne_amd import synth
    from egne_amd import train as TR
    setting = _entry.load_setting(os.path.join(os.path.dirname(TR.__file__), "configs", "baseline_edge.yaml"))
    B, steps = 64, 10
    torch.manual_seed(0)
    edge_net, model = _entry.seeded_networks(setting, "ritnet_v2", True)
    edge_net, model = edge_net.to(dev).eval(), model.to(dev).train()
    params = [p for n, p in model.named_parameters() if 'dsIdentify' not in n]
    opt = torch.optim.Adam(params, lr=5e-4, fused=True)
    b = {k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in synth.make_batch(B, seed=1234).items()}
    ic = torch.stack([(b["elNorm"][:, 0, 0] + 1) * 160, (b["elNorm"][:, 0, 1] + 1) * 120], dim=1).contiguous()
    args = types.SimpleNamespace(prec=torch.float32, edge_thres=0)
    led = scores.ScoreLedger(B * steps, dev)

    def step(track):
        edge = calc_edge(args, b["img"], edge_net, dev)
        opt.zero_grad()
        out = model(b["img"], edge, b["label"], b["pupil_center"], b["elNorm"], b["spatWts"], b["distMap"], b["cond"], b["ID"], 0.5)
        out[3].mean().backward()
        opt.step()
        if track:
            led.append(b["label"], model.predictions(), out[4], out[1], b["pupil_center"], ic, b["elNorm"], b["cond"], out[3])

    say("(c) a training step at B = %d (fp32 storage, --pipeline 0 order: edge network, forward, backward, fused Adam; batch on the device), "
        "device events around %d steps; runs take turns" % (B, steps))
    res = {0: [], 1: []}
    for r in range(4):
        for flag in (0, 1):
            led.reset()
            a, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            a.record()
            for _ in range(steps):
                step(flag)
            e.record()
            torch.cuda.synchronize()
            if r:
                res[flag].append(a.elapsed_time(e) / steps)
    for flag in (0, 1):
        say("    --track_scores %d: %s ms per step   (three runs after a warm one: %s)" % (flag, spread(res[flag]), ", ".join("%.2f" % v for v in res[flag])))
    say("    difference of the medians: %+.2f ms (%+.2f %%)" % (np.median(res[1]) - np.median(res[0]),
                                                                100 * (np.median(res[1]) / np.median(res[0]) - 1)))


say("Device-side score tracking (csrc/scores.hip, egne_amd.scores) on MI355X, one process.")
if "a" in PARTS:
    part_a()
if "b" in PARTS:
    part_b()
if "c" in PARTS:
    part_c()
os.makedirs(os.path.dirname(OUT), exist_ok=True)
with open(OUT, "w") as f:
    f.write("\n".join(lines) + "\n")
