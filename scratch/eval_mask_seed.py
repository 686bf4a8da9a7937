"""Measurement of evaluate.py --ellipse_seed mask: the seed step (egne_ellipse_init_from_mask, seven launches)
alone on preallocated buffers by device events at 2 and 128 rows (1 and 64 frames) of 240 x 320, next to egne_ellipse_init_from_pred and
the egne_ellipse_fit launch each of them feeds, in the same process; then the --low_latency 1 --device_io 1 loop per frame pair with
--ellipse_seed pred and mask, interleaved, two rounds each.  Writes profiles/eval_mask_seed.txt."""
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
from egne_amd import _lib, evaluate as E
from egne_amd.utils import _mesh_axes, _region_rows, DEFAULT_SEED_REGIONS
from common import bdcn_module, esf_module, gold
import mask_seed_refs as R

WARM, STEPS = 20, 200
H, W = 240, 320
dev = torch.device("cuda:0")
bd, net = bdcn_module().to(dev), esf_module("baseline_edge").to(dev).eval()
eyes = gold("evaluate_real_frames")["eyes"]
lines = []
L = _lib.lib()


def say(s):
    print(s, flush=True)
    lines.append(s)


def events(fn, calls, rounds=5):
    """us per call: `calls` back to back between two device events, median and extremes over `rounds` (after one warm round)."""
    out = []
    for r in range(rounds + 1):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        for _ in range(calls):
            fn()
        b.record()
        torch.cuda.synchronize()
        if r:
            out.append(a.elapsed_time(b) * 1e3 / calls)
    return "%8.1f us (%.1f .. %.1f)" % (np.median(out), min(out), max(out)), float(np.median(out))


def drawn(F):
    yy, xx = np.mgrid[0:H, 0:W]
    out = []
    for f in range(F):
        cy, cx = 120 + (f % 7) - 3, 160 + (f % 11) - 5
        r = np.hypot((yy - cy) * 1.1, xx - cx)
        out.append((r <= 70).astype(np.int64) + (r <= 25))
    return np.stack(out)


def network_maps(F):
    x = torch.stack([E.preprocess_frame(np.roll(eyes[k % 4], k // 4 - 8, 1), (H, W), True)[0] for k in range(F)]).to(dev)
    edge, seg, pup, iri = E.evaluate_ellseg_on_image(x, net, bd)
    return np.ascontiguousarray(seg).astype(np.int64)


def seed_and_fit(what, mask_np):
    F = mask_np.shape[0]
    n = 2 * F
    m = torch.from_numpy(mask_np).to(dev)
    fo_in, cb, sc = _region_rows(DEFAULT_SEED_REGIONS, F, dev)
    ws = torch.empty(int(L.egne_mask_seed_workspace_bytes(n, H, W)) // 8 + 1, dtype=torch.int64, device=dev)
    init = torch.empty((n, 5), dtype=torch.float64, device=dev)
    fo, cl = (torch.empty(n, dtype=torch.int32, device=dev) for _ in range(2))
    stats = torch.empty((n, 8), dtype=torch.int64, device=dev)
    status = torch.empty(1, dtype=torch.int32, device=dev)
    res = torch.empty((n, 5), dtype=torch.float64, device=dev)
    xs, ys = _mesh_axes(H, W, dev)
    st = _lib.stream_ptr()
    elp = torch.zeros((F, 10), dtype=torch.float32, device=dev)
    elp[:, 2:4], elp[:, 7:9] = 0.45, 0.16                      # a plausible regression output: centred, normalised axes
    pinit = torch.empty((n, 5), dtype=torch.float64, device=dev)
    pfo, pcl = (torch.empty(n, dtype=torch.int32, device=dev) for _ in range(2))

    def seed():
        assert L.egne_ellipse_init_from_mask(m.data_ptr(), F, fo_in.data_ptr(), cb.data_ptr(), sc.data_ptr(), n, H, W, 7, init.data_ptr(),
                                             fo.data_ptr(), cl.data_ptr(), stats.data_ptr(), status.data_ptr(), ws.data_ptr(), st) == 0

    def seed_pred():
        assert L.egne_ellipse_init_from_pred(elp.data_ptr(), F, H, W, pinit.data_ptr(), pfo.data_ptr(), pcl.data_ptr(), st) == 0

    def fit_mask():
        assert L.egne_ellipse_fit(m.data_ptr(), F, fo.data_ptr(), cl.data_ptr(), n, H, W, xs.data_ptr(), ys.data_ptr(), init.data_ptr(),
                                  res.data_ptr(), None, st) == 0

    def fit_pred():
        assert L.egne_ellipse_fit(m.data_ptr(), F, pfo.data_ptr(), pcl.data_ptr(), n, H, W, xs.data_ptr(), ys.data_ptr(), pinit.data_ptr(),
                                  res.data_ptr(), None, st) == 0
    seed()
    seed_pred()
    torch.cuda.synchronize()
    s = stats.cpu().numpy()
    assert int(status.item()) == 0
    calls = 200 if n == 2 else 50
    say("%s, %d frames (%d rows; components per row up to %d, chosen component up to %d pixels, %d rows absent):"
        % (what, F, n, s[:, 6].max(), s[:, 0].max(), int((fo.cpu().numpy() < 0).sum())))
    t_seed = events(seed, calls)
    say("    egne_ellipse_init_from_mask (7 launches)      %s" % t_seed[0])
    say("    egne_ellipse_init_from_pred (1 launch)        %s" % events(seed_pred, calls)[0])
    t_fm = events(fit_mask, calls)
    say("    egne_ellipse_fit on the mask seeds            %s" % t_fm[0])
    say("    egne_ellipse_fit on the regression-style seeds%s" % events(fit_pred, calls)[0])
    say("    seed step / the search it feeds: %.2f" % (t_seed[1] / t_fm[1]))


say("evaluate.py --ellipse_seed mask on MI355X, one process; device events around back-to-back eager calls on preallocated buffers,")
say("median (min .. max) of 5 rounds after a warm round; 240 x 320 class maps, default regions (iris = 1 | 2 scored against 1, pupil = 2)")
say("")
for F in (1, 64):
    seed_and_fit("(a) drawn iris disc + pupil disc", drawn(F))
    seed_and_fit("(a) class maps of the network on the example frames (seeded random weights: ragged maps)", network_maps(F))
    pats = R.patterns(H, W)
    seed_and_fit("(a) worst cases: noise p = 0.6 as classes 1 | 2, checkerboard inside it as class 2",
                 np.stack([(pats["noise_0.6"].astype(np.int64) + (pats["noise_0.6"] & pats["checkerboard"]))] * F))
    say("")

# ---- (b) the --low_latency 1 --device_io 1 loop: wall time per frame pair, from one written edge frame to the next -----------------------
tmpdir = tempfile.mkdtemp()
vid = os.path.join(tmpdir, "clip.avi")
w = E.MJPEGWriter(vid, 30, (640, 240))
for k in range(WARM + STEPS):
    a, b = eyes[2 * (k % 2)], eyes[2 * (k % 2) + 1]
    f = np.concatenate([np.roll(a, k % 17 - 8, 1), np.roll(b, 8 - k % 17, 1)], axis=1)
    w.write(np.stack([f] * 3, axis=2))
w.release()
stamps = []
real_write, real_release = E.MJPEGWriter.write, E.MJPEGWriter.release


def write(self, frame):
    real_write(self, frame)
    del self.frames[:]
    if "_edge_" in self.path:
        stamps.append(time.perf_counter())


E.MJPEGWriter.write, E.MJPEGWriter.release = write, (lambda self: None)
for rnd in range(2):
    for seed in ("pred", "mask"):
        del stamps[:]
        args = E.parse_args(["--low_latency", "1", "--device_io", "1", "--ellipse_seed", seed, "--method", "l" + seed])
        t0 = time.perf_counter()
        E.evaluate_ellseg_per_video(vid, args, net, bd, dev)
        t = np.diff(np.asarray([t0] + stamps))[WARM:] * 1e3
        say("(b) --low_latency 1 --device_io 1 loop, --ellipse_seed %s round %d: %8.3f %8.3f %8.3f ms per frame pair (median, mean, 90th "
            "percentile; %d pairs after %d warm-up)" % (seed, rnd, np.median(t), t.mean(), np.percentile(t, 90), len(t), WARM))
E.MJPEGWriter.write, E.MJPEGWriter.release = real_write, real_release
os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
with open(os.path.join(ROOT, "profiles", "eval_mask_seed.txt"), "w") as f:
    f.write("\n".join(lines) + "\n")
