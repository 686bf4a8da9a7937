"""Measurement of the device ElliFit + RANSAC: egne_ellipse_ransac_from_mask (five launches) alone on
preallocated buffers by device events at 2 and 128 rows (1 and 64 frames) of 240 x 320, on drawn discs and on the network's class
maps, next to the mask-seed step and the egne_ellipse_fit launch each of them feeds -- all settings of a class map interleaved
round by round in one process; then the --low_latency 1 --device_io 1 loop per frame pair with --ellipse_seed pred, mask and
ransac, interleaved, two rounds each.  Writes profiles/eval_ellifit.txt."""
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
from egne_amd.utils import _mesh_axes, _ransac_rows, _region_rows, DEFAULT_RANSAC_REGIONS, DEFAULT_SEED_REGIONS
from common import bdcn_module, esf_module, gold

WARM, STEPS = 20, 200
H, W = 240, 320
MAX_PTS, N_MIN, ITERS, THRES, N_GOOD = 4096, 15, 40, 5e-3, 15
dev = torch.device("cuda:0")
bd, net = bdcn_module().to(dev), esf_module("baseline_edge").to(dev).eval()
eyes = gold("evaluate_real_frames")["eyes"]
lines = []
L = _lib.lib()


def say(s):
    print(s, flush=True)
    lines.append(s)


def interleaved(fns, calls, rounds=5):
    """us per call of every function: `calls` back to back between two device events; the functions take turns inside a round, one
    warm round first; median (min .. max) over `rounds`."""
    out = {k: [] for k in fns}
    for r in range(rounds + 1):
        for k, fn in fns.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            a.record()
            for _ in range(calls):
                fn()
            b.record()
            torch.cuda.synchronize()
            if r:
                out[k].append(a.elapsed_time(b) * 1e3 / calls)
    return {k: ("%8.1f us (%.1f .. %.1f)" % (np.median(v), min(v), max(v)), float(np.median(v))) for k, v in out.items()}


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


def measure(what, mask_np):
    F = mask_np.shape[0]
    n = 2 * F
    m = torch.from_numpy(mask_np).to(dev)
    st = _lib.stream_ptr()
    xs, ys = _mesh_axes(H, W, dev)
    f64 = lambda *s: torch.empty(s, dtype=torch.float64, device=dev)      # noqa: E731
    i32 = lambda *s: torch.empty(s, dtype=torch.int32, device=dev)        # noqa: E731
    # mask seeds
    fo_in, cb, sc = _region_rows(DEFAULT_SEED_REGIONS, F, dev)
    ws_m = torch.empty(int(L.egne_mask_seed_workspace_bytes(n, H, W)) // 8 + 1, dtype=torch.int64, device=dev)
    init_m, fo_m, cl_m, stats_m, status_m = f64(n, 5), i32(n), i32(n), torch.empty((n, 8), dtype=torch.int64, device=dev), i32(1)
    # ransac
    rfo, rcb, rsc, reb = _ransac_rows(DEFAULT_RANSAC_REGIONS, F, dev)
    ws_r = torch.empty(int(L.egne_ellipse_ransac_workspace_bytes(n, H, W, MAX_PTS)) // 8 + 1, dtype=torch.int64, device=dev)
    raw, init_r, fo_r, cl_r, si, sf, status_r = f64(n, 5), f64(n, 5), i32(n), i32(n), i32(n, 4), f64(n, 2), i32(1)
    res = f64(n, 5)

    def seed_mask():
        assert L.egne_ellipse_init_from_mask(m.data_ptr(), F, fo_in.data_ptr(), cb.data_ptr(), sc.data_ptr(), n, H, W, 7, init_m.data_ptr(),
                                             fo_m.data_ptr(), cl_m.data_ptr(), stats_m.data_ptr(), status_m.data_ptr(), ws_m.data_ptr(),
                                             st) == 0

    def ransac(iters=ITERS):
        assert L.egne_ellipse_ransac_from_mask(m.data_ptr(), F, rfo.data_ptr(), rcb.data_ptr(), rsc.data_ptr(), reb.data_ptr(), n, H, W,
                                               MAX_PTS, N_MIN, iters, THRES, N_GOOD, None, 0, 2, None, raw.data_ptr(), init_r.data_ptr(),
                                               fo_r.data_ptr(), cl_r.data_ptr(), si.data_ptr(), sf.data_ptr(), None, status_r.data_ptr(),
                                               ws_r.data_ptr(), st) == 0, L.egne_last_error()

    def fit(init, fo, cl):
        assert L.egne_ellipse_fit(m.data_ptr(), F, fo.data_ptr(), cl.data_ptr(), n, H, W, xs.data_ptr(), ys.data_ptr(), init.data_ptr(),
                                  res.data_ptr(), None, st) == 0
    seed_mask()
    ransac()
    torch.cuda.synchronize()
    s = si.cpu().numpy()
    say("%s, %d frames (%d rows; boundary points per row %d .. %d, candidates per row up to %d, %d rows absent, status %d):"
        % (what, F, n, s[:, 0].min(), s[:, 0].max(), s[:, 3].max(), int((fo_r.cpu().numpy() < 0).sum()), int(status_r.item())))
    calls = 100 if n == 2 else 30
    t = interleaved({"ransac": ransac, "allpts": lambda: ransac(-1), "mask": seed_mask,
                     "fit_r": lambda: fit(init_r, fo_r, cl_r), "fit_m": lambda: fit(init_m, fo_m, cl_m)}, calls)
    ransac()
    say("    egne_ellipse_ransac_from_mask (5 launches, 41 iterations) %s" % t["ransac"][0])
    say("    the same with iters = -1 (points + all-points fit only)   %s" % t["allpts"][0])
    say("    egne_ellipse_init_from_mask (7 launches)                  %s" % t["mask"][0])
    say("    egne_ellipse_fit on the RANSAC seeds                      %s" % t["fit_r"][0])
    say("    egne_ellipse_fit on the mask seeds                        %s" % t["fit_m"][0])
    say("    RANSAC step / the search it feeds: %.2f;  RANSAC step / mask-seed step: %.2f"
        % (t["ransac"][1] / t["fit_r"][1], t["ransac"][1] / t["mask"][1]))


say("ElliFit + RANSAC on the device (csrc/ellifit.hip) on MI355X, one process; device events around back-to-back eager calls on")
say("preallocated buffers, the settings of a class map interleaved round by round, median (min .. max) of 5 rounds after a warm round;")
say("240 x 320 class maps, default regions, n_min 15, 40 iterations, T 5e-3, n_good 15, generated draws (seed 0), max_pts 4096")
say("")
for F in (1, 64):
    measure("(a) drawn iris disc + pupil disc", drawn(F))
    measure("(a) class maps of the network on the example frames (seeded random weights: ragged maps)", network_maps(F))
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
    for seed in ("pred", "mask", "ransac"):
        del stamps[:]
        args = E.parse_args(["--low_latency", "1", "--device_io", "1", "--ellipse_seed", seed, "--method", "l" + seed])
        t0 = time.perf_counter()
        E.evaluate_ellseg_per_video(vid, args, net, bd, dev)
        t = np.diff(np.asarray([t0] + stamps))[WARM:] * 1e3
        say("(b) --low_latency 1 --device_io 1 loop, --ellipse_seed %-6s round %d: %8.3f %8.3f %8.3f ms per frame pair (median, mean, 90th "
            "percentile; %d pairs after %d warm-up)" % (seed, rnd, np.median(t), t.mean(), np.percentile(t, 90), len(t), WARM))
E.MJPEGWriter.write, E.MJPEGWriter.release = real_write, real_release
os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
with open(os.path.join(ROOT, "profiles", "eval_ellifit.txt"), "w") as f:
    f.write("\n".join(lines) + "\n")
