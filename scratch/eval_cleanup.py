"""Measurement of evaluate.py --clean_mask 1: egne_class_map_cleanup (eleven launches) alone on preallocated
buffers by device events at 1 and 64 frames of 240 x 320 (2 and 128 rows), on drawn discs, on the network's class maps and on noise
+ checkerboard; the seed step + the search of --ellipse_seed mask and ransac on the raw map and on the cleaned map (the stage's own
time on top) -- all settings of a class map interleaved round by round in one process; then the --low_latency 1 --device_io 1 loop
per frame pair for the three seed kinds with and without the stage, interleaved, two rounds each.  Writes profiles/eval_cleanup.txt."""
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
from egne_amd.utils import (_layer_rows, _mesh_axes, _ransac_rows, _region_rows, DEFAULT_CLEAN_LAYERS, DEFAULT_RANSAC_REGIONS,
                            DEFAULT_SEED_REGIONS)
from common import bdcn_module, esf_module, gold
import mask_seed_refs as R

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
    raw_map = torch.from_numpy(mask_np).to(dev)
    cleaned = torch.empty_like(raw_map)
    st = _lib.stream_ptr()
    xs, ys = _mesh_axes(H, W, dev)
    f64 = lambda *s: torch.empty(s, dtype=torch.float64, device=dev)      # noqa: E731
    i32 = lambda *s: torch.empty(s, dtype=torch.int32, device=dev)        # noqa: E731
    i64 = lambda *s: torch.empty(s, dtype=torch.int64, device=dev)        # noqa: E731
    # the stage
    lfo, lcb, lpc, lfl = _layer_rows(DEFAULT_CLEAN_LAYERS, F, dev)
    ws_c = i64(int(L.egne_class_map_cleanup_workspace_bytes(n, H, W)) // 8 + 1)
    stats_c, status_c = i64(n, 4), i32(1)
    # mask seeds
    fo_in, cb, sc = _region_rows(DEFAULT_SEED_REGIONS, F, dev)
    ws_m = i64(int(L.egne_mask_seed_workspace_bytes(n, H, W)) // 8 + 1)
    init_m, fo_m, cl_m, stats_m, status_m = f64(n, 5), i32(n), i32(n), i64(n, 8), i32(1)
    # ransac
    rfo, rcb, rsc, reb = _ransac_rows(DEFAULT_RANSAC_REGIONS, F, dev)
    ws_r = i64(int(L.egne_ellipse_ransac_workspace_bytes(n, H, W, MAX_PTS)) // 8 + 1)
    raw, init_r, fo_r, cl_r, si, sf, status_r = f64(n, 5), f64(n, 5), i32(n), i32(n), i32(n, 4), f64(n, 2), i32(1)
    res = f64(n, 5)

    def clean():
        assert L.egne_class_map_cleanup(raw_map.data_ptr(), F, lfo.data_ptr(), lcb.data_ptr(), lpc.data_ptr(), lfl.data_ptr(), n, H, W, 1, 1,
                                        0, cleaned.data_ptr(), stats_c.data_ptr(), status_c.data_ptr(), ws_c.data_ptr(), st) == 0

    def mask_path(m):
        assert L.egne_ellipse_init_from_mask(m.data_ptr(), F, fo_in.data_ptr(), cb.data_ptr(), sc.data_ptr(), n, H, W, 7, init_m.data_ptr(),
                                             fo_m.data_ptr(), cl_m.data_ptr(), stats_m.data_ptr(), status_m.data_ptr(), ws_m.data_ptr(),
                                             st) == 0
        assert L.egne_ellipse_fit(m.data_ptr(), F, fo_m.data_ptr(), cl_m.data_ptr(), n, H, W, xs.data_ptr(), ys.data_ptr(), init_m.data_ptr(),
                                  res.data_ptr(), None, st) == 0

    def ransac_path(m):
        assert L.egne_ellipse_ransac_from_mask(m.data_ptr(), F, rfo.data_ptr(), rcb.data_ptr(), rsc.data_ptr(), reb.data_ptr(), n, H, W,
                                               MAX_PTS, N_MIN, ITERS, THRES, N_GOOD, None, 0, 2, None, raw.data_ptr(), init_r.data_ptr(),
                                               fo_r.data_ptr(), cl_r.data_ptr(), si.data_ptr(), sf.data_ptr(), None, status_r.data_ptr(),
                                               ws_r.data_ptr(), st) == 0, L.egne_last_error()
        assert L.egne_ellipse_fit(m.data_ptr(), F, fo_r.data_ptr(), cl_r.data_ptr(), n, H, W, xs.data_ptr(), ys.data_ptr(), init_r.data_ptr(),
                                  res.data_ptr(), None, st) == 0

    def both(path):
        clean()
        path(cleaned)
    clean()
    torch.cuda.synchronize()
    s = stats_c.cpu().numpy()
    changed = int((cleaned != raw_map).sum().item())
    assert int(status_c.item()) == 0
    say("%s, %d frames (%d rows; components per row up to %d, pixels added by filling per row up to %d, %d of %d pixels changed):"
        % (what, F, n, s[:, 1].max(), s[:, 3].max(), changed, raw_map.numel()))
    calls = 100 if n == 2 else 20
    t = interleaved({"clean": clean, "mask_raw": lambda: mask_path(raw_map), "mask_clean": lambda: both(mask_path),
                     "ransac_raw": lambda: ransac_path(raw_map), "ransac_clean": lambda: both(ransac_path)}, calls)
    say("    egne_class_map_cleanup (11 launches)                          %s" % t["clean"][0])
    say("    mask seeds + search on the raw map                            %s" % t["mask_raw"][0])
    say("    clean-up + mask seeds + search on the cleaned map             %s" % t["mask_clean"][0])
    say("    RANSAC seeds + search on the raw map                          %s" % t["ransac_raw"][0])
    say("    clean-up + RANSAC seeds + search on the cleaned map           %s" % t["ransac_clean"][0])
    say("    with the stage / without it: mask %.2f, ransac %.2f" % (t["mask_clean"][1] / t["mask_raw"][1],
                                                                      t["ransac_clean"][1] / t["ransac_raw"][1]))


say("evaluate.py --clean_mask 1 on MI355X, one process; device events around back-to-back eager calls on preallocated buffers, median")
say("(min .. max) of 5 rounds after a warm round, the settings of a class map taking turns inside every round; 240 x 320 class maps,")
say("default layers (iris blob of 1 | 2, pupil blob of 2 over it; opening, largest component, holes filled), default seed regions.")
say("Seeded random weights: no checkpoint exists here, so what the stage buys with trained weights is not measured.")
say("")
for F in (1, 64):
    measure("(a) drawn iris disc + pupil disc", drawn(F))
    measure("(a) class maps of the network on the example frames (seeded random weights: ragged maps)", network_maps(F))
    pats = R.patterns(H, W)
    measure("(a) worst cases: noise p = 0.6 as classes 1 | 2, checkerboard inside it as class 2",
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
    for seed in ("pred", "mask", "ransac"):
        for cm in ("0", "1"):
            del stamps[:]
            args = E.parse_args(["--low_latency", "1", "--device_io", "1", "--ellipse_seed", seed, "--clean_mask", cm,
                                 "--method", "l" + seed + cm])
            t0 = time.perf_counter()
            E.evaluate_ellseg_per_video(vid, args, net, bd, dev)
            t = np.diff(np.asarray([t0] + stamps))[WARM:] * 1e3
            say("(b) --low_latency 1 --device_io 1 loop, --ellipse_seed %-6s --clean_mask %s round %d: %8.3f %8.3f %8.3f ms per frame pair "
                "(median, mean, 90th percentile; %d pairs after %d warm-up)" % (seed, cm, rnd, np.median(t), t.mean(), np.percentile(t, 90),
                                                                              len(t), WARM))
E.MJPEGWriter.write, E.MJPEGWriter.release = real_write, real_release
os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
with open(os.path.join(ROOT, "profiles", "eval_cleanup.txt"), "w") as f:
    f.write("\n".join(lines) + "\n")
