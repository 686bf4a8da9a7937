"""Measurement of the self-consistency term (csrc/selfcorr.hip).  Writes profiles/selfcorr.txt.

1. egne_selfcorr_fwd (two launches) and egne_selfcorr_bwd (one) alone on preallocated buffers by device events, next to egne_loss_fwd
   and egne_loss_bwd of the same descriptor, at B = 64 and B = 256 frames of 240 x 320, logits stored as fp32 and as bf16 (NHWC slice,
   pix_stride 8); the four functions take turns inside a round.  Achieved bytes per second against the bytes the algorithm needs:
   forward = the logits slice read once (8 stored channels per pixel: the memory system fetches whole lines); backward = the same read
   plus a [B,3,H,W] fp32 tensor read and written.
2. One training step (forward + backward, no optimiser) of ESF-Net (baseline_edge) at B = 64 with selfCorr off and on, both storages,
   interleaved: the step that contains the launches.  Two models per setting: two models of one setting differ by more than the
   term costs.
3. bf16-storage gradient noise with and without the term (per-parameter gradient norms against the oracle's fp32 autograd, the
   statistic of tests/test_gpu_bf16.py) on the two batches tests/test_gpu_selfcorr.py uses.
"""
import ctypes as C
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch

import egne_amd  # noqa: F401
from egne_amd import _lib, synth
from common import batch_args, esf_module

H, W = 240, 320
dev = torch.device("cuda:0")
L = _lib.lib()
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


def interleaved(fns, calls, rounds=5):
    """ms per call of every function: `calls` back to back between two device events; the functions take turns inside a round, one
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
                out[k].append(a.elapsed_time(b) / calls)
    return {k: (float(np.median(v)), min(v), max(v)) for k, v in out.items()}


def op_level(B, dt):
    g = torch.Generator().manual_seed(B)
    st = _lib.stream_ptr()
    logits = (2 * torch.randn(B, H, W, 8, generator=g)).to(dt).to(dev)
    tgt = torch.randint(0, 3, (B, H, W), generator=g).to(dev)
    sw, dist = torch.ones(B, H, W, device=dev), torch.randn(B, 3, H, W, generator=g).to(dev)
    cond, pc = torch.zeros(B, 4, device=dev), (torch.rand(B, 2, generator=g) * torch.tensor([W, H])).to(dev)
    eln = (torch.rand(B, 2, 5, generator=g) * 2 - 1).to(dev)
    elOut = torch.tensor([0.05, -0.04, 0.55, 0.45, 0.3, 0.1, 0.02, 0.25, 0.2, 0.2]).repeat(B, 1).to(dev)
    gx, gy = torch.linspace(-1, 1, W).to(dev), torch.linspace(-1, 1, H).to(dev)
    part = torch.zeros(int(L.egne_loss_workspace_floats(B, H, W)), device=dev)
    terms, pcd, elp, coef = torch.zeros(8, device=dev), torch.zeros(B, 2, 2, device=dev), torch.zeros(B, 10, device=dev), torch.zeros(B, 32, device=dev)
    ws, sct = torch.zeros(int(L.egne_selfcorr_workspace_floats(B, H, W)), device=dev), torch.zeros(4, device=dev)
    up = (torch.zeros(B, 3, H, W, device=dev), torch.zeros(B, 2, 2, device=dev), torch.zeros(B, 10, device=dev))
    gl, ge, gsc = torch.zeros(B, H, W, 8, dtype=dt, device=dev), torch.zeros(B, 10, device=dev), torch.ones(1, device=dev)
    d = _lib.LossDesc()
    d.B, d.H, d.W = B, H, W
    d.logits, d.pix_stride, d.ch_off, d.dtype = logits.data_ptr(), 8, 0, (0 if dt == torch.float32 else 1)
    d.target, d.spatWts, d.distMap, d.cond = tgt.data_ptr(), sw.data_ptr(), dist.data_ptr(), cond.data_ptr()
    d.pupil_center, d.elNorm, d.elOut, d.alpha = pc.data_ptr(), eln.data_ptr(), elOut.data_ptr(), 0.3
    d.grid_x, d.grid_y = gx.data_ptr(), gy.data_ptr()
    d.partials, d.out_terms, d.pred_c, d.elPred = part.data_ptr(), terms.data_ptr(), pcd.data_ptr(), elp.data_ptr()
    d.coef = coef.data_ptr()
    d.g_op_nchw, d.g_pred_c, d.g_elOut_up = (t.data_ptr() for t in up)
    bwd = L.egne_loss_bwd if dt == torch.float32 else L.egne_loss_bwd_bf16
    fns = {
        "loss (egne_loss_fwd)": lambda: _lib.check(L.egne_loss_fwd(C.byref(d), st)),
        "selfcorr (egne_selfcorr_fwd)": lambda: _lib.check(L.egne_selfcorr_fwd(C.byref(d), 10.0, ws.data_ptr(), sct.data_ptr(), st)),
        "selfcorr.bwd (egne_selfcorr_bwd)": lambda: _lib.check(L.egne_selfcorr_bwd(C.byref(d), 10.0, ws.data_ptr(), gsc.data_ptr(), up[0].data_ptr(),
                                                                                   up[1].data_ptr(), up[2].data_ptr(), st)),
        "loss.bwd (egne_loss_bwd, upstream set)": lambda: _lib.check(bwd(C.byref(d), gsc.data_ptr(), gl.data_ptr(), 8, 0, ge.data_ptr(), st)),
    }
    res = interleaved(fns, calls=50)
    esz = 4 if dt == torch.float32 else 2
    read = B * H * W * 8 * esz
    nchw = B * 3 * H * W * 4
    alg = {"selfcorr (egne_selfcorr_fwd)": read, "selfcorr.bwd (egne_selfcorr_bwd)": read + 2 * nchw}
    say("B = %d, logits %s:" % (B, "fp32" if esz == 4 else "bf16"))
    for k, (med, lo, hi) in res.items():
        extra = "   %.3f GB algorithmic -> %.2f TB/s" % (alg[k] / 1e9, alg[k] / (med * 1e-3) / 1e12) if k in alg else ""
        say("    %-42s %8.4f ms (%.4f .. %.4f)%s" % (k, med, lo, hi, extra))
    torch.cuda.synchronize()


def step_level(B):
    b2 = synth.make_batch(2, seed=1234)
    g = torch.Generator().manual_seed(3)
    edge = torch.rand(B, 1, H, W, generator=g).to(dev)
    b = {k: (v.repeat(*([B // 2] + [1] * (v.dim() - 1))) if torch.is_tensor(v) else v) for k, v in b2.items()}
    args = [a.to(dev) if torch.is_tensor(a) else a for a in batch_args(b, edge)]
    # Two models of the same setting differ by several per cent in step time (which of them is slow changes from run to run and
    # follows the order in which they were built, not the flag: buffer placement), far more than the term's launches take, so each
    # setting is built twice, in the order off, on, on, off, and read against the spread between models of the SAME setting.
    import gc
    for dt in (torch.float32, torch.bfloat16):
        fns = {}
        for what, flag in (("selfCorr off", False), ("selfCorr on", True), ("selfCorr on, second model", True), ("selfCorr off, second model", False)):
            m = esf_module("baseline_edge").to(dev).to(dt)
            m.selfCorr = flag
            m.train()

            def step(m=m):
                m(*args)[3].sum().backward()
            step()                              # (the plan and its buffers are allocated here, in this order)
            fns[what] = step
        res = interleaved(fns, calls=10, rounds=4)
        say("training step (forward + backward) of ESF-Net baseline_edge, B = %d, %s storage:" % (B, "fp32" if dt == torch.float32 else "bf16"))
        for k, (med, lo, hi) in res.items():
            say("    %-32s %8.3f ms (%.3f .. %.3f)" % (k, med, lo, hi))
        del fns, m, step
        gc.collect()
        torch.cuda.empty_cache()


def bf16_noise():
    import test_gpu_selfcorr as T
    from egne_amd import engine
    from egne_amd.utils import calc_edge
    from common import bdcn_module
    import types
    say("bf16-storage gradient norms against the oracle's fp32 autograd (relative difference per parameter):")
    for what, bseed, wseed in (("batch seed 1234 / weights seed 0 (the setting of tests/test_gpu_bf16.py)", 1234, 0),
                               ("batch seed 77 / weights seed 5", 77, 5)):
        b = synth.make_batch(2, seed=bseed)
        old = engine.F16X3_ENABLED
        engine.F16X3_ENABLED = False
        try:
            edge = calc_edge(types.SimpleNamespace(prec=torch.float32, edge_thres=0), b["img"].to(dev), bdcn_module().to(dev), dev)
        finally:
            engine.F16X3_ENABLED = old
        sd = {k: v.clone() for k, v in esf_module("baseline_edge", seed=wseed).state_dict().items()}
        for flag in (False, True):
            lref, gref = T._oracle_grads(sd, b, edge, selfcorr=flag)
            lhip, params, _ = T._step(sd, b, edge, torch.bfloat16, selfcorr=flag)
            rel = T._norm_rel(params, gref)
            say("    %s, selfCorr %s: loss rel %.2e, median %.2e, 90th percentile %.2e, max %.2e"
                % (what, "on " if flag else "off", abs(lhip - lref) / abs(lref), np.median(rel), np.sort(rel)[int(0.9 * len(rel))], rel.max()))


def main():
    say("MI355X, %s" % torch.cuda.get_device_name(0))
    for B in (64, 256):
        for dt in (torch.float32, torch.bfloat16):
            op_level(B, dt)
    if "--no-noise" not in sys.argv:
        bf16_noise()
    if "--no-step" not in sys.argv:
        step_level(64)
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "selfcorr.txt"), "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
