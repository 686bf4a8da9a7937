#!/usr/bin/env python3
"""Record the REFERENCE's self-consistency term (loss.get_selfConsistency; DenseNet2D with selfCorr = True).

    python tests/golden/make_golden_selfcorr.py        # writes tests/golden/selfcorr.npz

Runs only where the reference is present; holds none of its text.

(a) loss.get_selfConsistency itself in float32 on the seeded cases of tests/selfcorr_refs.py: per case the value, the gradient w.r.t.
    the logits, the gradient w.r.t. elPred and which of its entries are finite.  Under current torch the reference's gradient w.r.t.
    the PUPIL ellipse is NaN as soon as one pixel of sigmoid(64 (1 - q)) underflows to 0 (kl_div's target gradient forms 0 * log 0);
    the generator asserts what the tests rely on: iris entries always finite, the covering set finite throughout, the typical set not.
(b) the reference's DenseNet2D (baseline_edge, B = 2, the seeded weights and batch of make_golden.gold_esf) with selfCorr = True in
    eval() and train(): the returned loss and the term it prints.  No gradients: they are NaN in the reference.
"""
import contextlib
import io
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import make_golden as MG  # noqa: E402  (installs the shim, imports the reference's modules)
import selfcorr_refs as R  # noqa: E402
from egne_amd import synth  # noqa: E402


def part_a(arrs):
    ref_loss = MG.REF["loss"]
    for shape, okp, es in R.CASES:
        op, el, ok = R.case_inputs(shape, okp, es)
        a, e = op.clone().requires_grad_(True), el.clone().requires_grad_(True)
        with contextlib.redirect_stdout(io.StringIO()):
            v = ref_loss.get_selfConsistency(a, e, ok)
        k = "a_" + R.case_key(shape, okp, es) + "_"
        if okp == "none":
            assert v == 0.0, v      # the reference returns the float 0.0: nothing to differentiate
            val, ga, ge = torch.zeros(()), torch.zeros_like(op), torch.zeros_like(el)
        else:
            ga, ge = torch.autograd.grad(v, (a, e))
            val = v.detach()
        fin = torch.isfinite(ge)
        assert torch.isfinite(val) and torch.isfinite(ga).all(), (shape, okp, es)
        assert fin[:, :5].all(), "iris gradient not finite: %s" % k
        if es == "covering":
            assert fin.all(), "the covering set must be finite throughout: %s" % k
        if es == "typical" and okp != "none":
            assert not fin[:, 5:].all(), "the typical set is expected to hit 0 * log 0: %s" % k
        arrs[k + "value"] = np.float32(val.item())
        arrs[k + "g_op"] = ga.numpy().astype(np.float32)
        arrs[k + "g_el"] = ge.numpy().astype(np.float32)
        arrs[k + "g_el_finite"] = fin.numpy()
        print("%-28s value %.6f  finite elPred entries %d / %d" % (k, val.item(), int(fin.sum()), fin.numel()))


def printed_term(text):
    vals = []
    for line in text.splitlines():
        try:
            vals.append(float(line.strip()))
        except ValueError:
            pass
    assert len(vals) == 1, "expected exactly one printed number, got %r" % text
    return vals[0]


def part_b(arrs):
    bd = MG.ref_bdcn()
    b = synth.make_batch(2, seed=1234)
    with torch.no_grad():
        edge = bd(torch.cat((b["img"],) * 3, 1))[-1]
    m = MG.ref_esf(MG.load_setting("baseline_edge"), "v2")
    m.selfCorr = True
    args = MG.batch_args(b, edge)
    arrs["b_img_sha"], arrs["b_edge_sha"] = MG.sha(b["img"]), MG.sha(edge)
    for mode in ("eval", "train"):
        getattr(m, mode)()
        out = io.StringIO()
        with contextlib.redirect_stdout(out), torch.set_grad_enabled(mode == "train"):
            loss = m(*args)[3]
        arrs["b_%s_loss" % mode] = loss.detach().numpy().astype(np.float32)
        arrs["b_%s_term" % mode] = np.float32(printed_term(out.getvalue()))
        print("DenseNet2D selfCorr %-5s loss %.6f term %.6f" % (mode, loss.item(), arrs["b_%s_term" % mode]))


def main():
    arrs = {}
    part_a(arrs)
    part_b(arrs)
    path = os.path.join(HERE, "selfcorr.npz")
    np.savez_compressed(path, **arrs)
    print("wrote %s %.1f KB" % (path, os.path.getsize(path) / 1024))


if __name__ == "__main__":
    main()
