"""-m gpu: test.py --device_metrics / --record_iou and train.py --track_scores end to end on synthetic frames (the pattern of
tests/test_gpu_scripts.py): what the scripts return, print and write with the flags on is what the host path computes from the same
tensors, bit for bit."""
import json
import os
import pickle
import re

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
SETTING = ["--setting", "configs/baseline_edge.yaml"]


@pytest.fixture(autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _same(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return a.shape == b.shape and np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(a[~np.isnan(a)], b[~np.isnan(b)])


def test_test_py_device_metrics_and_record_iou(tmp_path, monkeypatch, capsys):
    """16 synthetic frames in batches of 8: the four return values and the printed lines with --device_metrics 1 equal those of the host
    path; --record_iou 1 leaves the [16,3] per-sample IoUs of the ledger's rows; without --device_metrics 1 it says what it needs."""
    monkeypatch.chdir(tmp_path)
    from egne_amd import scores
    from egne_amd import test as T
    base = ["--synthetic", "16", "--batchsize", "8"] + SETTING
    host = T.main(base + ["--device_metrics", "0", "--record_iou", "1"])
    out_host = capsys.readouterr().out
    assert "needs --device_metrics 1" in out_host and not os.path.exists("img")
    seen = []
    orig = scores.ScoreLedger.rows
    monkeypatch.setattr(scores.ScoreLedger, "rows", lambda self: seen.append(orig(self)) or seen[-1])
    dev = T.main(base + ["--device_metrics", "1", "--record_iou", "1"])
    out_dev = capsys.readouterr().out
    assert len(host) == len(dev) == 4
    for h, d in zip(host, dev):
        assert _same(h, d), (host, dev)
    lines = lambda s: [l for l in s.splitlines() if l.startswith(("mIoU", "Latent", "Segmentation"))]      # noqa: E731
    assert len(lines(out_host)) == 5 and lines(out_host) == lines(out_dev)
    assert len(seen) == 1 and seen[0].shape == (16, scores.FIELDS)
    with open(os.path.join("img", "synthetic_baseline_ious.pkl"), "rb") as f:
        ious = pickle.load(f)
    assert ious.shape == (16, 3) and _same(ious, seen[0][:, scores.IOU:scores.IOU + 3]) and np.isfinite(ious).any()


def _train(TR, monkeypatch, expname, flag):
    got = []
    orig = TR.lossandaccuracy

    def spy(*a, **k):
        got.append(orig(*a, **k))
        return got[-1]
    monkeypatch.setattr(TR, "lossandaccuracy", spy)
    m = TR.main(["--synthetic", "16", "--batchsize", "4", "--epochs", "1", "--expname", expname, "--track_scores", flag] + SETTING)
    monkeypatch.setattr(TR, "lossandaccuracy", orig)
    return m, got


def test_train_py_track_scores(tmp_path, monkeypatch, capsys):
    """One epoch of 4 steps with --track_scores 1: one JSON line whose train_iou and iri_c/mu are the host functions applied to the
    tensors every append saw (captured by a hook here); validation returns and prints what --track_scores 0 does; the training plan's
    launch list has the same length either way (the ledger's two launches are queued behind the plan, not into it)."""
    monkeypatch.chdir(tmp_path)
    from egne_amd import scores, utils
    from egne_amd import train as TR
    m0, v0 = _train(TR, monkeypatch, "s0", "0")
    out0 = capsys.readouterr().out
    assert not os.path.exists(os.path.join("logs", "ritnet_v2", "s0", "scores.jsonl")) and "Train IoU" not in out0
    captured = {}
    orig = scores.ScoreLedger.append

    def hook(self, labels, mask, elOut, elPred, pc, ic, elNorm, cond, loss_terms=None):
        captured.setdefault(id(self), []).append([t.detach().cpu().numpy() for t in (labels, mask, elOut, elPred, pc, ic, elNorm, cond)])
        return orig(self, labels, mask, elOut, elPred, pc, ic, elNorm, cond, loss_terms)
    monkeypatch.setattr(scores.ScoreLedger, "append", hook)
    m1, v1 = _train(TR, monkeypatch, "s1", "1")
    out1 = capsys.readouterr().out
    assert len(v0) == len(v1) == 1 and _same(v0[0], v1[0]), (v0, v1)
    done = lambda s: re.findall(r"valid loss (\S+) mIoU (\S+)", s)      # noqa: E731
    assert len(done(out0)) == 1 and done(out0) == done(out1)
    assert m0._plans and {str(k): len(p.calls) for k, p in m0._plans.items()} == {str(k): len(p.calls) for k, p in m1._plans.items()}
    with open(os.path.join("logs", "ritnet_v2", "s1", "scores.jsonl")) as f:
        recs = [json.loads(l) for l in f]
    assert len(recs) == 1 and recs[0]["epoch"] == 0 and set(recs[0]) == {"epoch", "train", "valid", "loss/train", "loss/valid"}
    train_batches, valid_batches = list(captured.values())       # (the training ledger appends first)
    assert [len(b[0]) for b in train_batches] == [4, 4, 4, 4] and sum(len(b[0]) for b in valid_batches) == 4
    for name, bs in (("train", train_batches), ("valid", valid_batches)):
        ious, iri = [], []
        for labels, mask, elOut, elPred, pc, ic, elNorm, cond in bs:
            cf = cond.astype(np.float32)
            ious.append(utils.getSeg_metrics(labels, mask, cf[:, 1])[1])
            iri.append(utils.getPoint_metric(ic, elOut[:, 0:2], cf[:, 1], labels.shape[1:], True)[0])
        assert _same(recs[0][name]["train_iou"], np.nanmean(np.stack(ious, axis=0), axis=0)), name
        assert _same(recs[0][name]["iri_c/mu"], np.nanmean(iri)), name
    assert _same(recs[0]["loss/valid"], v1[0][0])
    assert re.search(r"^Epoch:0, Train IoU: \[", out1, re.M)
