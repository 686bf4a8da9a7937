"""-m gpu: csrc/scores.hip through egne_amd.scores against tests/scores_refs.py (pinned to the reference by tests/test_host_scores.py) and
against utils.getSeg_metrics / getPoint_metric / getAng_metric on host copies of the same tensors.  Integers and every row field
must be equal bit for bit, NaNs in the same places.

Shapes of the counting kernel (256 lanes take a pair of pixels each per pass of 512, a workgroup takes scores.CHUNK = 2048 pixels of a
frame): one pixel; less than a wave with an odd frame (the second frame starts 8-byte aligned only); one full wave of pairs plus an
odd tail; several passes with a ragged last one; the real 240 x 320 (37.5 chunks); and 3 x 6315 = 9 chunks + 1 pass + 1 pixel, odd,
so that frames 0 and 2 start 16-byte aligned and frame 1 does not."""
import numpy as np
import pytest
import torch

import scores_refs as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SHAPES = [(1, 1, 1), (2, 3, 5), (3, 7, 19), (5, 33, 65), (2, 240, 320), (3, 3, 6315)]


@pytest.fixture(autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _same(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return a.shape == b.shape and np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(a[~np.isnan(a)], b[~np.isnan(b)])


def _counts(yt, yp, ncls):
    from egne_amd import scores
    return scores.seg_confusion_counts(torch.from_numpy(yt).to(DEV), torch.from_numpy(yp).to(DEV), ncls).cpu().numpy()


@pytest.mark.parametrize("ncls", [2, 3])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_counts_equal_numpy(shape, ncls):
    """Maps with values outside [0, ncls) (negative, ncls, 255, 2^32 + 1) in both: they count for no class."""
    from egne_amd import scores
    assert scores.CHUNK == 2048 and 3 * 6315 == 9 * scores.CHUNK + 512 + 1
    yt, yp = R.maps(*shape, seed=sum(shape) + ncls, ncls=ncls)
    want = R.counts_ref(yt, yp, ncls)
    got = _counts(yt, yp, ncls)
    assert got.dtype == np.uint32 and np.array_equal(got, want)
    assert np.array_equal(_counts(yt, yp, ncls), got), "two runs differ"
    if ncls == 3:       # the rest of the pixels: all three classes sum to the frame where nothing strays
        yt2, yp2 = R.maps(*shape, seed=7, stray=False)
        c = _counts(yt2, yp2, 3)
        assert np.array_equal(c, R.counts_ref(yt2, yp2)) and (c[:, :, 0].sum(1) == shape[1] * shape[2]).all()


@pytest.mark.parametrize("off_t,off_p", [(1, 1), (1, 0), (0, 1)])
def test_counts_from_8_byte_aligned_bases(off_t, off_p):
    """Contiguous views that start 8 bytes behind a 16-byte boundary: both (pairs still line up) and one of the two (8-byte loads)."""
    from egne_amd import scores
    B, H, W = 3, 5, 13
    yt, yp = R.maps(B, H, W, seed=3)
    n = B * H * W
    ft, fp = torch.zeros(n + 2, dtype=torch.int64, device=DEV), torch.zeros(n + 2, dtype=torch.int64, device=DEV)
    vt, vp = ft[off_t:off_t + n].view(B, H, W), fp[off_p:off_p + n].view(B, H, W)
    vt.copy_(torch.from_numpy(yt)); vp.copy_(torch.from_numpy(yp))
    assert vt.data_ptr() % 16 == 8 * off_t and vp.data_ptr() % 16 == 8 * off_p and vt.is_contiguous()
    assert np.array_equal(scores.seg_confusion_counts(vt, vp).cpu().numpy(), R.counts_ref(yt, yp))


def test_wrong_inputs_are_refused():
    from egne_amd import scores
    yt, yp = (torch.from_numpy(a).to(DEV) for a in R.maps(2, 6, 8, seed=1))
    with pytest.raises(ValueError, match="contiguous"):
        scores.seg_confusion_counts(yt.transpose(1, 2), yp.transpose(1, 2))
    with pytest.raises(TypeError, match="int64"):
        scores.seg_confusion_counts(yt.to(torch.int32), yp)
    with pytest.raises(TypeError, match="int64"):
        scores.seg_confusion_counts(yt, yp.float())
    with pytest.raises(ValueError):
        scores.seg_confusion_counts(yt, yp[:1])
    with pytest.raises(ValueError):
        scores.seg_confusion_counts(yt, yp, ncls=4)
    with pytest.raises(RuntimeError):
        scores.seg_confusion_counts(yt.cpu(), yp.cpu())
    eo, ep, pc, ic, en, cond = (t.to(DEV) for t in R.vec_inputs(2, 5))
    led = scores.ScoreLedger(4, DEV)
    with pytest.raises(TypeError, match="float32"):
        led.append(yt, yp, eo, ep, pc.double(), ic, en, cond)
    with pytest.raises(TypeError, match="float32"):
        led.append(yt, yp, eo, ep, pc, ic.double(), en, cond)
    with pytest.raises(ValueError):
        led.append(yt, yp, eo[:, :9], ep, pc, ic, en, cond)
    assert led.n == 0 and led.rows().shape == (0, scores.FIELDS)


@pytest.fixture(scope="module")
def filled():
    """A ledger of 12 rows filled by three appends of 5, 4 and 3 samples (9 x 11 maps; a frame without pupil and one of a single
    class among them), the inputs, and the rows read back.  Computed once, never modified."""
    from egne_amd import scores
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    led = scores.ScoreLedger(12, DEV)
    parts = []
    for bn, n in enumerate((5, 4, 3)):
        yt, yp = R.maps(n, 9, 11, seed=20 + bn, stray=False)
        if bn == 0:
            yt[1][yt[1] == 2] = 1
            yt[2][:] = 0
        vec = R.vec_inputs(n, 30 + bn, (9, 11))
        loss = torch.tensor([0.25 + bn, 9.0], dtype=torch.float32) if bn != 1 else None
        led.append(torch.from_numpy(yt).to(DEV), torch.from_numpy(yp).to(DEV), *(t.to(DEV) for t in vec),
                   loss_terms=None if loss is None else loss.to(DEV))
        parts.append((yt, yp, vec, None if loss is None else float(loss[0])))
    return led, parts, led.rows()


def test_three_appends_land_at_their_offsets(filled):
    from egne_amd import scores
    led, parts, rows = filled
    assert rows.shape == (12, scores.FIELDS) and rows.dtype == np.float64 and led.n == 12 and led.batches == 3
    want = np.concatenate([R.rows_ref(yt, yp, *vec, loss=loss, batch_no=bn) for bn, (yt, yp, vec, loss) in enumerate(parts)])
    for f in range(scores.FIELDS):
        assert _same(rows[:, f], want[:, f]), "field %d: %r != %r" % (f, rows[:, f], want[:, f])
    assert [len(b) for b in scores.batches(rows)] == [5, 4, 3]
    assert np.isnan(rows[5:9, scores.LOSS]).all() and (rows[:5, scores.LOSS] == 0.25).all()


def test_rows_reduce_to_the_host_functions(filled):
    """Per batch: utils.getSeg_metrics, getPoint_metric and getAng_metric on host copies of the tensors against the reductions over rows."""
    from egne_amd import scores, utils
    _, parts, rows = filled
    for b, (yt, yp, vec, _) in zip(scores.batches(rows), parts):
        eo, ep, pc, ic, en, cond = (t.numpy() for t in vec)
        cf = cond.astype(np.float32)
        h = utils.getSeg_metrics(yt, yp, cf[:, 1])
        g = scores.seg_metrics(b)
        assert all(_same(a, c) for a, c in zip(g, h))
        for which, gt, pred, fc in (("pupil_latent", pc, eo[:, 5:7], 0), ("pupil_seg", pc, ep[:, 5:7], 0),
                                    ("iris_latent", ic, eo[:, 0:2], 1), ("iris_seg", ic, ep[:, 0:2], 1)):
            h = utils.getPoint_metric(gt, pred, cf[:, fc], (9, 11), True)
            g = scores.point_metric(b, which, fc)
            assert _same(g[0], h[0]) and _same(g[1], h[1]), which
        for k, which in enumerate(("iris", "pupil")):
            h = utils.getAng_metric(en[:, k, 4], eo[:, (4, 9)[k]], cf[:, 1])
            g = scores.ang_metric(b, which)
            assert _same(g[0], h[0]) and _same(g[1], h[1]), which
    assert np.isposinf(rows[0, scores.SCALE_IRIS]) and np.isnan(rows[1, scores.SCALE_PUPIL])


def test_full_ledger_raises_and_reset_clears(filled):
    from egne_amd import scores
    led, parts, rows = filled
    yt, yp, vec, _ = parts[2]
    with pytest.raises(RuntimeError, match="do not fit"):
        led.append(torch.from_numpy(yt).to(DEV), torch.from_numpy(yp).to(DEV), *(t.to(DEV) for t in vec))
    assert led.n == 12 and _same(led.rows(), rows)
    small = scores.ScoreLedger(3, DEV)
    small.append(torch.from_numpy(yt).to(DEV), torch.from_numpy(yp).to(DEV), *(t.to(DEV) for t in vec))
    assert _same(small.rows()[:, :scores.LOSS], rows[9:, :scores.LOSS])
    small.reset()
    assert small.n == 0 and small.batches == 0 and small.rows().shape == (0, scores.FIELDS)
    small.append(torch.from_numpy(yt).to(DEV), torch.from_numpy(yp).to(DEV), *(t.to(DEV) for t in vec))
    assert (small.rows()[:, scores.BATCH] == 0).all()


def test_two_classes_against_the_pupil_label():
    """ncls = 2 (DeepVOG: prediction 1 = pupil against labels == 2): the third IoU stays NaN, the first two are the host's."""
    from egne_amd import scores, utils
    yt, yp = R.maps(4, 9, 11, seed=8, stray=False)
    lab, pred = (yt == 2).astype(np.int64), (yp == 2).astype(np.int64)
    lab[3][:] = 0
    vec = R.vec_inputs(4, 9, (9, 11))
    led = scores.ScoreLedger(4, DEV, ncls=2)
    led.append(torch.from_numpy(lab).to(DEV), torch.from_numpy(pred).to(DEV), *(t.to(DEV) for t in vec))
    rows = led.rows()
    assert _same(rows, R.rows_ref(lab, pred, *vec, ncls=2))
    h = utils.getSeg_metrics(lab, pred, vec[5].numpy().astype(np.float32)[:, 1])
    assert all(_same(a, c) for a, c in zip(scores.seg_metrics(rows), h))
