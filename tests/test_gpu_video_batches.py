"""-m gpu: the video loop of evaluate.py across batches.  Five distinct frames at evaluate.BATCH_FRAMES = 2 make two full batches and
a ragged one, so results come back a batch late, the newest ready batch waits for the next, a redo reaches the batch queued behind
the overflowed one, and drain() empties both queues -- none of which a one-batch clip exercises."""
import itertools

import numpy as np
import pytest
import torch

import video_harness as V

pytestmark = pytest.mark.gpu
# (left eye, right eye) of frames F0..F4: halves permuted so that no two frames are alike.  320 columns are a multiple of the 16-pixel
# MCU, so an eye decodes to the same pixels on either side.
FRAMES = ((0, 1), (2, 3), (1, 0), (3, 2), (2, 1))
KEYS = set(range(5)) | {(j, i) for j in range(5) for i in range(2)}


@pytest.fixture(autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


@pytest.fixture(scope="module")
def nets():
    from common import bdcn_module, esf_module
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    dev = torch.device(V.DEV)
    return bdcn_module().to(dev), esf_module("baseline_edge").to(dev).eval()


@pytest.fixture
def E(monkeypatch):
    from egne_amd import evaluate
    monkeypatch.setattr(evaluate, "BATCH_FRAMES", 2)
    return evaluate


def test_batches_of_two_device_io_equals_the_host_path(tmp_path, nets, E):
    """--device_io 1 against --device_io 0 over batches (F0,F1), (F2,F3), (F4): equal dictionaries, byte-identical frames into both
    writers, in frame order."""
    vid = V.clip(tmp_path, FRAMES)
    V.run(vid, tmp_path, nets, [], "warm")
    host = V.run(vid, tmp_path, nets, ["--device_io", "0"], "host")
    dev = V.run(vid, tmp_path, nets, ["--device_io", "1"], "dev")
    assert not host.up and not host.down
    assert dev.up == [(torch.uint8, (2, 240, 640))] * 2 + [(torch.uint8, (1, 240, 640))]
    V.same_frames(host, dev, frames=5)
    assert [k for k, _ in host.written] == ["result", "edge"] * 5
    assert set(host.res) == KEYS and set(dev.res) == KEYS


@pytest.mark.parametrize("io", ["0", "1"])
def test_batches_of_two_redo_after_a_reported_overflow(tmp_path, nets, E, monkeypatch, io):
    """The first overflow query answers "overflowed": the first batch is done again, and so is the one queued behind it (the redo
    toggle) -- with the results of the undisturbed run."""
    vid = V.clip(tmp_path, FRAMES)
    V.run(vid, tmp_path, nets, ["--device_io", io], "warm")
    want = V.run(vid, tmp_path, nets, ["--device_io", io], "plain")
    real, calls = E._overflowed, []

    def once(net):
        calls.append(1)
        return True if len(calls) == 1 else real(net)
    monkeypatch.setattr(E, "_overflowed", once)
    got = V.run(vid, tmp_path, nets, ["--device_io", io], "redo")
    assert len(calls) > 2
    V.same_frames(want, got, frames=5)
    assert set(got.res) == KEYS


@pytest.mark.parametrize("io", ["0", "1"])
def test_batches_of_two_pair_results_with_their_frames(tmp_path, nets, E, monkeypatch, io):
    """Every (frame, eye) of the run in batches of two has its iris centre within 0.35 px (the bound test_evaluate_video_end_to_end
    holds between a batch of eight eyes and batches of two) of the run that takes all five frames as one batch.  The four eyes'
    centres differ pairwise by more than 1.0 px there (asserted; 17 px or more in the reference's own fits), so a result that lands
    on another frame or eye is further off than the bound."""
    from common import gold
    vid = V.clip(tmp_path, FRAMES)
    monkeypatch.setattr(E, "BATCH_FRAMES", 16)
    V.run(vid, tmp_path, nets, ["--device_io", io], "warm")
    one = V.run(vid, tmp_path, nets, ["--device_io", io], "one").res
    monkeypatch.setattr(E, "BATCH_FRAMES", 2)
    V.run(vid, tmp_path, nets, ["--device_io", io], "warm2")
    two = V.run(vid, tmp_path, nets, ["--device_io", io], "two").res
    assert set(one) == KEYS and set(two) == KEYS
    where = {0: (0, 0), 1: (0, 1), 2: (1, 0), 3: (1, 1)}           # eye -> a (frame, side) that shows it
    fits = gold("evaluate_real_frames")["fits"][:, 0, :2]
    for a, b in itertools.combinations(range(4), 2):
        apart = np.abs(one[where[a]][0][:2] - one[where[b]][0][:2]).max()
        print("iris centres of eyes %d and %d: %.2f px apart (reference's fits: %.2f)" % (a, b, apart, np.abs(fits[a] - fits[b]).max()))
        assert np.abs(fits[a] - fits[b]).max() >= 17
        assert apart > 1.0
    for k in sorted(KEYS - set(range(5))):
        print(k, two[k][0][:2], one[k][0][:2])
        np.testing.assert_allclose(two[k][0][:2], one[k][0][:2], atol=0.35, err_msg="frame %d eye %d" % k)


def test_batches_of_two_device_decode_writes_the_same_files(tmp_path, nets, E):
    """--device_io 1 --device_jpeg 1 --device_decode 1 writes the three files of the run without --device_decode, byte for byte."""
    vid = V.clip(tmp_path, FRAMES)
    base = ["--device_io", "1", "--device_jpeg", "1"]
    V.run(vid, tmp_path, nets, base, "warm")
    want = V.run(vid, tmp_path, nets, base, "host")
    got = V.run(vid, tmp_path, nets, base + ["--device_decode", "1"], "dev")
    V.same_files(want, got, frames=5)
    assert set(got.res) == KEYS
