"""-m gpu: train.py and test.py with --device_loader 1 (raw samples from the Dataset, every batch prepared by
egne_amd.loader.device_batch) end to end on synthetic raw frames."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def test_train_py_device_loader(tmp_path, monkeypatch, capsys):
    """One epoch: training batches augmented on the device, validation batches not; the epoch ends with a finite validation loss, a
    checkpoint and finite weights."""
    monkeypatch.chdir(tmp_path)
    from egne_amd import loader
    from egne_amd import train as TR
    seen = []
    orig = loader.device_batch

    def spy(raw, *a, **k):
        seen.append(bool(k.get("augment")))
        return orig(raw, *a, **k)
    monkeypatch.setattr(loader, "device_batch", spy)
    np.random.seed(3)
    m = TR.main(["--synthetic", "8", "--batchsize", "4", "--epochs", "1", "--setting", "configs/baseline_edge.yaml", "--device_loader", "1",
                 "--expname", "dl"])
    assert seen == [True, True, False], "two augmented training batches, one plain validation batch: %s" % seen
    text = capsys.readouterr().out
    line = [ln for ln in text.splitlines() if ln.startswith("Epoch 0 done")]
    assert line, text[-2000:]
    vloss = float(line[0].split("valid loss")[1].split()[0])
    assert np.isfinite(vloss)
    assert os.path.exists(os.path.join("logs", "ritnet_v2", "dl", "weights", "ritnet_v2_0.pkl"))
    bad = [k for k, v in m.state_dict().items() if v.dtype.is_floating_point and not torch.isfinite(v).all()]
    assert not bad, bad[:5]


def test_test_py_device_loader(capsys):
    from egne_amd import test as T
    miou, pd, idist, loss = T.main(["--synthetic", "4", "--batchsize", "2", "--setting", "configs/baseline_edge.yaml", "--device_loader", "1"])
    assert np.isfinite(miou) and 0 <= miou <= 1 and np.isfinite(loss)
    assert "mIoU" in capsys.readouterr().out
