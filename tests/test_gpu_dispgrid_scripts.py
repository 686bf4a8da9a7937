"""-m gpu: test.py and train.py --disp 1 end to end on synthetic frames.  Each script runs in ONE child process with its own time limit:
the child runs the script's main() at --disp 0 and then at --disp 1, so that the printed lines of the two runs can be compared."""
import os
import re
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MARK = "=====DISP-ON====="

CHILD = """
import sys
sys.path.insert(0, {root!r})
import egne_amd
from egne_amd import {module} as S
base = {argv!r}
S.main(base + ["--disp", "0"] + {off!r})
print({mark!r}, flush=True)
S.main(base + ["--disp", "1"] + {on!r})
"""


@pytest.fixture(autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _child(tmp_path, module, argv, off, on, limit):
    code = CHILD.format(root=ROOT, module=module, argv=argv, off=off, on=on, mark=MARK)
    p = subprocess.run([sys.executable, "-c", code], cwd=str(tmp_path), stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=limit)
    out = p.stdout.decode(errors="replace")
    assert p.returncode == 0, out[-3000:]
    before, _, after = out.partition(MARK)
    return before, after


def _jpeg_size(path):
    from PIL import Image
    im = Image.open(path)
    im.load()
    assert im.format == "JPEG" and im.mode == "RGB"
    return im.size


def test_test_py_disp(tmp_path):
    """8 synthetic frames in batches of 4: two JPEG files of 244 x 1290 (four 240 x 320 frames side by side), and the printed metric
    lines are those of the run without them."""
    off, on = _child(tmp_path, "test", ["--synthetic", "8", "--batchsize", "4", "--setting", "configs/baseline_edge.yaml"], [], [], 900)
    lines = lambda s: [l for l in s.splitlines() if l.startswith(("mIoU", "Latent", "Segmentation"))]      # noqa: E731
    assert len(lines(off)) == 5 and lines(off) == lines(on), (lines(off), lines(on))
    d = os.path.join(str(tmp_path), "img", "synthetic_baseline_disp")
    assert sorted(os.listdir(d)) == ["batch_00000.jpg", "batch_00001.jpg"]
    for f in os.listdir(d):
        assert _jpeg_size(os.path.join(d, f)) == (1290, 244)
    with open(os.path.join(d, "batch_00000.jpg"), "rb") as a, open(os.path.join(d, "batch_00001.jpg"), "rb") as b:
        assert a.read() != b.read()             # two batches, two pictures


def test_train_py_disp(tmp_path):
    """One epoch of two steps: disp/epoch_000.jpg is written, only under --disp 1, and the epoch's printed validation loss is that of
    the run without it."""
    base = ["--synthetic", "8", "--batchsize", "4", "--epochs", "1", "--setting", "configs/baseline_edge.yaml"]
    off, on = _child(tmp_path, "train", base, ["--expname", "d0"], ["--expname", "d1"], 900)
    done = lambda s: re.findall(r"valid loss (\S+) mIoU (\S+)", s)      # noqa: E731
    assert len(done(off)) == 1 and done(off) == done(on), (done(off), done(on))
    logs = os.path.join(str(tmp_path), "logs", "ritnet_v2")
    assert not os.path.exists(os.path.join(logs, "d0", "disp"))
    assert os.listdir(os.path.join(logs, "d1", "disp")) == ["epoch_000.jpg"]
    assert _jpeg_size(os.path.join(logs, "d1", "disp", "epoch_000.jpg")) == (1290, 244)
