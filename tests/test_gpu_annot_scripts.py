"""-m gpu: make_archive end to end on a Motion-JPEG .avi plus seeded annotation files, in both --store modes, and train.py on either
archive.  train.py runs in one child process per archive, each with its own time limit; the two print the same loss lines, because
the labels painted per batch are the labels the tool stored."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import annot_refs as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CHILD = """
import random
import sys
sys.path.insert(0, {root!r})
import numpy as np
import egne_amd
from egne_amd import train as S
np.random.seed(3)
random.seed(3)
S.main({argv!r})
"""


@pytest.fixture(autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


@pytest.fixture(scope="module")
def archives(tmp_path_factory):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from egne_amd import make_archive
    from egne_amd.evaluate import MJPEGWriter
    tmp = tmp_path_factory.mktemp("annot_scripts")
    n, every = 12, 3
    ball, iris, pupil, lid = R.seeded_annotations(n, 70)
    ball[5, 0] = -2.0           # frame 5 (count 6, a candidate) is rejected: its radius is negative
    frames = R.seeded_frames(n, 480, 640, 71)
    video = str(tmp / "clip.avi")
    w = MJPEGWriter(video, 25, (640, 480))
    for f in frames:
        w.write(np.repeat(f[..., None], 3, axis=2))
    w.release()
    R.write_annotation_files(video, ball, iris, pupil, lid, lead_rows=1)          # the NvGaze layout: frame k reads row k + 1
    outs = {}
    for store in ("masks", "annotations"):
        path = str(tmp / (store + ".npz"))
        outs[store] = (path, make_archive.main(["--frames", video, "--annotations", video, "--out", path, "--every", str(every), "--row_offset", "1",
                                                "--canvas", "480x640", "--store", store, "--batch", "2"]))
    return tmp, outs, (ball, iris, pupil, lid)


def test_make_archive_both_stores(archives):
    from egne_amd import dataprep, loader
    tmp, outs, (ball, iris, pupil, lid) = archives
    kept = [2, 8, 11]           # counts 3, 6, 9, 12 are candidates; count 6 is rejected
    with np.load(outs["masks"][0]) as z:
        m = {k: z[k] for k in z.files}
    assert set(m) == {"Images", "Masks", "Masks_noSkin", "pupil_loc", "Fits_pupil", "Fits_iris", "Fits_ball", "Info", "resolution"}
    assert list(m["Info"]) == ["3", "9", "12"] and m["Images"].shape == (3, 480, 640) and m["Images"].dtype == np.uint8
    assert np.array_equal(m["resolution"], np.tile([480, 640], (3, 1)))
    rec = R.pack(ball[kept], iris[kept], pupil[kept], lid[kept])
    noskin, skin, status = R.paint(rec, 480, 640)
    assert np.array_equal(m["Masks_noSkin"], noskin) and np.array_equal(m["Masks"], skin) and not status.any()
    loc, fp, fi = dataprep.annotation_fits(iris[kept], pupil[kept])
    assert np.array_equal(m["pupil_loc"], loc) and np.array_equal(m["Fits_pupil"], fp) and np.array_equal(m["Fits_iris"], fi)
    assert np.array_equal(m["Fits_ball"][:, :3], ball[kept][:, [1, 2, 0]])
    with np.load(outs["annotations"][0]) as z:
        a = {k: z[k] for k in z.files}
    assert set(a) == {"Images", "ann_ball", "ann_iris", "ann_pupil", "ann_lid", "Info", "resolution"}
    assert np.array_equal(a["Images"], m["Images"]) and np.array_equal(a["ann_lid"], lid[kept]) and np.array_equal(a["ann_iris"], iris[kept])
    raw = loader.RawArchive(outs["masks"][0])
    assert len(raw) == 3 and np.array_equal(raw[1][1], noskin[1])
    assert isinstance(loader.open_archive(outs["masks"][0]), loader.RawArchive)
    assert isinstance(loader.open_archive(outs["annotations"][0]), loader.AnnotationArchive)


def test_train_py_on_either_archive(archives):
    tmp, outs, _ = archives
    from egne_amd import synth
    from egne_amd.bdcn_new import BDCN
    bd = BDCN()
    torch.save({"a": synth.seeded_state_dict(bd.state_dict(), kind="bdcn")}, str(tmp / "gen_00000016.pt"))
    lines = {}
    for store in ("masks", "annotations"):
        argv = ["--device_loader", "1", "--raw_archive", outs[store][0], "--loader_size", "480x640", "--loader_scale", "0.5", "--epochs", "1",
                "--batchsize", "2", "--overfit", "1", "--setting", "configs/baseline_edge.yaml", "--expname", store]
        p = subprocess.run([sys.executable, "-c", CHILD.format(root=ROOT, argv=argv)], cwd=str(tmp), stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                           timeout=600)
        out = p.stdout.decode(errors="replace")
        assert p.returncode == 0, out[-3000:]
        done = re.findall(r"valid loss (\S+) mIoU (\S+)", out)
        assert len(done) == 1 and np.isfinite(float(done[0][0])), out[-2000:]
        lines[store] = [re.sub(r"done in \S+s", "done", ln).split(", edge")[0] for ln in out.splitlines() if "oss" in ln and ln.startswith("Epoch")]
    assert lines["masks"] and lines["masks"] == lines["annotations"], lines


def test_a_non_mjpeg_file_is_refused(tmp_path):
    from egne_amd import make_archive
    ball, iris, pupil, lid = R.seeded_annotations(2, 1)
    video = tmp_path / "clip.avi"
    video.write_bytes(b"RIFF\0\0\0\0AVI LIST\0\0\0\0hdrlstrh\0\0\0\0vidsH264" + b"\0" * 64)
    R.write_annotation_files(str(video), ball, iris, pupil, lid)
    with pytest.raises(SystemExit, match="not a Motion-JPEG"):
        make_archive.main(["--frames", str(video), "--annotations", str(video), "--out", str(tmp_path / "x.npz")])
    other = tmp_path / "clip.mp4"
    other.write_bytes(b"\0\0\0\x18ftypmp42" + b"\0" * 64)
    with pytest.raises(SystemExit, match="not a Motion-JPEG"):
        make_archive.main(["--frames", str(other), "--annotations", str(video), "--out", str(tmp_path / "x.npz")])
