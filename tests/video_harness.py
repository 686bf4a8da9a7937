"""Shared harness of the tests that drive evaluate.evaluate_ellseg_per_video on a small Motion-JPEG clip built from the eye crops of
the evaluate_real_frames fixture: one clip builder, one runner that records what reaches the two writers, the transfers of the
device-I/O path and the three files a run leaves behind, and the two comparisons."""
import io
import types

import numpy as np
import torch

DEV = "cuda:0"
FOUR_FRAMES = ((0, 1), (0, 1), (2, 3), (2, 3))       # (left eye, right eye) per frame: the clip of test_evaluate_video_end_to_end


def clip(tmp_path, frames=FOUR_FRAMES, progressive_at=None):
    """clip.avi under ``tmp_path``: one 640 x 240 frame per (left, right) pair of eye crops; frame ``progressive_at`` is stored as a
    progressive JPEG, which the device decoder does not take (asserted)."""
    from PIL import Image
    from common import gold
    from egne_amd import evaluate as E
    eyes = gold("evaluate_real_frames")["eyes"]
    vid = tmp_path / "clip.avi"
    w = E.MJPEGWriter(str(vid), 30, (640, 240))
    for k, (left, right) in enumerate(frames):
        bgr = np.stack([np.concatenate([eyes[left], eyes[right]], axis=1)] * 3, axis=2)
        if k == progressive_at:
            buf = io.BytesIO()
            Image.fromarray(bgr).save(buf, format="JPEG", quality=90, progressive=True)
            assert E.jpeg_parse(buf.getvalue()) is None
            w.write_jpeg(buf.getvalue())
        else:
            w.write(bgr)
    w.release()
    return vid


def run(vid, tmp_path, nets, extra, method):
    """evaluate_ellseg_per_video(vid) with ``extra`` flags.  Returns a record: ``res`` (the ellipse dictionary, whose keys the one on
    disk must share), ``written`` [(kind, frame)] handed to MJPEGWriter.write (before JPEG), ``streams`` [(kind, bytes)] handed to
    write_jpeg, ``up`` / ``down`` [(dtype, shape)] of every _upload_u8 / _download, ``files`` (dictionary on disk, result video's bytes,
    edge video's bytes).  The recorders wrap whatever the names hold at the call (a test's own patches included) and are taken off
    again before returning."""
    from egne_amd import evaluate as E
    bd, net = nets
    r = types.SimpleNamespace(written=[], streams=[], up=[], down=[])
    real = (E.MJPEGWriter.write, E.MJPEGWriter.write_jpeg, E._upload_u8, E._download)

    def write(self, frame):
        r.written.append((self.path.rsplit("_", 2)[-2], np.array(frame, copy=True)))
        return real[0](self, frame)

    def write_jpeg(self, data):
        r.streams.append((self.path.rsplit("_", 2)[-2], bytes(data)))
        return real[1](self, data)

    def upload(frames, device):
        t = real[2](frames, device)
        r.up.append((t.dtype, tuple(t.shape)))
        return t

    def download(t):
        r.down.append((t.dtype, tuple(t.shape)))
        return real[3](t)
    E.MJPEGWriter.write, E.MJPEGWriter.write_jpeg, E._upload_u8, E._download = write, write_jpeg, upload, download
    try:
        args = E.parse_args(["--path2data", str(tmp_path), "--method", method] + list(extra))
        r.res = E.evaluate_ellseg_per_video(str(vid), args, net, bd, torch.device(DEV))
    finally:
        E.MJPEGWriter.write, E.MJPEGWriter.write_jpeg, E._upload_u8, E._download = real
    pred = np.load(str(tmp_path / ("clip_pred2_%s.npy" % method)), allow_pickle=True).item()
    assert set(pred) == set(r.res)
    r.files = (pred,) + tuple(open(str(tmp_path / ("clip_%s_%s.avi" % (kind, method))), "rb").read() for kind in ("result", "edge"))
    return r


def same_ellipses(res_a, res_b, equal_nan=False):
    assert set(res_a) == set(res_b)
    for k in res_a:
        for e_a, e_b in zip(res_a[k], res_b[k]):
            assert e_a.shape == (5,) and np.array_equal(e_a, e_b, equal_nan=equal_nan), (k, e_a, e_b)


def same_frames(a, b, frames=4, equal_nan=False):
    """Two runs' ellipse dictionaries are equal, and the frames handed to their writers are the same bytes in the same order."""
    same_ellipses(a.res, b.res, equal_nan)
    assert [w[0] for w in a.written] == [w[0] for w in b.written] and len(a.written) == 2 * frames
    for (kind, fa), (_, fb) in zip(a.written, b.written):
        assert fa.dtype == np.uint8 and fa.shape == fb.shape == (240, 640, 3)
        assert np.array_equal(fa, fb), "%s frame differs in %d bytes" % (kind, np.count_nonzero(fa != fb))


def same_files(a, b, frames=4, equal_nan=False):
    """Two runs wrote the same three files: equal ellipse dictionaries, byte-identical videos."""
    same_ellipses(a.files[0], b.files[0], equal_nan)
    assert a.files[1] == b.files[1], "the result videos differ"
    assert a.files[2] == b.files[2], "the edge videos differ"
    assert len(a.files[1]) > frames * 4096
