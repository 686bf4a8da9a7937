"""-m gpu: evaluate.py --device_jpeg 1 -- the device Motion-JPEG encoder (egne_jpeg_encode) and the frame-number stamp (egne_stamp_mask),
pinned byte for byte against the restatement in jpeg_refs.py (whose tables and quality test_host_jpeg.py holds against PIL), and the
video loop with both against --device_io 1."""
import ctypes

import numpy as np
import pytest
import torch

import jpeg_refs as J
import video_harness as V

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FILL = 0xA5


@pytest.fixture(autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


@pytest.fixture(scope="module")
def nets():
    from common import bdcn_module, esf_module
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    dev = torch.device(DEV)
    return bdcn_module().to(dev), esf_module("baseline_edge").to(dev).eval()


def _E():
    from egne_amd import evaluate as E
    return E


def _R():
    return _E().JPEG_RESTART_MCUS


def _dev(a):
    return torch.from_numpy(np.array(a, copy=True, order="C")).to(DEV)


def _encode(imgs, quality, cap, guard=256, restart=None, H=None, null=None):
    """egne_jpeg_encode through ctypes on a stack of equally sized images; the output buffer (N*cap + guard bytes) is pre-filled with
    FILL.  Returns (status, buffer uint8 [N*cap + guard], lengths, flags)."""
    from egne_amd import _lib
    E, L = _E(), _lib.lib()
    frames = _dev(np.stack(imgs))
    N, Hh, W = frames.shape[:3]
    restart = _R() if restart is None else restart
    tabs = [_dev(a) for a in E.jpeg_tables(quality)]
    header = E.jpeg_header(W, Hh, quality, max(restart, 1))
    hd = _dev(np.frombuffer(header, np.uint8))
    out = torch.full((N * cap + guard,), FILL, dtype=torch.uint8, device=DEV)
    lengths = torch.full((N,), -7, dtype=torch.int32, device=DEV)
    flags = torch.full((N,), -7, dtype=torch.int32, device=DEV)
    ws = torch.empty(int(L.egne_jpeg_workspace_bytes(N, Hh, W)), dtype=torch.uint8, device=DEV)
    ptrs = [t.data_ptr() for t in tabs]
    if null is not None:
        ptrs[null] = None
    st = L.egne_jpeg_encode(frames.data_ptr(), N, Hh if H is None else H, W, ptrs[0], ptrs[1], ptrs[2], hd.data_ptr(), len(header), restart,
                            out.data_ptr(), ctypes.c_int64(cap), lengths.data_ptr(), flags.data_ptr(), ws.data_ptr(), _lib.stream_ptr())
    torch.cuda.synchronize()
    return st, out.cpu().numpy(), lengths.cpu().numpy(), flags.cpu().numpy()


def _default_cap(img, quality):
    H, W = img.shape[:2]
    return len(_E().jpeg_header(W, H, quality)) + (-(-H // 16) * 16) * (-(-W // 16) * 16) * 3 // 2


def _check_frame(buf, cap, n, length, want, what):
    got = buf[n * cap: n * cap + length].tobytes()
    assert length == len(want), "%s: length %d, restatement %d" % (what, length, len(want))
    if got != want:
        first = next(i for i in range(len(want)) if got[i] != want[i])
        raise AssertionError("%s: first difference at byte %d of %d" % (what, first, len(want)))
    assert (buf[n * cap + length: (n + 1) * cap] == FILL).all(), "%s: bytes written behind the file inside its slot" % what


CASES = [(name, q) for name in ("one_mcu", "odd_size", "noise", "flat", "grey", "overlay", "extremes", "strip", "real_plain", "real_rendered")
         for q in ((50, 90, 100) if name in ("noise", "extremes", "odd_size") else (90,))]


@pytest.mark.parametrize("name,quality", CASES)
def test_encoder_equals_the_restatement(name, quality):
    R = _R()
    img, qualities = J.images(R)[name]
    assert quality in qualities
    want, _ = J.encoded(name, quality, R)
    cap = max(_default_cap(img, quality), len(want) + 16)      # (noise at quality 100 is longer than the Python surface's default slot)
    st, buf, lengths, flags = _encode([img], quality, cap)
    assert st == 0
    print("%s quality %d: %d bytes (cap %d), flag %d" % (name, quality, lengths[0], cap, flags[0]))
    assert flags[0] == 0
    _check_frame(buf, cap, 0, int(lengths[0]), want, "%s q%d" % (name, quality))
    assert (buf[cap:] == FILL).all()


def test_python_surface_on_the_real_pair():
    E, R = _E(), _R()
    a, b = J.images(R)["real_plain"][0], J.images(R)["real_rendered"][0]
    out, lengths, flags = E.encode_jpeg_device(_dev(np.stack([a, b])))
    assert out.dtype == torch.uint8 and lengths.dtype == torch.int32 and flags.dtype == torch.int32
    assert tuple(out.shape) == (2, _default_cap(a, 90)) and tuple(lengths.shape) == (2,) and tuple(flags.shape) == (2,)
    out, lengths, flags = out.cpu().numpy(), lengths.cpu().numpy(), flags.cpu().numpy()
    for n, name in enumerate(("real_plain", "real_rendered")):
        assert flags[n] == 0 and out[n, :lengths[n]].tobytes() == J.encoded(name, 90, R)[0]
    with pytest.raises(ValueError, match="uint8"):
        E.encode_jpeg_device(_dev(a))
    with pytest.raises((ValueError, RuntimeError), match="CUDA"):
        E.encode_jpeg_device(torch.from_numpy(a[None]))


def test_batch_equals_single_calls_and_runs_are_identical():
    R = _R()
    names = ("noise", "overlay", "grey")                     # three different 40 x 56 images
    imgs = [J.images(R)[k][0] for k in names]
    cap = _default_cap(imgs[0], 90)
    st, buf, lengths, flags = _encode(imgs, 90, cap)
    assert st == 0 and not flags.any()
    for n, name in enumerate(names):
        st1, buf1, len1, flag1 = _encode([imgs[n]], 90, cap)
        assert st1 == 0 and flag1[0] == 0 and len1[0] == lengths[n]
        assert np.array_equal(buf1[:cap], buf[n * cap: (n + 1) * cap])
        _check_frame(buf, cap, n, int(lengths[n]), J.encoded(name, 90, R)[0], name)
    st2, buf2, lengths2, flags2 = _encode(imgs, 90, cap)
    assert st2 == 0 and np.array_equal(buf2, buf) and np.array_equal(lengths2, lengths) and np.array_equal(flags2, flags)


def test_capacity():
    R = _R()
    names = ("overlay", "noise", "grey")                     # the middle frame is the longest
    imgs = [J.images(R)[k][0] for k in names]
    want = [J.encoded(k, 90, R)[0] for k in names]
    assert len(want[1]) > len(want[0]) + 256 and len(want[1]) > len(want[2]) + 256
    cap = len(want[1]) - 1
    st, buf, lengths, flags = _encode(imgs, 90, cap)
    assert st == 0
    assert list(flags) == [0, 1, 0] and lengths[1] == 0
    for n in (0, 2):                                         # intact, and nothing behind them: the 256 bytes behind a slot included
        _check_frame(buf, cap, n, int(lengths[n]), want[n], names[n])
    assert (buf[2 * cap - 256: 2 * cap] == FILL).all()       # the last 256 bytes of the slot that overflowed ...
    assert (buf[3 * cap:] == FILL).all() and buf[3 * cap:].size == 256       # ... and the guard behind the last slot
    cap = len(want[1])                                       # exact
    st, buf, lengths, flags = _encode(imgs, 90, cap)
    assert st == 0 and not flags.any()
    for n in range(3):
        _check_frame(buf, cap, n, int(lengths[n]), want[n], names[n])
    assert (buf[3 * cap:] == FILL).all()
    for n in range(3):                                       # every frame alone in a slot of exactly its size, 256 guard bytes behind it
        st, buf, lengths, flags = _encode([imgs[n]], 90, len(want[n]))
        assert st == 0 and flags[0] == 0 and buf[:len(want[n])].tobytes() == want[n] and (buf[len(want[n]):] == FILL).all()
        st, buf, lengths, flags = _encode([imgs[n]], 90, len(want[n]) - 1)
        assert st == 0 and flags[0] == 1 and lengths[0] == 0 and (buf[len(want[n]) - 1:] == FILL).all()


@pytest.mark.parametrize("kwargs,word", [(dict(H=0), b"shape"), (dict(restart=0), b"restart_mcus"), (dict(null=1), b"table")])
def test_bad_arguments(kwargs, word):
    from egne_amd import _lib
    img = J.images(_R())["one_mcu"][0]
    st, buf, lengths, flags = _encode([img], 90, 2048, **kwargs)
    assert st != 0
    assert word in _lib.lib().egne_last_error()
    assert (buf == FILL).all() and lengths[0] == -7 and flags[0] == -7        # nothing ran


def test_stamp_mask_equals_the_host_blend():
    from egne_amd import _lib
    L = _lib.lib()
    rs = np.random.RandomState(3)
    frames = rs.randint(0, 256, (2, 20, 30, 3), dtype=np.uint8)
    mask = rs.randint(0, 256, (2, 12, 16), dtype=np.uint8)
    mask[0, :2] = 0
    mask[1, -2:] = 255
    for x0, y0 in ((3, 2), (20, 12), (-5, -4), (14, 8), (40, 5), (0, 20)):       # inside; clipped right + bottom; left + top; exact fit; outside
        d = _dev(frames)
        st = L.egne_stamp_mask(d.data_ptr(), 2, 20, 30, _dev(mask).data_ptr(), 12, 16, x0, y0, 0, 0, 255, _lib.stream_ptr())
        torch.cuda.synchronize()
        assert st == 0
        want = J.blend(frames, mask, x0, y0, (0, 0, 255))
        assert np.array_equal(d.cpu().numpy(), want), (x0, y0)
        assert (x0, y0) in ((40, 5), (0, 20)) or not np.array_equal(want, frames)
    d = _dev(frames)
    st = L.egne_stamp_mask(d.data_ptr(), 2, 20, 30, _dev(mask).data_ptr(), 12, 16, 5, 4, 10, 200, 77, _lib.stream_ptr())
    torch.cuda.synchronize()
    assert st == 0 and np.array_equal(d.cpu().numpy(), J.blend(frames, mask, 5, 4, (10, 200, 77)))
    assert L.egne_stamp_mask(d.data_ptr(), 2, 20, 30, None, 12, 16, 5, 4, 0, 0, 255, None) != 0
    assert L.egne_stamp_mask(d.data_ptr(), 2, 20, 30, _dev(mask).data_ptr(), 12, 16, 5, 4, 0, 0, 256, None) != 0
    assert b"ink" in L.egne_last_error()


def test_stamp_numbers_equals_put_frame_number():
    E = _E()
    frames = np.stack([J.images(_R())["real_rendered"][0], J.images(_R())["real_plain"][0]])
    want = frames.copy()
    for f, j in zip(want, (7, 123456)):
        E._put_frame_number(f, j)
    got = E.stamp_numbers_device(_dev(frames), (7, 123456)).cpu().numpy()
    assert np.array_equal(got, want) and not np.array_equal(got, frames)


@pytest.mark.parametrize("live", ["0", "1"])
def test_video_end_to_end_equals_device_io(tmp_path, nets, live):
    """The clip of test_gpu_evalio with --device_io 1 --device_jpeg 1 against --device_io 1 after a warm-up run: equal ellipse
    dictionaries; every stream handed to write_jpeg is the restatement's encoding of the frame (frame number included) that the
    --device_io 1 run handed to write at the same position; only stream bytes, lengths / flags and ellipses come down."""
    E, R = _E(), _R()
    vid = V.clip(tmp_path)
    base = ["--low_latency", live, "--device_io", "1"]
    V.run(vid, tmp_path, nets, base, "warm")
    dev = V.run(vid, tmp_path, nets, base, "dev")
    jpg = V.run(vid, tmp_path, nets, base + ["--device_jpeg", "1"], "jpg")
    V.same_ellipses(dev.res, jpg.res)
    wr0, st0, wr1, st1, down1 = dev.written, dev.streams, jpg.written, jpg.streams, jpg.down
    assert len(wr0) == 8 and not st0 and not wr1
    assert [k for k, _ in st1] == [k for k, _ in wr0] and sorted(k for k, _ in st1) == ["edge"] * 4 + ["result"] * 4
    for pos, ((kind, frame), (_, stream)) in enumerate(zip(wr0, st1)):
        want = J.encode(frame, 90, R)
        assert stream == want, "%s frame at position %d: %d bytes, restatement %d" % (kind, pos, len(stream), len(want))
    for kind in ("result", "edge"):
        frames = list(E.mjpeg_frames(str(tmp_path / ("clip_%s_jpg.avi" % kind))))
        assert len(frames) == 4 and all(f.shape == (240, 640) for f in frames)
    assert not [d for d in down1 if d[0] == torch.uint8 and len(d[1]) == 4]
    u8 = [int(np.prod(d[1])) for d in down1 if d[0] == torch.uint8]
    per_batch = 1 if live == "1" else 4
    assert len(u8) == 4 // per_batch
    for b, nbytes in enumerate(u8):
        used = sum(len(s) for _, s in st1[2 * per_batch * b: 2 * per_batch * (b + 1)])
        print("batch %d: %d uint8 bytes down, streams %d" % (b, nbytes, used))
        assert nbytes <= used + 4096
    assert [d for d in down1 if d[0] == torch.float64] == [(torch.float64, (2 * per_batch, 2, 5))] * (4 // per_batch)


@pytest.mark.parametrize("live", ["0", "1"])
def test_video_redo_after_a_reported_overflow(tmp_path, nets, monkeypatch, live):
    """The re-calibration path with --device_jpeg 1: the first overflow query answers "overflowed", the batch is rendered again and
    therefore encoded again -- same streams."""
    E = _E()
    vid = V.clip(tmp_path)
    extra = ["--low_latency", live, "--device_io", "1", "--device_jpeg", "1"]
    want = V.run(vid, tmp_path, nets, extra, "jpg")
    real, calls = E._overflowed, []

    def once(net):
        calls.append(1)
        return True if len(calls) == 1 else real(net)
    monkeypatch.setattr(E, "_overflowed", once)
    got = V.run(vid, tmp_path, nets, extra, "redo")
    assert len(calls) > 2 and not want.written and not got.written
    assert len(want.streams) == 8 and want.streams == got.streams
    V.same_ellipses(want.res, got.res)


def test_video_frames_that_do_not_fit_take_the_host_path(tmp_path, nets, monkeypatch):
    """Slots of the median stream length: the longer streams are flagged, their frames come down and go through _put_frame_number and
    write -- the very frames the --device_io 1 run writes --, the others still arrive encoded."""
    E, R = _E(), _R()
    vid = V.clip(tmp_path)
    base = ["--low_latency", "0", "--device_io", "1"]
    wr0 = V.run(vid, tmp_path, nets, base, "dev").written
    st1 = V.run(vid, tmp_path, nets, base + ["--device_jpeg", "1"], "jpg").streams
    sizes = sorted(len(s) for _, s in st1)
    cap = sizes[3]
    real = E.encode_jpeg_device
    monkeypatch.setattr(E, "encode_jpeg_device", lambda frames, quality=90, cap_=None: real(frames, quality, cap))
    cap_run = V.run(vid, tmp_path, nets, base + ["--device_jpeg", "1"], "cap")
    wr2, st2, down2 = cap_run.written, cap_run.streams, cap_run.down
    fits = [len(s) <= cap for _, s in st1]
    assert 0 < sum(fits) < 8 and len(wr2) == 8 - sum(fits) and len(st2) == sum(fits)
    assert [s for (_, s), ok in zip(st1, fits) if ok] == [s for _, s in st2]
    for (kind, frame), (kind2, frame2) in zip([w for w, ok in zip(wr0, fits) if not ok], wr2):
        assert kind == kind2 and np.array_equal(frame, frame2)
    assert sorted(d[1] for d in down2 if d[0] == torch.uint8 and len(d[1]) == 3) == [(240, 640, 3)] * len(wr2)
    frames = list(E.mjpeg_frames(str(tmp_path / "clip_result_cap.avi")))
    assert len(frames) == 4 and all(f.shape == (240, 640) for f in frames)
