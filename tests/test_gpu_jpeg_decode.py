"""-m gpu: evaluate.py --device_decode 1 -- the device Motion-JPEG decoder (egne_jpeg_decode) against the restatement in
jpeg_decode_refs.py (which test_host_jpeg_decode.py holds against PIL) on the streams of jpeg_decode_cases.py, in both modes and at
two subsequence lengths; the Python surface; guard bytes; a damaged stream; the video loop with and without the switch."""
import ctypes

import numpy as np
import pytest
import torch

import jpeg_decode_cases as C
import video_harness as V

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FILL, GUARD = 0xA5, 256
NAMES = list(C.cases())


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


def _dev(a):
    return torch.from_numpy(np.array(a, copy=True, order="C")).to(DEV)


def _decode(files, sub_bits=1024, mode=1, H=None, null_desc=False):
    """egne_jpeg_decode through ctypes on files of one geometry; grey_out, coef_out and flags lie between GUARD bytes of FILL.
    Returns (status, grey uint8 [N,H,W], coef int16 [N,blocks,64], flags, stats); asserts the guards."""
    from egne_amd import _lib
    E, L = _E(), _lib.lib()
    infos = [E.jpeg_parse(f) for f in files]
    N, Hh, W, sampling = len(files), infos[0]["H"], infos[0]["W"], infos[0]["sampling"]
    desc = np.stack([i["record"] for i in infos])
    parts, at = [], 0
    for n, (f, i) in enumerate(zip(files, infos)):
        scan = f[i["scan_off"]: i["scan_off"] + i["scan_len"]]
        desc[n, :8].view(np.int32)[:] = (at, len(scan))
        parts.append(scan + b"\0" * (-len(scan) % 4))
        at += len(parts[-1])
    nbytes = max(at, 4)
    streams, d = _dev(np.frombuffer(b"".join(parts).ljust(nbytes, b"\0"), np.uint8)), _dev(desc)
    hs, vs = (2 if sampling >= 2 else 1), (2 if sampling == 3 else 1)
    blocks = -(-Hh // (8 * vs)) * -(-W // (8 * hs)) * (1 if sampling == 0 else hs * vs + 2)
    sizes = (N * Hh * W, N * blocks * 128, N * 4)
    bufs = [torch.full((GUARD + s + GUARD,), FILL, dtype=torch.uint8, device=DEV) for s in sizes]
    stats = torch.full((N, 2), -7, dtype=torch.int32, device=DEV)
    ws = torch.empty(int(L.egne_jpeg_decode_workspace_bytes(N, Hh, W, sampling, nbytes, sub_bits if sub_bits % 32 == 0 else 128, 0)) + 16,
                     dtype=torch.uint8, device=DEV)
    st = L.egne_jpeg_decode(streams.data_ptr(), nbytes, None if null_desc else d.data_ptr(), N, Hh if H is None else H, W, sampling, sub_bits,
                            mode, bufs[0].data_ptr() + GUARD, bufs[1].data_ptr() + GUARD, bufs[2].data_ptr() + GUARD, stats.data_ptr(),
                            ws.data_ptr(), _lib.stream_ptr())
    torch.cuda.synchronize()
    host = [b.cpu().numpy() for b in bufs]
    for h, what in zip(host, ("grey_out", "coef_out", "flags")):
        assert (h[:GUARD] == FILL).all() and (h[-GUARD:] == FILL).all(), "guard bytes around %s were written" % what
    grey = host[0][GUARD:-GUARD].reshape(N, Hh, W)
    coef = host[1][GUARD:-GUARD].view(np.int16).reshape(N, blocks, 64)
    return st, grey, coef, host[2][GUARD:-GUARD].view(np.int32), stats.cpu().numpy()


@pytest.mark.parametrize("name", NAMES)
def test_decoder_equals_the_restatement(name):
    """coef_out and grey_out against the restatement, for mode 0 and 1 and sub_bits 128 and 1024: four identical results."""
    want_coef, want_L, _ = C.reference(name)
    first = None
    for mode in (0, 1):
        for sub_bits in (128, 1024):
            st, grey, coef, flags, stats = _decode([C.cases()[name]], sub_bits, mode)
            print("%s mode %d sub_bits %d: flag %d, rounds %d, ranges %d" % (name, mode, sub_bits, flags[0], stats[0, 0], stats[0, 1]))
            assert st == 0 and flags[0] == 0
            assert coef.shape[1:] == want_coef.shape and np.array_equal(coef[0], want_coef), "coefficients (mode %d, sub_bits %d)" % (mode, sub_bits)
            assert np.array_equal(grey[0], want_L), "grey frame (mode %d, sub_bits %d)" % (mode, sub_bits)
            first = first or (grey.copy(), coef.copy())
            assert np.array_equal(grey, first[0]) and np.array_equal(coef, first[1])
            assert stats[0, 0] == 0 or mode == 1


def test_rounds_and_windows_are_reached():
    """At sub_bits 128 some stream needs more than one synchronisation round, and the 240 x 320 noise fills more than one window of
    256 subsequences (at 1024 bits too); otherwise the multi-round / multi-window paths were not tested above."""
    rounds = {}
    for name in ("noise_48x64_q100", "ramp_64x64_q5", "video_0", "noise_240x320_q95"):
        st, _, _, flags, stats = _decode([C.cases()[name]], 128, 1)
        assert st == 0 and flags[0] == 0
        rounds[name] = tuple(stats[0])
    print(rounds)
    assert max(r for r, _ in rounds.values()) > 1
    assert rounds["noise_240x320_q95"][1] > 256
    st, _, _, flags, stats = _decode([C.cases()["noise_240x320_q95"]], 1024, 1)
    assert st == 0 and flags[0] == 0 and stats[0, 1] > 256
    st, _, _, flags, stats = _decode([C.cases()["restart_3"]], 1024, 0)
    assert st == 0 and tuple(stats[0]) == (0, 4)                 # mode 0: no rounds, one range per segment (12 MCUs / 3)


def test_python_surface_on_the_video_frames(tmp_path):
    E = _E()
    files = [C.cases()["video_%d" % k] for k in C.FIXTURE_FRAMES]
    w = E.MJPEGWriter(str(tmp_path / "v.avi"), 30, (640, 240))
    for f in files:
        w.write_jpeg(f)
    w.release()
    want = list(E.mjpeg_frames(str(tmp_path / "v.avi")))
    assert list(E.mjpeg_chunks(str(tmp_path / "v.avi"))) == files and len(want) == 5
    grey, flags = E.decode_jpeg_device(files, DEV)
    assert grey.dtype == torch.uint8 and tuple(grey.shape) == (5, 240, 640) and flags.dtype == torch.int32 and tuple(flags.shape) == (5,)
    assert grey.is_cuda and not flags.cpu().numpy().any()
    assert np.array_equal(grey.cpu().numpy(), np.stack(want))
    out = torch.zeros((5, 240, 640), dtype=torch.uint8, device=DEV)
    g2, f2 = E.decode_jpeg_device(files, DEV, sub_bits=256, mode=0, out=out)
    assert g2 is out and torch.equal(out, grey) and torch.equal(f2, flags)
    with pytest.raises(ValueError, match="out"):
        E.decode_jpeg_device(files, DEV, out=out[:4])


def test_batch_equals_single_calls_and_runs_are_identical():
    names = ("restart_1", "restart_pil_3", "restart_8")         # three 40 x 56 streams of different lengths and restart intervals
    files = [C.cases()[k] for k in names]
    assert len({len(f) for f in files}) == 3
    st, grey, coef, flags, stats = _decode(files, 128, 1)
    assert st == 0 and not flags.any()
    for n, name in enumerate(names):
        st1, grey1, coef1, flags1, _ = _decode([files[n]], 128, 1)
        assert st1 == 0 and flags1[0] == 0
        assert np.array_equal(grey1[0], grey[n]) and np.array_equal(coef1[0], coef[n])
        assert np.array_equal(grey[n], C.reference(name)[1]) and np.array_equal(coef[n], C.reference(name)[0])
    st2, grey2, coef2, flags2, stats2 = _decode(files, 128, 1)
    assert st2 == 0 and np.array_equal(grey2, grey) and np.array_equal(coef2, coef) and np.array_equal(flags2, flags) and np.array_equal(stats2, stats)


@pytest.mark.parametrize("mode", [0, 1])
def test_half_a_scan_is_flagged_and_its_neighbours_are_right(mode):
    """(The host program of test_host_jpeg_decode.py has walked this stream under the sanitizers.)"""
    files = [C.cases()["video_0"], C.half_scan(C.cases()["video_1"]), C.cases()["video_100"]]
    assert _E().jpeg_parse(files[1]) is not None
    st, grey, coef, flags, _ = _decode(files, 1024, mode)         # (_decode asserts the guards)
    assert st == 0 and list(flags) == [0, 1, 0]
    for n, name in ((0, "video_0"), (2, "video_100")):
        assert np.array_equal(grey[n], C.reference(name)[1]) and np.array_equal(coef[n], C.reference(name)[0])


@pytest.mark.parametrize("kwargs,word", [(dict(sub_bits=100), b"sub_bits"), (dict(H=0), b"shape"), (dict(null_desc=True), b"table")])
def test_bad_arguments(kwargs, word):
    from egne_amd import _lib
    st, grey, coef, flags, stats = _decode([C.cases()["420_16x16"]], **kwargs)
    assert st != 0
    assert word in _lib.lib().egne_last_error()
    assert (grey == FILL).all() and (coef.view(np.uint8) == FILL).all() and (flags.view(np.uint8) == FILL).all() and (stats == -7).all()


# ---- the video loop ---------------------------------------------------------------------------------------------------------------------
def _run(vid, tmp_path, nets, extra, method):
    """The run's record (video_harness.run); the four-frame clip leaves an ellipse pair per frame and per eye."""
    r = V.run(vid, tmp_path, nets, extra, method)
    assert len(r.res) == 4 + 8
    return r


@pytest.mark.parametrize("live", ["0", "1"])
def test_video_end_to_end_equals_the_host_decode(tmp_path, nets, monkeypatch, live):
    """--device_io 1 --device_jpeg 1 --device_decode 1 writes the same three files, byte for byte, as the run without --device_decode
    (after a warm-up run); the decoded frames never exist on the host, and PIL's decoder is not called."""
    E = _E()
    vid = V.clip(tmp_path)
    base = ["--low_latency", live, "--device_io", "1", "--device_jpeg", "1"]
    _run(vid, tmp_path, nets, base, "warm")
    want = _run(vid, tmp_path, nets, base, "host")
    calls, ups = [], []
    real_host, real_up = E._decode_host, E._upload_u8
    monkeypatch.setattr(E, "_decode_host", lambda data: calls.append(1) or real_host(data))
    monkeypatch.setattr(E, "_upload_u8", lambda frames, device: ups.append(1) or real_up(frames, device))
    monkeypatch.setattr(E, "mjpeg_frames", lambda path: (_ for _ in ()).throw(AssertionError("the host decoder ran")))
    real_dec, sizes = E.decode_jpeg_device, []
    monkeypatch.setattr(E, "decode_jpeg_device", lambda datas, *a, **kw: sizes.append(len(datas)) or real_dec(datas, *a, **kw))
    got = _run(vid, tmp_path, nets, base + ["--device_decode", "1"], "dev")
    monkeypatch.undo()
    V.same_files(want, got)
    assert not calls and not ups
    assert sizes == ([1] * 4 if live == "1" else [4])           # one decode per frame pair in the live loop, one per batch otherwise


@pytest.mark.parametrize("live", ["0", "1"])
def test_video_without_device_jpeg(tmp_path, nets, live):
    """--device_io 1 --device_decode 1 alone (PIL encodes the output): the same three files as --device_io 1."""
    E = _E()
    vid = V.clip(tmp_path)
    base = ["--low_latency", live, "--device_io", "1"]
    _run(vid, tmp_path, nets, base, "warm")
    V.same_files(_run(vid, tmp_path, nets, base, "host"), _run(vid, tmp_path, nets, base + ["--device_decode", "1"], "dev"))


@pytest.mark.parametrize("live", ["0", "1"])
def test_video_with_a_progressive_frame_and_a_flagged_one(tmp_path, nets, monkeypatch, live):
    """A progressive frame spliced into the video takes the host path; a frame whose flag comes back non-zero (here: forced, and its
    decoded row overwritten) is decoded by PIL at draw time and its batch is done again: the files are still the host decode's."""
    E = _E()
    vid = V.clip(tmp_path, progressive_at=1)
    base = ["--low_latency", live, "--device_io", "1", "--device_jpeg", "1"]
    _run(vid, tmp_path, nets, base, "warm")
    want = _run(vid, tmp_path, nets, base, "host")
    calls = []
    real_host = E._decode_host
    monkeypatch.setattr(E, "_decode_host", lambda data: calls.append(1) or real_host(data))
    got = _run(vid, tmp_path, nets, base + ["--device_decode", "1"], "dev")
    V.same_files(want, got)
    assert len(calls) == 1                                     # the progressive frame, once
    real_dec, flagged = E.decode_jpeg_device, []

    def spoiled(datas, *a, **kw):
        grey, flags = real_dec(datas, *a, **kw)
        if not flagged:                                          # the first device frame of the video: flag it, and spoil its row
            flagged.append(1)
            flags[0] = 1
            grey[0] = 77
        return grey, flags
    monkeypatch.setattr(E, "decode_jpeg_device", spoiled)
    del calls[:]
    got = _run(vid, tmp_path, nets, base + ["--device_decode", "1"], "flag")
    V.same_files(want, got)
    assert flagged and len(calls) == 2                           # the progressive frame and the flagged one


@pytest.mark.parametrize("live", ["0", "1"])
def test_video_redo_after_a_reported_overflow(tmp_path, nets, monkeypatch, live):
    """The re-calibration path with the decode in front: the first overflow query answers "overflowed", the batch is done again from
    the decoded device frames -- same files."""
    E = _E()
    vid = V.clip(tmp_path)
    extra = ["--low_latency", live, "--device_io", "1", "--device_jpeg", "1", "--device_decode", "1"]
    _run(vid, tmp_path, nets, extra, "warm")
    want = _run(vid, tmp_path, nets, extra, "dev")
    real, calls = E._overflowed, []

    def once(net):
        calls.append(1)
        return True if len(calls) == 1 else real(net)
    monkeypatch.setattr(E, "_overflowed", once)
    got = _run(vid, tmp_path, nets, extra, "redo")
    assert len(calls) > 2
    V.same_files(want, got)


def test_video_frame_nobody_decodes_names_the_frame(tmp_path, nets, monkeypatch):
    E = _E()
    vid = V.clip(tmp_path)
    real_dec = E.decode_jpeg_device

    def flag_all(datas, *a, **kw):
        grey, flags = real_dec(datas, *a, **kw)
        flags[:] = 1
        return grey, flags
    monkeypatch.setattr(E, "decode_jpeg_device", flag_all)
    monkeypatch.setattr(E, "_decode_host", lambda data: None)
    with pytest.raises(SystemExit, match=r"frame 0 .*--device_decode 0"):
        _run(vid, tmp_path, nets, ["--device_io", "1", "--device_decode", "1"], "none")
