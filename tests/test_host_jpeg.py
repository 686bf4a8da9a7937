"""No GPU: the definition of the device Motion-JPEG encoder (evaluate.py --device_jpeg 1) as restated in jpeg_refs.py --
its tables and the product's against what PIL writes, its streams through PIL's decoder, its quality against PIL's own encoder, the
symbols the image set exercises, the frame-number mask against _put_frame_number, the flag."""
import io

import numpy as np
import pytest
from PIL import Image

import jpeg_refs as J

import egne_amd  # noqa: F401
from egne_amd import evaluate as E

R = E.JPEG_RESTART_MCUS
CASES = [(name, q) for name, (_, qs) in J.images(R).items() for q in qs]


def _segments(data):
    """[(marker, body)] of a JPEG file up to and including SOS."""
    assert data[:2] == b"\xff\xd8"
    segs, i = [], 2
    while True:
        assert data[i] == 0xFF
        m, n = data[i + 1], int.from_bytes(data[i + 2: i + 4], "big")
        segs.append((m, data[i + 4: i + 2 + n]))
        i += 2 + n
        if m == 0xDA:
            return segs


def _pil_file(img_bgr, quality):
    buf = io.BytesIO()
    Image.fromarray(np.ascontiguousarray(img_bgr[..., ::-1])).save(buf, format="JPEG", quality=quality)
    return buf.getvalue()


@pytest.mark.parametrize("quality", [50, 90, 100])
def test_tables_equal_what_pil_writes(quality):
    img = J.images(R)["noise"][0]
    pil = _segments(_pil_file(img, quality))
    dqt = [b for m, b in pil if m == 0xDB]
    dht = {b[0]: b[1:] for m, b in pil if m == 0xC4}
    assert [len(b) for b in dqt] == [65, 65] and sorted(len(b) + 3 for b in dht.values()) == [31, 31, 181, 181]
    qt, huff, dct = E.jpeg_tables(quality)
    ours = _segments(E.jpeg_header(56, 40, quality, R))
    for which in (0, 1):
        assert dqt[which] == bytes([which]) + J.dqt_body(quality, which)                 # the restatement
        assert dqt[which] == bytes([which]) + qt[which].tobytes()                        # the product's device table
    assert [b for m, b in ours if m == 0xDB] == dqt                                      # the product's header
    assert {b[0]: b[1:] for m, b in ours if m == 0xC4} == dht
    firsts = {(0, 0): 0, (0, 1): 16, (1, 0): 32, (1, 1): 288}
    for cls, ident in J.DHT_ORDER:
        assert dht[cls << 4 | ident] == J.dht_body(cls, ident)
        table = J.huffman(cls, ident)
        want = np.zeros(16 if cls == 0 else 256, np.uint32)
        for sym, (code, length) in table.items():
            want[sym] = length << 16 | code
        first = firsts[(cls, ident)]
        assert np.array_equal(huff[first: first + want.size], want)
    assert np.array_equal(dct, J.dct_matrix()) and dct.dtype == np.int32
    assert E.jpeg_header(56, 40, quality, R) == J.header(56, 40, quality, R)


def test_header_layout():
    h = E.jpeg_header(640, 240, 90)
    assert [m for m, _ in _segments(h)] == [0xE0, 0xDB, 0xDB, 0xC0, 0xC4, 0xC4, 0xC4, 0xC4, 0xDD, 0xDA]
    segs = dict((m, b) for m, b in _segments(h) if m in (0xC0, 0xDD))
    assert segs[0xC0] == bytes([8, 0, 240, 2, 128, 3, 1, 0x22, 0, 2, 0x11, 1, 3, 0x11, 1])
    assert int.from_bytes(segs[0xDD], "big") == R and 1 <= R <= 8


@pytest.mark.parametrize("name,quality", CASES)
def test_streams_open_in_pil(name, quality):
    img = J.images(R)[name][0]
    stream, _ = J.encoded(name, quality, R)
    im = Image.open(io.BytesIO(stream))
    im.load()
    assert im.size == (img.shape[1], img.shape[0]) and im.mode == "RGB" and im.format == "JPEG"
    assert stream[-2:] == b"\xff\xd9"


@pytest.mark.parametrize("name", list(J.images(R)))
def test_quality_is_pils_within_the_margin(name):
    """PSNR against the source at qualities 50 / 90 / 100: at least PIL's own encoder's minus PSNR_MARGIN_DB (DESIGN.md 6e has the
    table this margin was set from: worst shortfall 0.04 dB -> the floor of 0.1 dB)."""
    img = J.images(R)[name][0]
    for quality in (50, 90, 100):
        stream, _ = J.encoded(name, quality, R)
        mine = J.psnr(np.asarray(Image.open(io.BytesIO(stream)))[..., ::-1], img)
        pil_stream = _pil_file(img, quality)
        pil = J.psnr(np.asarray(Image.open(io.BytesIO(pil_stream)))[..., ::-1], img)
        print("%-14s quality %3d: %6d bytes (PIL %6d), PSNR %7.2f dB (PIL %7.2f), shortfall %+.3f dB"
              % (name, quality, len(stream), len(pil_stream), mine, pil, pil - mine))
        assert mine >= pil - J.PSNR_MARGIN_DB


def test_margin_is_the_floor():
    assert J.PSNR_MARGIN_DB == 0.1


def test_image_set_covers_the_coder():
    total = J.new_histogram()
    for name, quality in CASES:
        h = J.encoded(name, quality, R)[1]
        for k, v in h.items():
            total[k] = [a + b for a, b in zip(total[k], v)] if isinstance(v, list) else total[k] + v
    print(total)
    assert total["zrl"] > 0
    assert total["eob"] > 0 and total["no_eob"] > 0
    assert total["dc_cat"][11] > 0
    assert total["ac_cat"][10] > 0
    assert total["stuffed"] > 0
    assert total["rst_wrapped"] > 0 and all(total["rst"])
    strip = J.images(R)["strip"][0]
    assert strip.shape[0] == 16 and strip.shape[1] // (16 * R) >= 10


@pytest.mark.parametrize("j", [0, 9, 10, 99, 100, 999, 1000, 99999, 999999])
def test_mask_and_blend_equal_put_frame_number(j):
    rs = np.random.RandomState(j % 1000)
    frames = rs.randint(0, 256, (2, 48, 96, 3), dtype=np.uint8)
    want = frames.copy()
    for f in want:
        E._put_frame_number(f, j)
    ph, pw, x0, y0 = E._STAMP_PATCH
    mask = E.frame_number_mask(j, ph, pw, x0, y0)
    assert mask.shape == (ph, pw) and mask.dtype == np.uint8 and mask.any()
    got = J.blend(frames, np.stack([mask, mask]), x0, y0, (0, 0, 255))
    assert np.array_equal(got, want)
    assert not np.array_equal(got, frames)


def test_mask_patch_must_hold_the_number():
    with pytest.raises(AssertionError, match="outside"):
        E.frame_number_mask(999999, 8, 20, 10, 14)
    assert E.frame_number_mask(7).shape == E._STAMP_PATCH[:2]


def test_write_jpeg_appends_the_stream_as_it_is(tmp_path):
    img = J.images(R)["overlay"][0]
    stream, _ = J.encoded("overlay", 90, R)
    w = E.MJPEGWriter(str(tmp_path / "a.avi"), 30, (img.shape[1], img.shape[0]))
    w.write_jpeg(stream)
    w.write(img)
    w.release()
    data = open(str(tmp_path / "a.avi"), "rb").read()
    assert stream in data
    frames = list(E.mjpeg_frames(str(tmp_path / "a.avi")))
    assert len(frames) == 2 and frames[0].shape == img.shape[:2]


def test_flag():
    assert E.parse_args([]).device_jpeg == 0
    a = E.parse_args(["--device_io", "1", "--device_jpeg", "1"])
    assert a.device_jpeg == 1 and a.device_io == 1
    with pytest.raises(SystemExit):
        E.parse_args(["--device_jpeg", "1"])
    with pytest.raises(SystemExit):
        E.parse_args(["--device_io", "0", "--device_jpeg", "1"])
