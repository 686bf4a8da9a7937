"""The streams of the device Motion-JPEG decoder's tests (test_host_jpeg_decode.py, test_gpu_jpeg_decode.py): each the smallest one
that reaches its branch, built with PIL at test time, plus the five frames of the example video in golden/mjpeg_example_frames.npz.
``reference(name)`` is the restatement's result for a stream, computed once per process."""
import functools
import io
import os

import numpy as np
from PIL import Image

import jpeg_decode_refs as D
import jpeg_refs as J

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FIXTURE_FRAMES = (0, 1, 100, 225, 450)


def colour_image(H, W, seed=0):
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:H, 0:W]
    return np.stack([127 + 100 * np.sin(xx / 7.0 + yy / 5.0), 127 + 120 * np.cos(xx / 3.0 + yy / 11.0),
                     rng.integers(0, 256, (H, W))], -1).clip(0, 255).astype(np.uint8)


def _pil(img, **kw):
    buf = io.BytesIO()
    Image.fromarray(img).save(buf, format="JPEG", **kw)
    return buf.getvalue()


def without_dht(j):
    """The file with its DHT segments cut out."""
    out, p = j[:2], 2
    while True:
        m, n = j[p + 1], int.from_bytes(j[p + 2: p + 4], "big")
        if m != 0xC4:
            out += j[p: p + 2 + n]
        p += 2 + n
        if m == 0xDA:
            return out + j[p:]


@functools.lru_cache(maxsize=None)
def cases():
    """{name: JPEG file}"""
    rs = np.random.RandomState(11)
    noise = lambda h, w: rs.randint(0, 256, (h, w, 3)).astype(np.uint8)       # noqa: E731
    ramp = np.add.outer(np.arange(64) * 2, np.arange(64) * 2).clip(0, 255).astype(np.uint8)
    c = {}
    c["grey_8x8"] = _pil(colour_image(8, 8)[..., 0], quality=90)
    c["grey_1x1"] = _pil(colour_image(1, 1)[..., 2], quality=90)
    c["420_16x16"] = _pil(colour_image(16, 16), quality=90, subsampling=2)
    c["420_17x33"] = _pil(colour_image(17, 33, 1), quality=90, subsampling=2)
    c["420_33x15"] = _pil(colour_image(33, 15, 2), quality=75, subsampling=2)
    c["444_24x40"] = _pil(colour_image(24, 40, 3), quality=90, subsampling=0)
    c["422_24x40"] = _pil(colour_image(24, 40, 3), quality=90, subsampling=1)
    c["422_9x21"] = _pil(colour_image(9, 21, 4), quality=85, subsampling=1)
    c["noise_48x64_q100"] = _pil(noise(48, 64), quality=100, subsampling=2)
    c["ramp_64x64_q5"] = _pil(np.stack([ramp, ramp[::-1], ramp.T], -1), quality=5, subsampling=2)
    c["optimize_29x37"] = _pil(colour_image(29, 37, 5), quality=60, subsampling=2, optimize=True)
    c["no_dht_29x37"] = without_dht(_pil(colour_image(29, 37, 5), quality=60, subsampling=2))
    img = np.ascontiguousarray(colour_image(40, 56, 6)[..., ::-1])
    for r in (1, 3, 8):                                       # the device encoder's own streams (its restatement, pinned byte for byte)
        c["restart_%d" % r] = J.encode(img, 90, r)
    c["restart_pil_3"] = _pil(colour_image(40, 56, 6), quality=90, subsampling=2, restart_marker_blocks=3)
    c["restart_pil_grey_2"] = _pil(colour_image(20, 50, 7)[..., 1], quality=90, restart_marker_blocks=2)
    c["noise_240x320_q95"] = _pil(noise(240, 320), quality=95, subsampling=2)
    with np.load(os.path.join(GOLD, "mjpeg_example_frames.npz")) as g:
        for k in FIXTURE_FRAMES:
            c["video_%d" % k] = g["frame_%d" % k].tobytes()
    return c


@functools.lru_cache(maxsize=None)
def reference(name):
    """(coefficients int16 [blocks,64], L uint8 [H,W], RGB uint8 [H,W,3] or None) of the restatement."""
    coef, g = D.coefficients(cases()[name])
    L, rgb = D.reconstruct(coef, g)
    return coef, L, rgb


def half_scan(j):
    """The file cut off at half its entropy-coded scan, EOI put back."""
    p = 2
    while True:
        m, n = j[p + 1], int.from_bytes(j[p + 2: p + 4], "big")
        p += 2 + n
        if m == 0xDA:
            end = j.index(b"\xff\xd9", p)
            cut = p + (end - p) // 2
            if j[cut - 1] == 0xFF:
                cut -= 1
            return j[:cut] + b"\xff\xd9"
