"""Shared by test_host_jpeg.py and test_gpu_jpeg.py: a NumPy / pure-Python restatement of the integer baseline-JPEG definition that
csrc/jpeg.hip implements, with its own copy of the ITU-T T.81 Annex K tables (parsed from the DQT / DHT segment
bodies as the standard lays them out), a histogram of the symbols it emitted, the test images, and the host blend of the frame number.
Nothing here imports the product's tables: the product (evaluate.jpeg_tables / jpeg_header) is compared against this and against PIL."""
import functools

import numpy as np

# ---- Annex K, as segment bodies: DQT = 64 divisors in zigzag order (tables K.1 / K.2), DHT = 16 counts + the symbols (K.3 - K.6) ----------
_DQT_HEX = (
    "100b0c0e0c0a100e0d0e1211101318281a181616183123251d283a333d3c3933383740485c4e404457453738506d51575f626768673e4d71797064785c656763",
    "1112121815182f1a1a2f634238426363636363636363636363636363636363636363636363636363636363636363636363636363636363636363636363636363",
)
_DHT_HEX = {   # (class, id) -> counts[16] + symbols
    (0, 0): "00010501010101010100000000000000000102030405060708090a0b",
    (1, 0): "0002010303020403050504040000017d01020300041105122131410613516107227114328191a1082342b1c11552d1f02433627282090a161718191a25262728"
            "292a3435363738393a434445464748494a535455565758595a636465666768696a737475767778797a838485868788898a92939495969798999aa2a3a4a5a6a7"
            "a8a9aab2b3b4b5b6b7b8b9bac2c3c4c5c6c7c8c9cad2d3d4d5d6d7d8d9dae1e2e3e4e5e6e7e8e9eaf1f2f3f4f5f6f7f8f9fa",
    (0, 1): "00030101010101010101010000000000000102030405060708090a0b",
    (1, 1): "00020102040403040705040400010277000102031104052131061241510761711322328108144291a1b1c109233352f0156272d10a162434e125f11718191a26"
            "2728292a35363738393a434445464748494a535455565758595a636465666768696a737475767778797a82838485868788898a92939495969798999aa2a3a4a5"
            "a6a7a8a9aab2b3b4b5b6b7b8b9bac2c3c4c5c6c7c8c9cad2d3d4d5d6d7d8d9dae2e3e4e5e6e7e8e9eaf2f3f4f5f6f7f8f9fa",
}
DHT_ORDER = ((0, 0), (1, 0), (0, 1), (1, 1))          # DC luminance, AC luminance, DC chrominance, AC chrominance

# PSNR of the restatement may fall short of PIL's own encoder (same image, same quality) by at most this many dB: twice the worst
# shortfall measured over images() x qualities 50 / 90 / 100 (table in DESIGN.md section 6e), and not below 0.1 dB
PSNR_MARGIN_DB = 0.1


def zigzag():
    """Natural (row-major, row = vertical frequency) index of the k-th coefficient in zigzag order (T.81 figure A.6)."""
    zz = []
    for s in range(15):
        pts = [(y, s - y) for y in range(8) if 0 <= s - y < 8]
        zz += [y * 8 + x for y, x in (pts[::-1] if s % 2 == 0 else pts)]
    return zz


def dqt_body(quality, which):
    """64 divisors (zigzag order) of libjpeg's quality scaling of the Annex K table ``which`` (0 luminance, 1 chrominance)."""
    base = bytes.fromhex(_DQT_HEX[which])
    scale = 5000 // quality if quality < 50 else 200 - 2 * quality
    return bytes(min(max((b * scale + 50) // 100, 1), 255) for b in base)


def dht_body(cls, ident):
    return bytes.fromhex(_DHT_HEX[(cls, ident)])


@functools.lru_cache(None)
def huffman(cls, ident):
    """symbol -> (code, length), the canonical code of T.81 Annex C from the counts and symbols of a DHT body."""
    body = dht_body(cls, ident)
    counts, syms = body[:16], body[16:]
    assert sum(counts) == len(syms)
    table, code, k = {}, 0, 0
    for length in range(1, 17):
        for _ in range(counts[length - 1]):
            table[syms[k]] = (code, length)
            code += 1
            k += 1
        code <<= 1
    return table


def dct_matrix():
    """T[u][x] = rint(8192 * a(u) * cos((2x+1) u pi / 16)), a(0) = sqrt(1/8), a(u>0) = sqrt(2/8), float64 -> int64."""
    u, x = np.arange(8, dtype=np.float64)[:, None], np.arange(8, dtype=np.float64)[None, :]
    a = np.where(u == 0, np.sqrt(1.0 / 8.0), np.sqrt(2.0 / 8.0))
    return np.rint(8192.0 * a * np.cos((2 * x + 1) * u * np.pi / 16)).astype(np.int64)


def _seg(marker, body):
    return bytes([0xFF, marker]) + (len(body) + 2).to_bytes(2, "big") + body


def header(W, H, quality, restart_mcus):
    h = b"\xff\xd8" + _seg(0xE0, b"JFIF\0\x01\x01\0\0\x01\0\x01\0\0")
    for which in (0, 1):
        h += _seg(0xDB, bytes([which]) + dqt_body(quality, which))
    h += _seg(0xC0, bytes([8]) + H.to_bytes(2, "big") + W.to_bytes(2, "big") + bytes([3, 1, 0x22, 0, 2, 0x11, 1, 3, 0x11, 1]))
    for cls, ident in DHT_ORDER:
        h += _seg(0xC4, bytes([cls << 4 | ident]) + dht_body(cls, ident))
    h += _seg(0xDD, restart_mcus.to_bytes(2, "big"))
    return h + _seg(0xDA, bytes([3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0]))


def new_histogram():
    return {"zrl": 0, "eob": 0, "no_eob": 0, "dc_cat": [0] * 12, "ac_cat": [0] * 11, "stuffed": 0, "rst": [0] * 8, "rst_wrapped": 0}


def quantised_blocks(bgr, quality):
    """The frame's quantised coefficients in zigzag order: (Y [Hp/8, Wp/8, 64], Cb [Hp/16, Wp/16, 64], Cr likewise), int64."""
    bgr = np.asarray(bgr)
    assert bgr.dtype == np.uint8 and bgr.ndim == 3 and bgr.shape[2] == 3
    H, W = bgr.shape[:2]
    p = np.pad(bgr, ((0, -H % 16), (0, -W % 16), (0, 0)), mode="edge").astype(np.int64)
    B, G, R = p[..., 0], p[..., 1], p[..., 2]
    Y = (19595 * R + 38470 * G + 7471 * B + 32768) >> 16
    Cb = (-11059 * R - 21709 * G + 32768 * B + 8388608 + 32767) >> 16
    Cr = (32768 * R - 27439 * G - 5329 * B + 8388608 + 32767) >> 16
    T, zz = dct_matrix(), zigzag()
    out = []
    for plane, which in ((Y, 0), (Cb, 1), (Cr, 1)):
        if which:
            h2, w2 = plane.shape[0] // 2, plane.shape[1] // 2
            plane = (plane.reshape(h2, 2, w2, 2).sum(axis=(1, 3)) + 2) >> 2
        hb, wb = plane.shape[0] // 8, plane.shape[1] // 8
        s = plane.reshape(hb, 8, wb, 8).transpose(0, 2, 1, 3) - 128
        F = np.matmul(np.matmul(T, s), T.T)                               # exact: |F| < 2**35
        q = np.frombuffer(dqt_body(quality, which), np.uint8).astype(np.int64)
        Fz = F.reshape(hb, wb, 64)[..., zz]
        out.append(np.sign(Fz) * ((np.abs(Fz) + (q << 25)) // (q << 26)))
    return tuple(out)


def _bits_of(v):
    """(category s, the s bits T.81 F.1.2.1 appends for v)."""
    s = int(abs(v)).bit_length()
    return s, (v if v >= 0 else v + (1 << s) - 1)


def encode(bgr, quality, restart_mcus, hist=None):
    """One complete baseline JPEG file (bytes) of the uint8 BGR image by the definition of DESIGN.md 6e; ``hist`` (new_histogram())
    collects what was emitted."""
    hist = new_histogram() if hist is None else hist
    H, W = np.asarray(bgr).shape[:2]
    Yq, Cbq, Crq = quantised_blocks(bgr, quality)
    mh, mw = Cbq.shape[:2]
    tabs = {0: (huffman(0, 0), huffman(1, 0)), 1: (huffman(0, 1), huffman(1, 1))}
    out = bytearray(header(W, H, quality, restart_mcus))
    acc = nbits = 0

    def put(code, length):
        nonlocal acc, nbits
        acc = (acc << length) | code
        nbits += length

    pred = [0, 0, 0]
    for m in range(mh * mw):
        if m and m % restart_mcus == 0:
            pad = -nbits % 8
            put((1 << pad) - 1, pad)
            data = acc.to_bytes(nbits // 8, "big")
            hist["stuffed"] += data.count(b"\xff")
            idx = (m // restart_mcus - 1) % 8
            hist["rst"][idx] += 1
            hist["rst_wrapped"] += int(m // restart_mcus - 1 >= 8)
            out += data.replace(b"\xff", b"\xff\x00") + bytes([0xFF, 0xD0 + idx])
            acc = nbits = 0
            pred = [0, 0, 0]
        my, mx = divmod(m, mw)
        for comp, blk in ((0, Yq[2 * my, 2 * mx]), (0, Yq[2 * my, 2 * mx + 1]), (0, Yq[2 * my + 1, 2 * mx]), (0, Yq[2 * my + 1, 2 * mx + 1]),
                          (1, Cbq[my, mx]), (2, Crq[my, mx])):
            dc_tab, ac_tab = tabs[min(comp, 1)]
            dc = int(blk[0])
            s, extra = _bits_of(dc - pred[comp])
            pred[comp] = dc
            hist["dc_cat"][s] += 1
            put(*dc_tab[s])
            put(extra, s)
            last = 0
            for k in np.flatnonzero(blk[1:]) + 1:
                k = int(k)
                run = k - last - 1
                while run > 15:
                    put(*ac_tab[0xF0])
                    hist["zrl"] += 1
                    run -= 16
                s, extra = _bits_of(int(blk[k]))
                hist["ac_cat"][s] += 1
                put(*ac_tab[run << 4 | s])
                put(extra, s)
                last = k
            if last < 63:
                put(*ac_tab[0x00])
                hist["eob"] += 1
            else:
                hist["no_eob"] += 1
    pad = -nbits % 8
    put((1 << pad) - 1, pad)
    data = acc.to_bytes(nbits // 8, "big")
    hist["stuffed"] += data.count(b"\xff")
    out += data.replace(b"\xff", b"\xff\x00") + b"\xff\xd9"
    return bytes(out)


def psnr(a, b):
    d = np.asarray(a, np.float64) - np.asarray(b, np.float64)
    return 10.0 * np.log10(255.0 ** 2 / max(float(np.mean(d * d)), 1e-12))


# ---- images (height x width x BGR) -------------------------------------------------------------------------------------------------
def _ramp(h, w):
    y, x = np.mgrid[0:h, 0:w]
    return np.stack([(x * 255) // max(w - 1, 1), (y * 255) // max(h - 1, 1), ((x + y) * 255) // max(w + h - 2, 1)], axis=2).astype(np.uint8)


def _overlay(h, w):
    img = _ramp(h, w)
    img[7, :] = (255, 0, 0)
    img[:, 19] = (0, 0, 255)
    for k in range(min(h, w)):
        img[k, k] = (36, 231, 253)
    y, x = np.mgrid[0:h, 0:w]
    img[(y - 26) ** 2 + (x - 40) ** 2 <= 81] = (120, 183, 53)
    return img


def _extremes(h, w):
    y, x = np.mgrid[0:h, 0:w]
    img = np.where(((y // 8) + (x // 8)) % 2 == 0, 0, 255)
    img[:, w // 2:] = np.where((y[:, w // 2:] + x[:, w // 2:]) % 2 == 0, 0, 255)       # pixel checkerboard next to the 8 x 8 blocks
    img[16:32, w // 2:w // 2 + 16] = np.where((y[16:32, :16] + x[16:32, :16]) % 2 == 0, 255, 0)   # ... and its inverse
    return np.stack([img] * 3, axis=2).astype(np.uint8)


def real_pair():
    """Two real 240 x 640 frames (two eyes side by side) of the evaluate_real_frames fixture: one plain grey -> BGR, one with the class
    colours of the fixture's masks."""
    from common import gold
    g = gold("evaluate_real_frames")
    a = np.concatenate([g["eyes"][0], g["eyes"][1]], axis=1)
    b = np.concatenate([g["eyes"][2], g["eyes"][3]], axis=1)
    plain = np.stack([a] * 3, axis=2).astype(np.uint8)
    rendered = np.stack([b] * 3, axis=2).astype(np.uint8)
    masks = np.asarray(g["masks"])
    if masks.ndim == 3 and masks.shape[1:] == (240, 320) and masks.shape[0] >= 4:
        m = np.concatenate([masks[2], masks[3]], axis=1)
        rendered[m == 1] = (120, 183, 53)
        rendered[m == 2] = (36, 231, 253)
    return plain, rendered


@functools.lru_cache(None)
def images(restart_mcus):
    """name -> (uint8 BGR image, qualities it is encoded at).  Every image at 90; noise / extremes / odd size also at 50 and 100."""
    rs = np.random.RandomState(7)
    full = (50, 90, 100)
    grey = (rs.randint(0, 256, (40, 56), dtype=np.uint8) // 4 * 3 + _ramp(40, 56)[..., 2] // 4).astype(np.uint8)
    plain, rendered = real_pair()
    strip = np.concatenate([_ramp(16, 16 * restart_mcus * 5), rs.randint(0, 256, (16, 16 * restart_mcus * 5, 3), dtype=np.uint8)], axis=1)
    return {
        "one_mcu": (rs.randint(0, 256, (16, 16, 3), dtype=np.uint8), (90,)),
        "odd_size": (_overlay(40, 56)[3:16, 5:26].copy(), full),
        "noise": (rs.randint(0, 256, (40, 56, 3), dtype=np.uint8), full),
        # (B, G, R) whose Y, Cb, Cr = 100, 145, 111 give DC coefficients on multiples of the quality-50 divisors (16, 17, 17): on a constant
        # image the whole error is three DC roundings, and off such a point the PSNR only says which way each encoder's happened to fall
        "flat": (np.full((40, 56, 3), (130, 106, 76), np.uint8), (90,)),
        "grey": (np.stack([grey] * 3, axis=2), (90,)),
        "overlay": (_overlay(40, 56), (90,)),
        "extremes": (_extremes(48, 64), full),
        "strip": (np.ascontiguousarray(strip), (90,)),
        "real_plain": (plain, (90,)),
        "real_rendered": (rendered, (90,)),
    }


@functools.lru_cache(None)
def encoded(name, quality, restart_mcus):
    """(stream, histogram) of images()[name] -- computed once per process and shared by the tests."""
    hist = new_histogram()
    return encode(images(restart_mcus)[name][0], quality, restart_mcus, hist), hist


# ---- frame number -----------------------------------------------------------------------------------------------------------------
def blend(frames, mask, x0, y0, ink_bgr):
    """What egne_stamp_mask computes: frames uint8 [N,H,W,3] (a copy is returned), mask uint8 [N,ph,pw] at origin (x0, y0), clipped."""
    out = np.array(frames, copy=True)
    N, H, W = out.shape[:3]
    ph, pw = mask.shape[1:]
    ys, xs = slice(max(y0, 0), min(y0 + ph, H)), slice(max(x0, 0), min(x0 + pw, W))
    if ys.start >= ys.stop or xs.start >= xs.stop:
        return out
    a = mask[:, ys.start - y0: ys.stop - y0, xs.start - x0: xs.stop - x0].astype(np.int64)[..., None]
    t = out[:, ys, xs].astype(np.int64) * (255 - a) + np.asarray(ink_bgr, np.int64) * a + 128
    out[:, ys, xs] = (((t >> 8) + t) >> 8).astype(np.uint8)
    return out
