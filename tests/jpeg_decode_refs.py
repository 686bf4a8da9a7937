"""NumPy restatement of the decode path the device Motion-JPEG decoder is pinned to (evaluate.py --device_decode 1):
libjpeg-turbo's defaults -- sequential Huffman decode (T.81 F.2.2), jidctint "islow", fancy upsampling -- followed by PIL's
convert('L').  Integer arithmetic with arithmetic shifts throughout.  test_host_jpeg_decode.py holds it against PIL byte for byte;
the GPU tests hold the kernels against it.  Its marker walk is its own (the product's is evaluate.jpeg_parse)."""
import numpy as np

import jpeg_refs as J

ZZ = [0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28,
      35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63]


def _lookup(counts, symbols):
    """By the next 16 bits: (code length, symbol); length 0 = no code."""
    table, code, k = [(0, 0)] * 65536, 0, 0
    for length in range(1, 17):
        for _ in range(counts[length - 1]):
            lo = code << (16 - length)
            table[lo: lo + (1 << (16 - length))] = [(length, symbols[k])] * (1 << (16 - length))
            code, k = code + 1, k + 1
        code <<= 1
    return table


def parse(j):
    """(H, W, [(h, v, tq)], {tq: int64 [64]}, {(class, id): lookup}, [(td, ta)], restart interval, scan bytes up to EOI)."""
    assert j[:2] == b"\xff\xd8"
    p, qt, ht, ri = 2, {}, {}, 0
    while True:
        assert j[p] == 0xFF
        m, n = j[p + 1], int.from_bytes(j[p + 2: p + 4], "big")
        b = j[p + 4: p + 2 + n]
        if m == 0xDB:
            for k in range(0, len(b), 65):
                assert b[k] >> 4 == 0
                qt[b[k] & 15] = np.array(list(b[k + 1: k + 65]), np.int64)
        elif m == 0xC4:
            k = 0
            while k < len(b):
                counts = list(b[k + 1: k + 17])
                ht[(b[k] >> 4, b[k] & 15)] = _lookup(counts, b[k + 17: k + 17 + sum(counts)])
                k += 17 + sum(counts)
        elif m == 0xC0:
            assert b[0] == 8
            H, W = int.from_bytes(b[1:3], "big"), int.from_bytes(b[3:5], "big")
            comps = [(b[7 + 3 * i] >> 4, b[7 + 3 * i] & 15, b[8 + 3 * i]) for i in range(b[5])]
        elif m == 0xDD:
            ri = int.from_bytes(b, "big")
        elif m == 0xDA:
            sel = [(b[2 + 2 * i] >> 4, b[2 + 2 * i] & 15) for i in range(b[0])]
            scan = j[p + 2 + n:]
            if not ht:                                      # AVI Motion-JPEG: the tables of Annex K
                for cls, ident in J.DHT_ORDER:
                    body = J.dht_body(cls, ident)
                    ht[(cls, ident)] = _lookup(list(body[:16]), body[16:])
            return H, W, comps, qt, ht, sel, ri, scan[:scan.index(b"\xff\xd9")]
        else:
            assert m in (0xE0, 0xE1, 0xE2, 0xEE, 0xFE) or 0xE0 <= m <= 0xEF, hex(m)
        p += 2 + n


def coefficients(j):
    """The quantised coefficients of a baseline file after DC prediction: (int16 [blocks, 64] in zigzag order, blocks in MCU order,
    geometry dict(H, W, hs, vs, mw, mh, comps, qt))."""
    H, W, comps, qt, ht, sel, ri, scan = parse(j)
    hs, vs = comps[0][0], comps[0][1]
    if len(comps) == 1:
        hs = vs = 1                                        # a scan of one component is not interleaved
    assert all(c[:2] == (1, 1) for c in comps[1:])
    mw, mh = -(-W // (8 * hs)), -(-H // (8 * vs))
    order = [0] * (hs * vs) + list(range(1, len(comps)))
    # segments: RSTm removed, stuffing removed
    segs, at = [], 0
    while True:
        nxt = min((k for k in (scan.find(bytes((0xFF, 0xD0 + m)), at) for m in range(8)) if k >= 0), default=-1)
        segs.append(scan[at: nxt if nxt >= 0 else len(scan)].replace(b"\xff\x00", b"\xff"))
        if nxt < 0:
            break
        at = nxt + 2
    nmcu = mw * mh
    assert len(segs) == (-(-nmcu // ri) if ri else 1), (len(segs), nmcu, ri)
    out = np.zeros((nmcu * len(order), 64), np.int16)
    blk = 0
    for s, seg in enumerate(segs):
        bits = "".join(format(x, "08b") for x in seg) + "1" * 32
        pos, pred = 0, [0] * len(comps)
        for _ in range(min(ri, nmcu - s * ri) if ri else nmcu):
            for ci in order:
                dct, act = ht[(0, sel[ci][0])], ht[(1, sel[ci][1])]
                length, cat = dct[int(bits[pos: pos + 16], 2)]
                assert length
                pos += length
                if cat:
                    v = int(bits[pos: pos + cat], 2)
                    pos += cat
                    pred[ci] += v if v >= 1 << (cat - 1) else v - (1 << cat) + 1
                out[blk, 0] = pred[ci]
                k = 1
                while k < 64:
                    length, rs = act[int(bits[pos: pos + 16], 2)]
                    assert length
                    pos += length
                    r, cat = rs >> 4, rs & 15
                    if cat == 0:
                        if r == 15:
                            k += 16
                            continue
                        break
                    k += r
                    v = int(bits[pos: pos + cat], 2)
                    pos += cat
                    out[blk, k] = v if v >= 1 << (cat - 1) else v - (1 << cat) + 1
                    k += 1
                blk += 1
        assert pos <= 8 * len(seg) and 8 * len(seg) - pos < 8, (s, pos, len(seg))
    assert blk == len(out)
    return out, dict(H=H, W=W, hs=hs, vs=vs, mw=mw, mh=mh, comps=comps, qt=qt)


def _idct1(x, sh):
    """One pass of jidctint.c's jpeg_idct_islow along the last axis (CONST_BITS 13), descaled by ``sh``."""
    i = [x[..., k] for k in range(8)]
    z2, z3 = i[2], i[6]
    z1 = (z2 + z3) * 4433
    t2, t3 = z1 - z3 * 15137, z1 + z2 * 6270
    t0, t1 = (i[0] + i[4]) << 13, (i[0] - i[4]) << 13
    t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
    t0, t1, t2, t3 = i[7], i[5], i[3], i[1]
    z1, z2, z3, z4 = t0 + t3, t1 + t2, t0 + t2, t1 + t3
    z5 = (z3 + z4) * 9633
    t0, t1, t2, t3 = t0 * 2446, t1 * 16819, t2 * 25172, t3 * 12299
    z1, z2, z3, z4 = -z1 * 7373, -z2 * 20995, -z3 * 16069 + z5, -z4 * 3196 + z5
    t0, t1, t2, t3 = t0 + z1 + z3, t1 + z2 + z4, t2 + z2 + z3, t3 + z1 + z4
    o = [t10 + t3, t11 + t2, t12 + t1, t13 + t0, t13 - t0, t12 - t1, t11 - t2, t10 - t3]
    return np.stack([(v + (1 << (sh - 1))) >> sh for v in o], -1)


def _plane(blocks, q):
    """blocks int64 [by, bx, 64] in zigzag order -> uint8-valued samples [by*8, bx*8]."""
    by, bx, _ = blocks.shape
    nat = np.zeros((by, bx, 64), np.int64)
    nat[..., ZZ] = blocks * q
    b = nat.reshape(by, bx, 8, 8)
    w = _idct1(b.swapaxes(-1, -2), 11).swapaxes(-1, -2)          # columns first
    o = np.clip(_idct1(w, 18) + 128, 0, 255)
    return o.transpose(0, 2, 1, 3).reshape(by * 8, bx * 8)


def upsample_h2v2(c):
    """libjpeg's h2v2 fancy upsampling of a plane already cropped to the image's ceil(H/2) x ceil(W/2)."""
    h, w = c.shape
    cp = np.concatenate([c[:1], c, c[-1:]], 0)
    rows = np.empty((2 * h, w), np.int64)
    rows[0::2], rows[1::2] = cp[1:-1] * 3 + cp[:-2], cp[1:-1] * 3 + cp[2:]
    last, nxt = np.concatenate([rows[:, :1], rows[:, :-1]], 1), np.concatenate([rows[:, 1:], rows[:, -1:]], 1)
    out = np.empty((2 * h, 2 * w), np.int64)
    out[:, 0::2], out[:, 1::2] = (rows * 3 + last + 8) >> 4, (rows * 3 + nxt + 7) >> 4
    return out


def upsample_h2v1(c):
    """libjpeg's h2v1 fancy upsampling of a plane cropped to H x ceil(W/2)."""
    last, nxt = np.concatenate([c[:, :1], c[:, :-1]], 1), np.concatenate([c[:, 1:], c[:, -1:]], 1)
    out = np.empty((c.shape[0], 2 * c.shape[1]), np.int64)
    out[:, 0::2], out[:, 1::2] = (c * 3 + last + 1) >> 2, (c * 3 + nxt + 2) >> 2
    return out


def reconstruct(coef, g):
    """(L uint8 [H,W], RGB uint8 [H,W,3] or None for a grey file) from coefficients()'s results."""
    H, W, hs, vs, mw, mh = g["H"], g["W"], g["hs"], g["vs"], g["mw"], g["mh"]
    ncomp = len(g["comps"])
    bpm = hs * vs + ncomp - 1
    c = coef.astype(np.int64).reshape(mh, mw, bpm, 64)
    yb = c[:, :, :hs * vs].reshape(mh, mw, vs, hs, 64).transpose(0, 2, 1, 3, 4).reshape(mh * vs, mw * hs, 64)
    Y = _plane(yb, g["qt"][g["comps"][0][2]])[:H, :W]
    if ncomp == 1:
        return Y.astype(np.uint8), None
    ch, cw = -(-H // vs), -(-W // hs)
    chroma = []
    for k in (1, 2):
        p = _plane(c[:, :, hs * vs + k - 1], g["qt"][g["comps"][k][2]])[:ch, :cw]     # cropped BEFORE upsampling
        if (hs, vs) == (2, 2):
            p = upsample_h2v2(p)
        elif (hs, vs) == (2, 1):
            p = upsample_h2v1(p)
        else:
            assert (hs, vs) == (1, 1)
        chroma.append(p[:H, :W] - 128)
    cb, cr = chroma
    R = np.clip(Y + ((91881 * cr + 32768) >> 16), 0, 255)
    G = np.clip(Y + ((-22554 * cb + 32768 - 46802 * cr) >> 16), 0, 255)
    B = np.clip(Y + ((116130 * cb + 32768) >> 16), 0, 255)
    L = (19595 * R + 38470 * G + 7471 * B + 32768) >> 16
    return L.astype(np.uint8), np.stack([R, G, B], -1).astype(np.uint8)


def decode(j):
    return reconstruct(*coefficients(j))
