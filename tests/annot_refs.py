"""NumPy restatement of the label maps from TEyeD annotations (csrc/annot_core.h, include/egne_hip.h) and of
dataprep.pack_annotations' arithmetic: test infrastructure only.  Integers are int64, the ellipse is float64 with one NumPy operation
per rounding, in the order the header states, so the kernel (built without FMA contraction) matches byte for byte."""
import hashlib

import numpy as np

RECORD_WORDS, MAX_VERTS = 150, 64
HAS_BALL, HAS_IRIS, HAS_PUPIL, HAS_LID = 1, 2, 4, 8
ST_IRIS_ZERO_AXIS, ST_PUPIL_ZERO_AXIS, ST_EMPTY = 1, 2, 4


def sha(a):
    a = np.ascontiguousarray(a)
    return hashlib.sha256(str((a.dtype.str, a.shape)).encode() + a.tobytes()).hexdigest()


def _grid(R, C):
    return np.arange(C, dtype=np.int64)[None, :], np.arange(R, dtype=np.int64)[:, None]


def circle_map(R, C, bx, by, br):
    x, y = _grid(R, C)
    if br < 0:
        return np.zeros((R, C), bool)
    dx, dy = x - int(bx), y - int(by)
    return dx * dx + dy * dy <= int(br) * int(br)


def ellipse_map(R, C, ex, ey, A, B, c, s):
    """cv2.ellipse's convention (first axis along (c, s), y down); nothing for a half-axis <= 0; evaluated inside the square of
    half-width max(A, B) + 1 about the centre."""
    if A <= 0 or B <= 0:
        return np.zeros((R, C), bool)
    x, y = _grid(R, C)
    ix, iy = x - int(ex), y - int(ey)
    m = max(int(A), int(B)) + 1
    box = (np.abs(ix) <= m) & (np.abs(iy) <= m)
    dx, dy = ix.astype(np.float64), iy.astype(np.float64)
    c, s, A, B = np.float64(c), np.float64(s), np.float64(A), np.float64(B)
    X = dx * c + dy * s
    Y = dy * c - dx * s
    XB, YA, AB = X * B, Y * A, A * B
    return box & (XB * XB + YA * YA <= AB * AB)


def polygon_map(R, C, pts):
    """Even-odd with the boundary included, the definition of include/egne_hip.h, edge by edge over the whole canvas."""
    x, y = _grid(R, C)
    odd, on = np.zeros((R, C), bool), np.zeros((R, C), bool)
    n = len(pts)
    for i in range(n):
        (x0, y0), (x1, y1) = (int(v) for v in pts[i]), (int(v) for v in pts[(i + 1) % n])
        if y0 > y1:
            x0, y0, x1, y1 = x1, y1, x0, y0
        cross = (x - x0) * (y1 - y0) - (x1 - x0) * (y - y0)
        if y0 != y1:
            odd ^= (y >= y0) & (y < y1) & (cross < 0)
        on |= (cross == 0) & (y >= y0) & (y <= y1) & (x >= min(x0, x1)) & (x <= max(x0, x1))
    return odd | on


def unpack(rec):
    """One record -> dict (flags, ball, iris, pupil, lid points)."""
    rec = np.ascontiguousarray(rec, np.int32)
    d = rec.view(np.float64)
    n = min(max(int(rec[1]), 0), MAX_VERTS)
    return {"flags": int(rec[0]), "ball": tuple(int(v) for v in rec[2:5]),
            "iris": tuple(int(v) for v in rec[6:10]) + (float(d[5]), float(d[6])),
            "pupil": tuple(int(v) for v in rec[14:18]) + (float(d[9]), float(d[10])),
            "lid": rec[22:22 + 2 * n].reshape(n, 2).astype(np.int64)}


def paint(records, R, C, src_hw=None, with_skin=True):
    """(noskin, skin or None, status): int8 [B,R,C] maps and int32 [B] status words of a batch of records."""
    records = np.asarray(records, np.int32).reshape(-1, RECORD_WORDS)
    B = len(records)
    noskin = np.zeros((B, R, C), np.int8)
    skin = np.zeros((B, R, C), np.int8) if with_skin else None
    status = np.zeros(B, np.int32)
    for b in range(B):
        u = unpack(records[b])
        r, c = (R, C) if src_hw is None else (min(max(int(src_hw[b][0]), 0), R), min(max(int(src_hw[b][1]), 0), C))
        m = np.zeros((r, c), np.int8)
        if u["flags"] & HAS_BALL:
            m[circle_map(r, c, *u["ball"])] = 1
        for bit, key, val, st in ((HAS_IRIS, "iris", 2, ST_IRIS_ZERO_AXIS), (HAS_PUPIL, "pupil", 3, ST_PUPIL_ZERO_AXIS)):
            if u["flags"] & bit:
                if u[key][2] <= 0 or u[key][3] <= 0:
                    status[b] |= st
                m[ellipse_map(r, c, *u[key])] = val
        if not m.any():
            status[b] |= ST_EMPTY
        noskin[b, :r, :c] = m
        if with_skin:
            skin[b, :r, :c] = np.where(polygon_map(r, c, u["lid"]), m, 0) if u["flags"] & HAS_LID else m
    return noskin, skin, status


def pack(ball, iris, pupil, lid, present=None):
    """dataprep.pack_annotations' arithmetic, frame by frame with Python's own int(): (r, cx, cy), (angle, cx, cy, w, h) twice and
    [n,2] points per frame (None: absent)."""
    B = len(ball)
    rec = np.zeros((B, RECORD_WORDS), np.int32)
    d = rec.view(np.float64)
    for b in range(B):
        pr = [True] * 4 if present is None else list(present[b])
        flags = 0
        if ball[b] is not None and pr[0]:
            flags |= HAS_BALL
            rec[b, 2:5] = (int(ball[b][1]), int(ball[b][2]), int(ball[b][0]))
        for e, bit, w, on in ((iris[b], HAS_IRIS, 6, pr[1]), (pupil[b], HAS_PUPIL, 14, pr[2])):
            if e is not None and on:
                flags |= bit
                rec[b, w:w + 4] = (int(e[1]), int(e[2]), int(e[3] / 2), int(e[4] / 2))
                t = np.radians(np.float64(e[0]))
                d[b, w // 2 + 2], d[b, w // 2 + 3] = np.cos(t), np.sin(t)
        if lid[b] is not None and pr[3]:
            flags |= HAS_LID
            rec[b, 1] = len(lid[b])
            for k, p in enumerate(lid[b]):
                rec[b, 22 + 2 * k], rec[b, 23 + 2 * k] = int(p[0]), int(p[1])
        rec[b, 0] = flags
    return rec


# ---- the cases of tests/test_gpu_annot.py and of the host program ------------------------------------------------------------------------
def eyelid(rng, R, C, n=34, jitter=0.0, cross=False, reach=0.0):
    """An eyelid-shaped n-gon as float points: the upper arc left to right, the lower arc back; ``reach`` pushes it beyond the canvas."""
    h = n // 2
    t = np.linspace(0, 1, h)
    x0, x1 = C * (0.1 - reach), C * (0.9 + reach)
    cy, ay = R * rng.uniform(0.4, 0.6), R * rng.uniform(0.15, 0.4 + reach)
    up = np.stack([x0 + (x1 - x0) * t, cy - ay * np.sin(np.pi * t)], 1)
    lo = np.stack([x1 - (x1 - x0) * np.linspace(0, 1, n - h), cy + ay * rng.uniform(0.5, 1) * np.sin(np.pi * np.linspace(0, 1, n - h))], 1)
    p = np.concatenate([up, lo]) + rng.uniform(-jitter, jitter, (n, 2))
    if cross:          # swap two vertices of the lower arc: a self-intersection
        i, j = h + 2, n - 3
        p[[i, j]] = p[[j, i]]
    return p


def special_frames(R, C):
    """The named corner cases on an R x C canvas: a list of (name, ball, iris, pupil, lid, present)."""
    cx, cy = C / 2.0, R / 2.0
    s = min(R, C)
    full = [(-3, -2), (C + 5, -4), (C + 3, R + 6), (-7, R + 2)]
    none = [(C + 3, 1), (C + 9, 2), (C + 5, R - 1)]
    base_lid = eyelid(np.random.RandomState(R * 1000 + C), R, C)
    ok = (True, True, True, True)
    F = [
        ("plain", (s * 0.45, cx, cy), (30.0, cx, cy, s * 0.5, s * 0.4), (120.0, cx + 1, cy - 1, s * 0.2, s * 0.25), base_lid, ok),
        ("partly_outside", (s * 0.6, C - 2.5, 1.5), (0.0, -2.6, R - 1.9, s * 0.7, s * 0.3), (90.0, C - 1.0, R - 1.0, s * 0.3, s * 0.5), base_lid, ok),
        ("wholly_outside", (3.0, -40.0, -50.0), (10.0, C + 60.0, 5.0, 20.0, 12.0), (15.0, 5.0, R + 70.0, 9.0, 30.0), base_lid, ok),          # paints nothing
        ("negative_half", (2.9, -0.5, -0.5), (180.0, -0.5, cy, s * 0.4, s * 0.2), (-33.0, cx, -0.9, s * 0.3, s * 0.1), full, ok),
        ("radius_zero", (0.7, cx, cy), (137.25, cx, cy, 2.0, 2.0), (0.0, cx, cy, 3.9, 2.1), full, (True, False, False, True)),
        ("radius_huge", (4.0 * (R + C), cx, cy), (137.25, cx - 2, cy + 1, s * 0.9, s * 0.35), (-137.25, cx + 2, cy, s * 0.3, s * 0.6), base_lid, ok),
        ("zero_axes", (s * 0.3, cx, cy), (45.0, cx, cy, 1.9, s * 0.5), (45.0, cx, cy, s * 0.4, 0.0), base_lid, ok),
        ("pupil_outside_iris", (s * 0.5, cx, cy), (20.0, cx - s * 0.2, cy, s * 0.3, s * 0.3), (70.0, cx + s * 0.25, cy + 2, s * 0.2, s * 0.15), full, ok),
        ("lid_self_intersects", (s * 0.5, cx, cy), (0.0, cx, cy, s * 0.6, s * 0.5), (90.0, cx, cy, s * 0.2, s * 0.2),
         eyelid(np.random.RandomState(7), R, C, cross=True, jitter=1.0), ok),
        ("lid_horizontal_edges", (s * 0.5, cx, cy), (0.0, cx, cy, s * 0.6, s * 0.5), (90.0, cx, cy, s * 0.2, s * 0.2),
         [(1, R // 3), (C - 2, R // 3), (C - 2, R // 2), (C // 2, R // 2), (C // 2, (2 * R) // 3), (1, (2 * R) // 3)], ok),
        ("lid_shared_vertex", (s * 0.5, cx, cy), (0.0, cx, cy, s * 0.6, s * 0.5), (90.0, cx, cy, s * 0.2, s * 0.2),
         [(1, 1), (C // 2, R // 2), (C - 2, 1), (C - 2, R - 2), (C // 2, R // 2), (1, R - 2)], ok),          # two rising edges meet at the centre
        ("lid_covers_all", (s * 0.5, cx, cy), (200.0, cx, cy, s * 0.6, s * 0.5), (90.0, cx, cy, s * 0.2, s * 0.2), full, ok),
        ("lid_covers_none", (s * 0.5, cx, cy), (0.0, cx, cy, s * 0.6, s * 0.5), (90.0, cx, cy, s * 0.2, s * 0.2), none, ok),
        ("absent_ball_lid", (s * 0.5, cx, cy), (0.0, cx, cy, s * 0.6, s * 0.5), (90.0, cx, cy, s * 0.2, s * 0.2), base_lid, (False, True, True, False)),
        ("absent_all", (s * 0.5, cx, cy), (0.0, cx, cy, s * 0.6, s * 0.5), (90.0, cx, cy, s * 0.2, s * 0.2), base_lid, (False, False, False, False)),
        ("triangle", (s * 0.5, cx, cy), (0.0, cx, cy, s * 0.6, s * 0.5), (90.0, cx, cy, s * 0.2, s * 0.2), [(0, 0), (C - 1, R // 2), (C // 3, R - 1)], ok),
        ("n64", (s * 0.5, cx, cy), (61.0, cx, cy, s * 0.7, s * 0.5), (90.0, cx, cy, s * 0.2, s * 0.2),
         eyelid(np.random.RandomState(64), R, C, n=64, jitter=0.7, reach=0.2), ok),
        ("zero_area_lid", (s * 0.5, cx, cy), (0.0, cx, cy, s * 0.9, s * 0.9), (90.0, cx, cy, s * 0.2, s * 0.2),
         [(0, 0), (C - 1, R - 1), (0, 0), (C - 1, R - 1)], ok),
    ]
    return F


def case_records(R, C, B, first=0):
    """B records of special_frames(R, C), starting at ``first`` (wrapping), through pack(): (names, records)."""
    F = special_frames(R, C)
    pick = [F[(first + i) % len(F)] for i in range(B)]
    rec = pack([f[1] for f in pick], [f[2] for f in pick], [f[3] for f in pick], [f[4] for f in pick], [f[5] for f in pick])
    return [f[0] for f in pick], rec


def ragged_hw(R, C, B):
    """Frame sizes for a ragged batch: the canvas itself, then smaller frames (one of a single row)."""
    sizes = [(R, C), (max(1, R - 3), max(1, C - 5)), (max(1, R // 2), C), (1, max(1, C // 3)), (R, max(1, C - 1))]
    return np.array([sizes[i % len(sizes)] for i in range(B)], np.int32)


def distance_to_edges(px, py, pts):
    """Euclidean distance of the points (px, py) to the nearest edge (a segment) of the closed polygon ``pts``."""
    p = np.stack([px, py], 1).astype(np.float64)
    best = np.full(len(p), np.inf)
    n = len(pts)
    for i in range(n):
        a, b = np.asarray(pts[i], np.float64), np.asarray(pts[(i + 1) % n], np.float64)
        ab = b - a
        L = float(ab @ ab)
        t = np.clip(((p - a) @ ab) / L, 0, 1) if L > 0 else np.zeros(len(p))
        q = a + t[:, None] * ab
        best = np.minimum(best, np.hypot(*(p - q).T))
    return best


def seeded_annotations(n, seed, R=480, C=640):
    """Seeded TEyeD-shaped rows for n frames: (ball [n,3], iris [n,5], pupil [n,5], lid [n,34,2]) float64, all accepted by
    annotation_keep, angles on both sides of 90, some lid points negative or beyond the canvas."""
    rng = np.random.RandomState(seed)
    s = min(R, C)
    ball, iris, pupil, lid = [], [], [], []
    for i in range(n):
        cx, cy = C * rng.uniform(0.35, 0.65), R * rng.uniform(0.35, 0.65)
        ball.append((s * rng.uniform(0.3, 0.5), cx + rng.uniform(-5, 5), cy + rng.uniform(-5, 5)))
        iw = s * rng.uniform(0.3, 0.45)
        iris.append((rng.uniform(0, 180), cx, cy, iw, iw * rng.uniform(0.6, 1.0)))
        pw = iw * rng.uniform(0.25, 0.5)
        pupil.append((rng.uniform(0, 180), cx + rng.uniform(-3, 3), cy + rng.uniform(-3, 3), pw, pw * rng.uniform(0.6, 1.0)))
        lid.append(eyelid(rng, R, C, jitter=1.5, reach=0.15 * (i % 3 == 1)))
    return np.array(ball), np.array(iris), np.array(pupil), np.array(lid)


# ---- made-up datasets for the tool: frames plus the four annotation files -------------------------------------------------------------------
LID_FIELDS = list(range(2, 35, 2)) + list(range(68, 35, -2))


def write_annotation_files(prefix, ball, iris, pupil, lid, lead_rows=0):
    """The four TEyeD files behind ``prefix`` (';'-separated, one header line, a trailing ';'); ``lead_rows`` rows of zeros in front
    (1: the NvGaze layout, where frame k reads row k + 1)."""
    n = len(ball) + lead_rows
    lm = np.zeros((n, 70))
    for k, i in enumerate(LID_FIELDS):
        lm[lead_rows:, i], lm[lead_rows:, i + 1] = lid[:, k, 0], lid[:, k, 1]
    tabs = {"eye_ball": np.zeros((n, 4)), "iris_eli": np.zeros((n, 6)), "pupil_eli": np.zeros((n, 6)), "lid_lm_2D": lm}
    tabs["eye_ball"][lead_rows:, 1:], tabs["iris_eli"][lead_rows:, 1:], tabs["pupil_eli"][lead_rows:, 1:] = ball, iris, pupil
    for name, t in tabs.items():
        t[:, 0] = np.arange(n)
        with open(prefix + name + ".txt", "w") as f:
            f.write("FRAME;VALUES;\n" + "".join(";".join(repr(float(v)) for v in row) + ";\n" for row in t))


def write_frame_dir(path, images):
    """Lossless PNG files whose sorted names keep the order."""
    import os
    from PIL import Image
    os.makedirs(path)
    for k, im in enumerate(images):
        Image.fromarray(im).save(os.path.join(path, "%05d.png" % k))
    return path


def seeded_frames(n, r, c, seed):
    """Smooth uint8 frames (a JPEG keeps them within a few grey levels)."""
    rng = np.random.RandomState(seed)
    y, x = np.mgrid[0:r, 0:c]
    return np.stack([np.clip(128 + 80 * np.sin(x / rng.uniform(9, 30) + rng.uniform(0, 6)) * np.cos(y / rng.uniform(9, 30)) + rng.randint(-20, 20),
                             0, 255).astype(np.uint8) for _ in range(n)])
