"""NumPy restatement of the reference's item path (CurriculumLib.DataLoader_riteyes.__getitem__, :94-166, with pad2Size
helperfunctions.py:406-428, scaleFn :78-89 and get_ellipse_info :488-518), augmentation off -- TEST INFRASTRUCTURE ONLY.

Pinned by tests/golden/loader.npz, which tests/golden/make_golden_loader.py records by driving the reference's own __getitem__.
OpenCV is not installed: the three cv2 calls of the path go through ``Cv2Recorder``, which RECORDS what it is handed (the fixture
pins those arguments against the reference) and answers with this project's restatements -- oracle.dataprep's Canny / dilate and
evaluate.resize_lanczos4 / resize_nearest, all PARITY UNPINNED against OpenCV itself.
"""
import hashlib
import math

import numpy as np

import egne_amd  # noqa: F401
from egne_amd import evaluate, synth
from oracle import dataprep as OD

INTER_NEAREST, INTER_LANCZOS4 = 0, 4          # OpenCV's documented enum values

# (synth.augment_case seed, source rows, source columns, annotation dropped: None | "pupil" | "ellipses" | "mask" | "iris")
CASES_PLAIN = [(7, 24, 32, None), (8, 20, 28, None), (10, 16, 32, None), (9, 24, 32, "pupil"), (11, 20, 28, "ellipses"),
               (13, 24, 32, "mask")]
SIZE_PLAIN = (24, 32)
CASES_SCALED = [(7, 48, 64, None), (8, 44, 60, None), (9, 48, 64, "pupil"), (10, 40, 64, "iris"), (13, 48, 60, "mask")]
SIZE_SCALED, SCALE = (48, 64), 0.5


def sha(a):
    a = np.ascontiguousarray(a)
    return hashlib.sha256(a.tobytes()).hexdigest() + " " + str(a.dtype) + " " + "x".join(str(n) for n in a.shape)


def raw_case(seed, r, c, drop=None):
    """One raw sample (what readImage returns) of r x c pixels from synth.augment_case, its ellipses scaled to the frame."""
    base, mask, pc, el = synth.augment_case(seed, H=r, W=c)
    sc = min(r / 240.0, c / 320.0)
    rng = np.random.RandomState(5000 + seed)
    iris = np.array([c * rng.uniform(0.4, 0.6), r * rng.uniform(0.4, 0.6), sc * rng.uniform(50, 75), sc * rng.uniform(50, 70), rng.uniform(-1.5, 1.5)])
    pupil = np.array([iris[0] + rng.uniform(-1, 1), iris[1] + rng.uniform(-1, 1), sc * rng.uniform(15, 30), sc * rng.uniform(12, 25), rng.uniform(-1.5, 1.5)])
    pc = pupil[:2].copy()
    mask = mask.astype(np.int8)
    if drop in ("pupil", "ellipses"):
        pupil[:] = -1
    if drop == "pupil":
        pc[:] = -1
    if drop in ("iris", "ellipses"):
        iris[:] = -1
    if drop == "mask":
        mask[:] = -1
    cond = np.array([np.all(pc == -1), np.all(mask == -1) or np.all(mask == 0), np.all(pupil == -1), np.all(iris == -1)])
    return base, mask, np.stack([iris, pupil]), pc, cond, np.array([seed, 0, seed % 4], np.int64)


class Cv2Recorder:
    """Stand-ins for cv2.Canny, cv2.dilate and cv2.resize: record the arguments, return the project's restatement."""

    def __init__(self):
        self.calls = []

    def Canny(self, image, threshold1, threshold2):
        self.calls.append("Canny %s %r %r" % (sha(image), threshold1, threshold2))
        return OD.canny_label_edges(image).astype(np.uint8) * 255

    def dilate(self, src, kernel, iterations=1):
        self.calls.append("dilate %s %r %r" % (sha(src), tuple(kernel), iterations))
        out = src.copy()
        out[1:] = np.maximum(src[1:], src[:-1])          # oracle/dataprep.py: the tuple (3, 3) is a two-row, one-column element
        return out

    def resize(self, src, dsize, interpolation):
        self.calls.append("resize %s %r %r" % (sha(src), tuple(int(d) for d in dsize), int(interpolation)))
        return (evaluate.resize_lanczos4 if interpolation == INTER_LANCZOS4 else evaluate.resize_nearest)(src, dsize)


def _rot(t):
    c, s = math.cos(t), math.sin(t)
    return np.array([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]])


def _trans(x, y):
    return np.array([[1.0, 0.0, x], [0.0, 1.0, y], [0.0, 0.0, 1.0]])


def ellipse_transform(param, H):
    """my_ellipse(param).transform(H)[0][:-1]: through the conic, float64 [5]."""
    cx, cy, a, b, th = (float(v) for v in param)
    Hr, Ht = _rot(-th), _trans(-cx, -cy)
    Q = np.diag([1 / a ** 2, 1 / b ** 2, -1.0])
    mat = Ht.T @ Hr.T @ Q @ Hr @ Ht
    Hi = np.linalg.inv(H)
    m = Hi.T @ mat @ Hi
    qa, qb, qc, qd, qe = m[0, 0], 2 * m[0, 1], m[1, 1], 2 * m[0, 2], 2 * m[1, 2]
    if abs(qb) <= 1e-40:
        t2 = 0.0 if qa <= qc else math.pi / 2
    else:
        t2 = 0.5 * math.atan2(qb, qa - qc)
    den = qb ** 2 - 4 * qa * qc
    tx, ty = (2 * qc * qd - qb * qe) / den, (2 * qa * qe - qb * qd) / den
    R2, T2 = _rot(t2), _trans(tx, ty)
    mn = R2.T @ T2.T @ m @ T2 @ R2
    return np.array([tx, ty, math.sqrt(1 / mn[0, 0]), math.sqrt(1 / mn[1, 1]), t2])


def ellipse_info(param, H, absent):
    """get_ellipse_info(param, H, cond)[1]."""
    if absent:
        return -np.ones(5)
    p = ellipse_transform(param, H)
    if p[2] > p[3]:
        p[[2, 3]] = p[[3, 2]]
        p[4] = 0.5 * math.pi + p[4]
    return p


def item(sample, size, scale=False, cv2=None):
    """The nine outputs of __getitem__ for one raw sample, as NumPy arrays of the reference's dtypes; ``cv2``: a Cv2Recorder."""
    cv2 = Cv2Recorder() if cv2 is None else cv2
    img, label, el, pc, cond, info = (np.array(a) for a in sample)
    el = el.astype(np.float64)
    pc = pc.astype(np.float64)
    r, c = img.shape
    up_r, up_c = size[0] - r, size[1] - c
    if up_r % 2 or up_c % 2 or up_r < 0 or up_c < 0:
        raise ValueError("pad2Size: odd or negative difference")
    up_r, up_c = up_r // 2, up_c // 2
    img = np.pad(img, ((up_r, up_r), (up_c, up_c)))
    label = np.pad(label, ((up_r, up_r), (up_c, up_c)))
    for k in range(2):
        if not np.all(el[k] == -1):
            el[k, :2] += (up_c, up_r)
    if not np.all(pc == -1):
        pc = pc + (up_c, up_r)
    if scale:
        dsize = (int(scale * img.shape[1]), int(scale * img.shape[0]))
        Hs = np.diag([scale, scale, 1.0])
        img = cv2.resize(img, dsize, INTER_LANCZOS4)
        label = cv2.resize(label, dsize, INTER_NEAREST)
        if np.all(el[0] == -1):           # the quirk of :85-86: the FIRST ellipse decides for both, and replaces the second
            el = np.stack([el[0], el[0]])
        else:
            el = np.stack([ellipse_transform(el[0], Hs), ellipse_transform(el[1], Hs)])
        if not np.all(pc == -1):
            pc = scale * pc
    label = label.copy()
    label[label == 1] = 0
    label[label == 2] = 1
    label[label == 3] = 2
    sw = 1 + cv2.dilate(cv2.Canny(label.astype(np.uint8), 0, 1) / 255, (3, 3), iterations=1) * 20
    dm = np.stack([OD.one_hot2dist(label.astype(np.uint8) == i) for i in range(3)])
    x = (img - img.mean()) / img.std()
    H, W = img.shape
    Hn = np.array([[2 / W, 0, -1], [0, 2 / H, -1], [0, 0, 1]])
    eln = np.stack([ellipse_info(el[0], Hn, cond[3]), ellipse_info(el[1], Hn, cond[2])])
    ic = el[0, :2] if not cond[3] else pc
    return (x[None].astype(np.float32), label.astype(np.int64), sw.astype(np.float32), dm.astype(np.float32), pc.astype(np.float32),
            ic.astype(np.float32), eln.astype(np.float32), cond.astype(bool), info.astype(np.int64)), cv2.calls


OUTPUTS = ("img", "label", "spatWts", "distMap", "pupil_center", "iris_center", "elNorm", "cond", "imInfo")


def ulp32_distance(a, b):
    """Units in the last place between two float32 arrays (same sign assumed where they differ by little)."""
    a = np.asarray(a, np.float32).view(np.int32).astype(np.int64)
    b = np.asarray(b, np.float32).view(np.int32).astype(np.int64)
    a = np.where(a < 0, -(a & 0x7fffffff), a)
    b = np.where(b < 0, -(b & 0x7fffffff), b)
    return np.abs(a - b)
