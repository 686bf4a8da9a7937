"""Inputs shared by tests/test_gpu_fit.py and tests/test_host_fit_cases.py: seeded class maps, ellipses and searches for the ellipse-fit
kernel (csrc/fit.hip) at shapes the 240x320 fixtures do not reach -- partial mask words and ballots, intervals clamped at a frame edge,
more rows than one pass covers -- and the oracle's answers for them (oracle/fit.py), computed once per process."""
import functools

import numpy as np

from oracle import fit as ofit

# (H, W): smallest legal | two words per row, 15 bits in the last | one bit in the third word (the second ballot holds one pixel) |
# 19 bits in the third word | W % 64 == 32 (the upper ballot half of the last step has no word) | more than 256 rows | the workload
SHAPES = [(2, 2), (33, 47), (37, 65), (61, 83), (64, 96), (300, 40), (240, 320)]
VALUES = np.array([-1, 0, 1, 2, 3, 255], np.int64)
CLASSES = (1, 2, 3)
N_RANDOM = 300
SHORT, LONG = 12, 16        # a row of fewer than SHORT inside pixels is tested pixel by pixel, LONG or more are surely walked


def render(H, W, el):
    """bool [H,W]: pixels inside the ellipse (cx, cy, a, b, theta in radians), float64 on the pixel grid (as make_golden.py does)."""
    cx, cy, a, b, t = el
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    X = (xx - cx) * np.cos(t) + (yy - cy) * np.sin(t)
    Y = -(xx - cx) * np.sin(t) + (yy - cy) * np.cos(t)
    return (X / a) ** 2 + (Y / b) ** 2 <= 1.0


def masks(H, W):
    """int64 [3,H,W] class maps with values from VALUES: 0 = background noise, two overlapping ellipses of classes 1 and 2 and 0.5 %
    speckle; 1 = all class 1; 2 = noise and an ellipse with no class 3 anywhere."""
    rng = np.random.RandomState(7 * (H * 1000 + W) + 1)
    m = np.zeros((3, H, W), np.int64)
    m[0] = VALUES[rng.choice(len(VALUES), size=(H, W), p=[0.05, 0.75, 0.05, 0.05, 0.05, 0.05])]
    m[0][render(H, W, (0.45 * W, 0.5 * H, 0.38 * W, 0.3 * H, 0.4))] = 1
    m[0][render(H, W, (0.55 * W, 0.45 * H, 0.2 * W, 0.22 * H, -0.3))] = 2
    sp = rng.rand(H, W) < 0.005
    m[0][sp] = VALUES[rng.randint(0, len(VALUES), size=int(sp.sum()))]
    m[1] = 1
    no3 = VALUES[VALUES != 3]
    m[2] = no3[rng.choice(len(no3), size=(H, W), p=[0.1, 0.6, 0.1, 0.1, 0.1])]
    m[2][render(H, W, (0.3 * W, 0.6 * H, 0.25 * W, 0.35 * H, 1.1))] = 1
    return m


def random_ellipses(H, W):
    """[N_RANDOM,5] float64 (cx, cy, a, b, angle in degrees): centres up to 20 % outside the frame, axes log-uniform over
    [0.3, 1.5 max(H, W)] px (ratios beyond 1000:1), a fifth of the angles exactly 0 / 90 / 45 / -45 degrees."""
    rng = np.random.RandomState(H * 1000 + W)
    n = N_RANDOM
    cx = rng.uniform(-0.2, 1.2, n) * W
    cy = rng.uniform(-0.2, 1.2, n) * H
    lo, hi = np.log(0.3), np.log(1.5 * max(H, W))
    a = np.exp(rng.uniform(lo, hi, n))
    b = np.exp(rng.uniform(lo, hi, n))
    r = rng.rand(n)
    ang = rng.uniform(-180.0, 180.0, n)
    special = np.array([0.0, 90.0, 45.0, -45.0])
    pick = r < 0.2
    ang[pick] = special[np.minimum((r[pick] / 0.05).astype(int), 3)]
    return np.stack([cx, cy, a, b, ang], axis=1)


# the non-tame set: (index changed, value) on the base ellipse (W/2, H/2, 0.3 W, 0.3 H, 10 degrees), and what the oracle makes of it
# at every shape: "empty" = no pixel inside (NaN or infinite parameters make every comparison false, or the ellipse is far away),
# "counted" = a finite count of at least one pixel (a = -3 is a = 3 after the conic round trip; a = 1e6 is a band through the frame)
NONTAME = {
    "a=0": (2, 0.0, "empty"),
    "a=-3": (2, -3.0, "counted"),
    "b=1e-9": (3, 1e-9, "empty"),
    "a=1e6": (2, 1e6, "counted"),
    "a=nan": (2, float("nan"), "empty"),
    "cx=1e7": (0, 1e7, "empty"),
}


def hand_ellipses(H, W):
    """(names, [k,5]) of the ellipses made by hand: whole frame, one per corner pixel, tangent to the first row / the last column from
    inside (whole-pixel axes), the non-tame set."""
    ax, ay = max(1, W // 4), max(1, H // 4)
    out = [("cover", ((W - 1) / 2.0, (H - 1) / 2.0, 2.0 * (H + W), 2.0 * (H + W), 0.0))]
    for name, x, y in (("corner00", 0, 0), ("corner0W", W - 1, 0), ("cornerH0", 0, H - 1), ("cornerHW", W - 1, H - 1)):
        out.append((name, (float(x), float(y), 0.4 * W + 1.0, 0.3 * H + 1.0, 20.0)))
    out.append(("tangent_row0", ((W - 1) / 2.0, float(ay), float(ax), float(ay), 0.0)))
    out.append(("tangent_lastcol", (float(W - 1 - ax), (H - 1) / 2.0, float(ax), float(ay), 0.0)))
    for name, (idx, val, _) in NONTAME.items():
        el = [W / 2.0, H / 2.0, 0.3 * W, 0.3 * H, 10.0]
        el[idx] = val
        out.append((name, tuple(el)))
    return [n for n, _ in out], np.array([e for _, e in out], np.float64)


def ellipses(H, W):
    """(names, [m,5]): the random ellipses ("r0" ...) followed by the hand-made ones."""
    names, hand = hand_ellipses(H, W)
    return ["r%d" % i for i in range(N_RANDOM)] + names, np.concatenate([random_ellipses(H, W), hand])


def count_batch(H, W):
    """One launch per shape: every ellipse against every (mask, class).  Returns (masks [3,H,W], ell [n,5], frame_of [n], cls [n],
    ell_index [n]) with n = 9 * number of ellipses."""
    _, ell = ellipses(H, W)
    m = len(ell)
    combos = [(f, c) for f in range(3) for c in CLASSES]
    fo = np.repeat([f for f, _ in combos], m).astype(np.int32)
    cl = np.repeat([c for _, c in combos], m).astype(np.int32)
    idx = np.tile(np.arange(m), len(combos))
    return masks(H, W), ell[idx], fo, cl, idx


@functools.lru_cache(maxsize=None)
def inside_maps(H, W):
    """The oracle's rasterised ellipse (oracle.fit.ell_inside, the map ell_counts counts) of every ellipse of the shape: bool [m,H,W]."""
    _, ell = ellipses(H, W)
    mesh = ofit.mesh_f32(H, W)
    with np.errstate(all="ignore"):
        out = np.stack([ofit.ell_inside((H, W), e, mesh) for e in ell])
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def oracle_counts(H, W):
    """uint32 [n,3] (nseg, nell, inter) for count_batch(H, W): what oracle.fit.ell_counts returns for every row (the map of an ellipse
    is rasterised once and counted against the nine class masks; tests/test_host_fit_cases.py holds this equal to ell_counts)."""
    mk, _, fo, cl, idx = count_batch(H, W)
    ins = inside_maps(H, W)
    out = np.zeros((len(idx), 3), np.uint32)
    segs = {(f, c): mk[f] == c for f in range(3) for c in CLASSES}
    for i in range(len(idx)):
        seg, ell = segs[(int(fo[i]), int(cl[i]))], ins[idx[i]]
        out[i] = (np.count_nonzero(seg), np.count_nonzero(ell), np.count_nonzero(ell & seg))
    out.setflags(write=False)
    return out


def population(H, W):
    """Fractions of the random ellipses by what the oracle's map looks like: strictly interior and non-empty, clipped by a frame edge
    (touches the border without covering the frame), empty, covering everything, and holding both a short and a long row."""
    ins = inside_maps(H, W)[:N_RANDOM]
    nell = ins.reshape(N_RANDOM, -1).sum(1)
    border = ins[:, 0].any(1) | ins[:, -1].any(1) | ins[:, :, 0].any(1) | ins[:, :, -1].any(1)
    rows = ins.sum(2)
    mixed = ((rows > 0) & (rows < SHORT)).any(1) & (rows >= LONG).any(1)
    full = nell == H * W
    return {"interior": float(np.mean((nell > 0) & ~border)), "clipped": float(np.mean(border & ~full)),
            "empty": float(np.mean(nell == 0)), "full": float(np.mean(full)), "mixed_rows": float(np.mean(mixed))}


# name -> (H, W, rendered ellipse (cx, cy, a, b, theta) | "empty" | "full", init (cx, cy, a, b, theta), evaluations of the oracle's search)
SEARCHES = {
    "inside": (61, 83, (40, 30, 18, 11, 0.4), (41, 29, 16, 13, 0.3), 76),
    "clipped_left_top": (61, 83, (6, 5, 20, 12, -0.6), (6, 5, 18, 14, -0.5), 23),
    "clipped_right_bottom": (61, 83, (78, 57, 20, 12, 0.9), (78, 57, 22, 10, 1.0), 29),
    "centre_outside": (61, 83, (-5, 30, 25, 15, 0.2), (-5, 30, 22, 17, 0.1), 98),
    "larger_than_frame": (33, 47, (23, 16, 60, 40, 0.3), (23, 16, 55, 45, 0.2), 8),
    "thin": (61, 83, (40, 30, 30, 2.5, 0.7), (40, 30, 28, 3.5, 0.6), 70),
    # the oracle ends at a = 1.0: the search scores a candidate axis of exactly 0 (inf / NaN conic parameters, whole-frame fallback)
    "tiny": (61, 83, (40, 30, 1.6, 1.2, 0), (40, 30, 2, 1.5, 0), 13),
    # theta exactly 0: the first evaluation takes the |b| <= 1e-40 branches of the conic normalisation
    "theta0_a_gt_b": (100, 130, (60, 50, 30, 20, 0), (60, 50, 28, 22, 0), 25),
    "theta0_a_lt_b": (100, 130, (60, 50, 20, 30, 0), (60, 50, 22, 28, 0), 38),
    "empty": (33, 47, "empty", (23, 16, 10, 8, 0.2), 8),                 # NaN scores
    "full": (33, 47, "full", (23, 16, 10, 8, 0.2), 139),
    "2x2": (2, 2, "full", (0.5, 0.5, 1, 1, 0), 20),
    "wide": (40, 200, (100, 20, 80, 15, 0.05), (100, 20, 75, 17, 0), 40),
    "tall": (200, 40, (20, 100, 15, 80, 0.05), (20, 100, 17, 75, 0.1), 56),
    "clipped_workload": (240, 320, (300, 200, 60, 40, 0.5), (300, 200, 55, 45, 0.4), 87),
}

# the batch of more than 256 rows (tests/test_gpu_fit.py, launch forms): rendered ellipse, init -- the tall ellipse, the same with axes
# swapped and a quarter turn, one off-centre and one cut by the bottom-left corner; the all-class-1 frame is searched too
TALL_SHAPE = (300, 40)
TALL_SEARCHES = [
    ((20, 150, 15, 120, 0.05), (20, 150, 17, 110, 0.1)),
    ((20, 150, 120, 15, 0.05 + np.pi / 2), (20, 150, 110, 17, 0.1 + np.pi / 2)),
    ((22, 90, 12, 60, -0.05), (22, 90, 10, 66, 0.0)),
    ((5, 260, 15, 100, 0.05), (5, 260, 13, 90, 0.1)),
]


def search_mask(name):
    """bool [H,W] mask of a search case."""
    H, W, what = SEARCHES[name][:3]
    if isinstance(what, str):
        return np.full((H, W), what == "full")
    return render(H, W, tuple(float(v) for v in what))


def search_init(name):
    return np.array(SEARCHES[name][3], np.float64)


@functools.lru_cache(maxsize=None)
def oracle_search(name):
    """(result [5] float64, evaluations) of oracle.fit.fit_ellipse for a search case."""
    with np.errstate(all="ignore"):
        out, nev = ofit.fit_ellipse(search_mask(name), list(search_init(name)), count_evals=True)
    out.setflags(write=False)
    return out, nev


def seed_params(F):
    """float32 [F,10] regression outputs as make_golden.py draws them (centres within +-0.5, axes 0.1..0.5, angle within +-1.5); the
    first frame's two ellipses have theta exactly 0 with a < b and a > b (the two |b| <= 1e-40 branches of mat2param, which a
    non-square frame tells apart)."""
    rng = np.random.RandomState(100 + F)
    p = np.stack([rng.uniform(-.5, .5, 2 * F), rng.uniform(-.5, .5, 2 * F), rng.uniform(.1, .5, 2 * F), rng.uniform(.1, .5, 2 * F),
                  rng.uniform(-1.5, 1.5, 2 * F)], axis=1)
    p[0] = (0.1, -0.2, 0.2, 0.4, 0.0)
    p[1] = (-0.3, 0.1, 0.45, 0.15, 0.0)
    return p.astype(np.float32).reshape(F, 10)
