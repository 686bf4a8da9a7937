"""NumPy restatement of csrc/mask_seed.hip (ellipse seeds from the class map) and the masks its tests share.  NumPy only.

components8 / seed_stats are exact integer work; seed_from_stats is the float64 block of the kernel's last launch, line for line."""
import math

import numpy as np

DEFAULT_REGIONS = ((0b110, 1), (0b100, 2))
SHAPES = ((240, 320), (61, 83), (300, 40), (65, 129), (64, 64), (3, 5), (2, 2))


def components8(region):
    """Labels int32 [H,W] of the 8-connected components of the bool map ``region``: 0 outside, 1.. in raster order of each component's
    first pixel.  Two passes: runs of every row joined (union-find) to the runs of the row above that they touch, then renumbered."""
    region = np.asarray(region, dtype=bool)
    H, W = region.shape
    parent, runs, prev = [], [], []                      # runs: (row, first column, last column, id)
    def find(a):
        while parent[a] != a:
            parent[a] = parent[parent[a]]
            a = parent[a]
        return a
    for y in range(H):
        row = np.concatenate(([False], region[y], [False]))
        edges = np.flatnonzero(row[1:] != row[:-1])
        cur, j = [], 0
        for x0, x1 in zip(edges[0::2], edges[1::2] - 1):
            k = len(parent)
            parent.append(k)
            while j < len(prev) and prev[j][1] < x0 - 1:  # both lists ascend: runs that end left of this one end left of the next too
                j += 1
            for i in range(j, len(prev)):
                px0, px1, pk = prev[i]
                if px0 > x1 + 1:
                    break
                a, b = find(k), find(pk)                  # touches, diagonals included
                if a != b:
                    parent[max(a, b)] = min(a, b)
            cur.append((int(x0), int(x1), k))
            runs.append((y, int(x0), int(x1), k))
        prev = cur
    labels = np.zeros((H, W), np.int32)
    number = {}
    for y, x0, x1, k in runs:                            # runs are in raster order: a root is numbered at its component's first pixel
        r = find(k)
        if r not in number:
            number[r] = len(number) + 1
        labels[y, x0:x1 + 1] = number[r]
    return labels


def seed_stats(region, min_area):
    """The eight int64 values of a row: (N, Sx, Sy, Sxx, Sxy, Syy) over the largest component (tie: raster-first), the number of
    components, the pixels of the region.  The six sums are 0 when that component has fewer than ``min_area`` pixels (or none)."""
    region = np.asarray(region, dtype=bool)
    lab = components8(region)
    ncomp = int(lab.max())
    out = np.zeros(8, np.int64)
    out[6], out[7] = ncomp, int(np.count_nonzero(region))
    if ncomp == 0:
        return out
    areas = np.bincount(lab.ravel(), minlength=ncomp + 1)[1:]
    best = int(np.argmax(areas)) + 1                      # argmax: the first of equal areas = the lowest label = raster-first
    N = int(areas[best - 1])
    if N < min_area or N == 0:
        return out
    y, x = np.nonzero(lab == best)
    x, y = x.astype(np.int64), y.astype(np.int64)
    out[:6] = (N, x.sum(), y.sum(), (x * x).sum(), (x * y).sum(), (y * y).sum())
    return out


def seed_from_stats(stats, H, W):
    """(cx, cy, a, b, theta) float64 from a row's eight values; -1 five times for an absent row (N = 0)."""
    N, Sx, Sy, Sxx, Sxy, Syy = (int(v) for v in stats[:6])
    if N == 0:
        return np.full(5, -1.0)
    Ixx = N * Sxx - Sx * Sx; Iyy = N * Syy - Sy * Sy; Ixy = N * Sxy - Sx * Sy            # noqa: E702
    Jxx = 12 * Ixx + N * N; Jyy = 12 * Iyy + N * N; Jxy = 12 * Ixy                       # noqa: E702
    assert max(abs(v) for v in (N * Sxx, N * Syy, N * Sxy, Sx * Sx, Sy * Sy, Sx * Sy, Jxx, Jyy, Jxy)) < 2 ** 62
    n = float(N); d12 = 12.0 * n * n; sx = float(W) / (W - 1); sy = float(H) / (H - 1)   # noqa: E702
    mxx = (float(Jxx) / d12) * (sx * sx); myy = (float(Jyy) / d12) * (sy * sy); mxy = (float(Jxy) / d12) * (sx * sy)   # noqa: E702
    cx = (float(Sx) / n) * sx; cy = (float(Sy) / n) * sy                                 # noqa: E702
    d = mxx - myy; r = math.sqrt(d * d + 4.0 * mxy * mxy)                                # noqa: E702
    a = 2.0 * math.sqrt((mxx + myy + r) / 2.0)
    b = 2.0 * math.sqrt(max((mxx + myy - r) / 2.0, 0.0))
    theta = 0.5 * math.atan2(2.0 * mxy, d)
    return np.array([cx, cy, a, b, theta], dtype=np.float64)


def region_of(mask, class_bits):
    """Pixels whose class id (0..31 only) has its bit set in ``class_bits``."""
    m = np.asarray(mask, dtype=np.int64)
    ok = (m >= 0) & (m < 32)
    return ok & (((int(class_bits) >> np.where(ok, m, 0)) & 1) == 1)


def seeds_rows(mask, frame_of, class_bits, search_cls, min_area):
    """What egne_ellipse_init_from_mask writes for arbitrary rows: (init [n,5], out_frame_of [n], out_cls [n], stats [n,8])."""
    F, H, W = mask.shape
    n = len(frame_of)
    init, fo, stats = np.full((n, 5), -1.0), np.full(n, -1, np.int32), np.zeros((n, 8), np.int64)
    for i in range(n):
        f = int(frame_of[i])
        if not 0 <= f < F or int(class_bits[i]) == 0:
            continue
        stats[i] = seed_stats(region_of(mask[f], class_bits[i]), min_area)
        if stats[i, 0] > 0:
            init[i], fo[i] = seed_from_stats(stats[i], H, W), f
    return init, fo, np.asarray(search_cls, np.int32).copy(), stats


def seeds(mask, regions=DEFAULT_REGIONS, min_area=7):
    """For a batch [F,H,W] and ``regions`` per frame: row R*f + r is region r of frame f.  Same returns as seeds_rows."""
    F, R = mask.shape[0], len(regions)
    return seeds_rows(mask, np.repeat(np.arange(F), R), np.tile([b for b, _ in regions], F).astype(np.int64),
                      np.tile([c for _, c in regions], F), min_area)


# ---- masks ---------------------------------------------------------------------------------------------------------------------------
def _spiral(H, W):
    m = np.zeros((H, W), bool)
    y = x = 0
    dy, dx = 0, 1
    m[0, 0] = True
    turned = False
    for _ in range(2 * H * W):
        ny, nx, ay, ax = y + dy, x + dx, y + 2 * dy, x + 2 * dx
        if 0 <= ny < H and 0 <= nx < W and not m[ny, nx] and not (0 <= ay < H and 0 <= ax < W and m[ay, ax]):
            y, x, turned = ny, nx, False
            m[y, x] = True
        elif turned:
            break
        else:
            dy, dx, turned = dx, -dy, True
    return m


def patterns(H, W, min_area=7):
    """name -> bool [H,W] for every pattern that fits the shape."""
    yy, xx = np.mgrid[0:H, 0:W]
    z = lambda: np.zeros((H, W), bool)                      # noqa: E731
    out = {"empty": z(), "full": np.ones((H, W), bool), "checkerboard": (yy + xx) % 2 == 0}
    m = z(); m[H // 2, W // 3] = True; out["one_pixel"] = m                                   # noqa: E702
    bh, bw = max(1, H // 4), max(1, W // 5)
    if H - bh > bh and W - bw > bw:
        m = z(); m[H - bh:, :bw] = True; m[:bh, W - bw:] = True; out["two_equal_blobs"] = m   # noqa: E702  (the top-right one comes first)
    m = z(); m[:H // 2, :W // 2] = True; m[H // 2:, W // 2:] = True; out["diagonal_join"] = m  # noqa: E702
    if W >= 3:
        m = z(); m[:, ::2] = True; m[H - 1, :] = True; out["comb"] = m                        # noqa: E702
    if min(H, W) >= 5:
        out["spiral"] = _spiral(H, W)
    if min(H, W) >= 40:
        cy, cx, s = (H - 1) / 2.0, (W - 1) / 2.0, float(min(H, W))
        rr = np.hypot(yy - cy, xx - cx)
        out["ring_with_blob"] = ((rr <= 0.45 * s) & (rr >= 0.32 * s)) | (rr <= 0.12 * s)
    if W > 64 or H > 256:                                   # a component across column 63 / 64 and, where the shape has it, row 255 / 256
        m = z()
        if W > 64:
            m[H // 3: H // 3 + 3, 60:69] = True
        if H > 256:
            m[250:263, 2:6] = True
        out["straddle"] = m
    m = z(); m[0, :] = True; m[H - 1, :] = True; m[:, 0] = True; m[:, W - 1] = True; out["borders"] = m   # noqa: E702
    for p in (0.4, 0.6):
        out["noise_%g" % p] = np.random.RandomState(H * 1000 + W + int(p * 10)).rand(H, W) < p
    if H * W >= min_area:
        bw = min(W, 4)
        for k in (min_area - 1, min_area):
            m = z()
            for i in range(k):
                m[i // bw, i % bw] = True
            out["area_%d" % k] = m
    return out


def _cases():
    out = {}
    for H, W in SHAPES:
        for name, m in patterns(H, W).items():
            out["%dx%d_%s" % (H, W, name)] = (H, W, m.astype(np.int64))
    return out


CASES = _cases()            # name -> (H, W, int64 mask: 1 inside the region, 0 outside)


# ---- the drawn ellipses of the recovery test -------------------------------------------------------------------------------------------
def drawn_ellipses(n=12, H=240, W=320):
    """[(true ellipse (cx, cy, a, b, theta), clean bool mask, mask with a 7x9 stray blob and a stray pixel)]: RandomState(0), centres
    100..220 / 80..160, a 12..60, b/a 0.5..0.95, angles +-80 degrees, rasterised by the oracle of the search (oracle.fit.ell_inside)."""
    from oracle import fit as ofit
    rng = np.random.RandomState(0)
    mesh = ofit.mesh_f32(H, W)
    out = []
    for _ in range(n):
        cx, cy = rng.uniform(100, 220), rng.uniform(80, 160)
        a = rng.uniform(12, 60)
        b = a * rng.uniform(0.5, 0.95)
        th = np.deg2rad(rng.uniform(-80, 80))
        clean = np.array(ofit.ell_inside((H, W), [cx, cy, a, b, th * 180.0 / ofit.PI_REF], mesh))
        dirty = clean.copy()
        by, bx = (4, 6) if cy > H / 2 else (H - 12, W - 16)          # a corner the ellipse (a <= 60 around the centre ranges) cannot reach
        dirty[by:by + 7, bx:bx + 9] = True
        dirty[H - 2 if cy <= H / 2 else 1, 2] = True
        out.append((np.array([cx, cy, a, b, th]), clean, dirty))
    return out
