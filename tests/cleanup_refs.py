"""NumPy restatement of the class-map clean-up (csrc/cleanup.hip; the contract in include/egne_hip.h) and the maps its tests share.
NumPy only.  open3 / largest8 / fill_holes4 / clean_rows follow the contract sentence by sentence; the holes come from a breadth-first
flood from the frame border over frontier arrays, which shares nothing with the kernel's union-find over runs."""
import numpy as np

import mask_seed_refs as M

DEFAULT_LAYERS = ((0b110, 1, 3), (0b100, 2, 3))
SHAPES = ((2, 2), (3, 5), (2, 64), (5, 65), (7, 127), (9, 129), (64, 64), (61, 83), (300, 40), (240, 320))


def _shift(a, dy, dx, fill):
    """out[y, x] = a[y + dy, x + dx], ``fill`` where that lies outside the frame."""
    H, W = a.shape
    out = np.full((H, W), fill, dtype=bool)
    ys, yd = (slice(dy, H), slice(0, H - dy)) if dy >= 0 else (slice(0, H + dy), slice(-dy, H))
    xs, xd = (slice(dx, W), slice(0, W - dx)) if dx >= 0 else (slice(0, W + dx), slice(-dx, W))
    out[yd, xd] = a[ys, xs]
    return out


N4 = ((-1, 0), (1, 0), (0, -1), (0, 1))


def open3(S):
    """The 3x3-cross opening of the bool map S: erosion whose border does not constrain, dilation whose border is background."""
    S = np.asarray(S, dtype=bool)
    E = S.copy()
    for dy, dx in N4:
        E &= _shift(S, dy, dx, True)
    O = E.copy()
    for dy, dx in N4:
        O |= _shift(E, dy, dx, False)
    return O


def eligible(mask, do_open):
    """Pixels that count: ids 0..31, and with ``do_open`` only those that lie in the opening of their own class."""
    m = np.asarray(mask, dtype=np.int64)
    ok = (m >= 0) & (m < 32)
    if not do_open:
        return ok
    out = np.zeros(m.shape, bool)
    for c in np.unique(m[ok]):
        out |= open3(m == c)
    return out


def largest8(R):
    """(K, components): the 8-connected component of R with the most pixels, on a tie the one whose first pixel comes first in raster
    order (labels of components8 ascend in that order; argmax takes the first of equals)."""
    lab = M.components8(R)
    n = int(lab.max())
    if n == 0:
        return np.zeros(lab.shape, bool), 0
    areas = np.bincount(lab.ravel(), minlength=n + 1)[1:]
    return lab == int(np.argmax(areas)) + 1, n


def fill_holes4(K):
    """K and every 4-connected component of its complement that has no pixel in the first or last row or column: a breadth-first
    flood of the complement from the border pixels; what the flood does not reach is a hole."""
    K = np.asarray(K, dtype=bool)
    H, W = K.shape
    Wp = W + 2
    todo = np.zeros((H + 2, Wp), bool)                     # complement pixels the flood has not reached; a wall of False around the frame
    todo[1:-1, 1:-1] = ~K
    edge = np.zeros((H + 2, Wp), bool)
    edge[1, 1:-1] = edge[H, 1:-1] = edge[1:-1, 1] = edge[1:-1, W] = True
    flat = todo.reshape(-1)
    front = np.flatnonzero(todo & edge)
    flat[front] = False
    steps = np.array([-Wp, Wp, -1, 1])
    slot = np.empty(flat.size, np.int64)
    while front.size:
        cand = (front[:, None] + steps[None, :]).reshape(-1)
        cand = cand[flat[cand]]
        slot[cand] = np.arange(cand.size)                  # a pixel reached from two sides: the last writer alone keeps it
        front = cand[slot[cand] == np.arange(cand.size)]
        flat[front] = False
    return K | todo[1:-1, 1:-1]


def clean_rows(mask, frame_of, class_bits, paint_cls, flags, do_open=True, min_area=1, fill_cls=0, cache=None):
    """What egne_class_map_cleanup writes: (out int64 [F,H,W], stats int64 [n,4]).  ``cache``: a dictionary the caller may hand over
    to share the eligibility maps and component searches between calls on the same ``mask``."""
    mask = np.asarray(mask, dtype=np.int64)
    F, H, W = mask.shape
    cache = {} if cache is None else cache
    out = np.full((F, H, W), fill_cls, np.int64)
    stats = np.zeros((len(frame_of), 4), np.int64)
    for i in range(len(frame_of)):
        f, cb, fl = int(frame_of[i]), int(class_bits[i]) & 0xffffffff, int(flags[i])
        if not 0 <= f < F:
            continue
        ek = ("elig", f, bool(do_open))
        if ek not in cache:
            cache[ek] = eligible(mask[f], do_open)
        rk = ("row", f, bool(do_open), cb)
        if rk not in cache:
            R = cache[ek] & M.region_of(mask[f], cb)
            cache[rk] = (R,) + largest8(R)
        R, big, ncomp = cache[rk]
        K = big if fl & 1 else R
        kpx = int(np.count_nonzero(K))
        stats[i, :3] = (np.count_nonzero(R), ncomp, kpx)
        if kpx < min_area or kpx == 0:
            continue
        if fl & 2:
            hk = ("fill", f, bool(do_open), cb, fl & 1)
            if hk not in cache:
                cache[hk] = fill_holes4(K)
            P = cache[hk]
            stats[i, 3] = int(np.count_nonzero(P)) - kpx
        else:
            P = K
        out[f][P] = int(paint_cls[i])
    return out, stats


def layer_rows(layers, F):
    """(frame_of, class_bits, paint_cls, flags) for ``layers`` applied to every one of F frames: row L*f + j is layer j of frame f."""
    L = len(layers)
    return (np.repeat(np.arange(F), L), np.tile([b for b, _, _ in layers], F), np.tile([c for _, c, _ in layers], F),
            np.tile([g for _, _, g in layers], F))


def clean(mask, layers=DEFAULT_LAYERS, do_open=True, min_area=1, fill_cls=0, cache=None):
    """utils.clean_class_maps: (out, stats)."""
    return clean_rows(mask, *layer_rows(layers, mask.shape[0]), do_open=do_open, min_area=min_area, fill_cls=fill_cls, cache=cache)


# ---- maps --------------------------------------------------------------------------------------------------------------------------------
def _place(H, W, block):
    """``block`` one pixel inside the frame where it fits with a margin, else at the corner; None where it does not fit at all."""
    h, w = block.shape
    if h > H or w > W:
        return None
    m = np.zeros((H, W), bool)
    oy, ox = (1 if h + 2 <= H else 0), (1 if w + 2 <= W else 0)
    m[oy:oy + h, ox:ox + w] = block
    return m


def _diag_ring():
    b = np.zeros((5, 5), bool)
    b[0, 1:4] = b[4, 1:4] = b[1:4, 0] = b[1:4, 4] = True          # four sides of three pixels; the corners join them diagonally only
    return b


def extra_patterns(H, W):
    """name -> bool [H,W]: the shapes of holes and joins the filling can get wrong, where they fit the frame."""
    out = {}
    ring = _diag_ring()
    gap = ring.copy(); gap[0, 2] = False                                                          # noqa: E702
    block = np.ones((5, 5), bool); block[1, 1] = False; block[0, 0] = False                         # noqa: E702  hole (1,1), outside (0,0)
    island = np.ones((7, 7), bool); island[1:6, 1:6] = False; island[3, 3] = True                   # noqa: E702
    for name, b in (("diag_ring", ring), ("diag_ring_gap", gap), ("hole_diag_contact", block), ("blob_in_hole", island)):
        m = _place(H, W, b)
        if m is not None:
            out[name] = m
    if min(H // 2, W // 2) >= 5:
        s = np.kron(M._spiral(H // 2, W // 2), np.ones((2, 2), bool)).astype(bool)
        m = np.zeros((H, W), bool)
        m[:s.shape[0], :s.shape[1]] = s
        out["spiral2"] = m
    return out


def class_map(pattern, odd_ids=False):
    """A bool pattern as a class map: class 2 on the pattern, class 0 elsewhere; ``odd_ids``: ids 32, 255 and -1 sprinkled over both."""
    m = np.where(pattern, 2, 0).astype(np.int64)
    if odd_ids:
        H, W = m.shape
        r = np.random.RandomState(H * 7 + W).rand(H, W)
        m[r < 0.04] = 32
        m[(r >= 0.04) & (r < 0.08)] = 255
        m[(r >= 0.08) & (r < 0.12)] = -1
    return m


def maps(H, W):
    """name -> int64 class map [H,W]: the mask-seed patterns, the extra ones, and a noise map with ids outside 0..31 mixed in."""
    pats = dict(M.patterns(H, W))
    pats.update(extra_patterns(H, W))
    out = {name: class_map(p) for name, p in pats.items()}
    out["odd_ids"] = class_map(pats["noise_0.6"], odd_ids=True)
    r = np.random.RandomState(H + W * 1000)
    blobs = (r.rand(H, W) < 0.5)
    out["three_classes"] = np.where(open3(blobs), 2, np.where(r.rand(H, W) < 0.6, 1, 0)).astype(np.int64)
    return out


TEST_ROWS = ((0b100, 2), (0b001, 5))          # the pattern's class painted as 2, the background class painted as 5 over fill_cls 9
