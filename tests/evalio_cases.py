"""Inputs and host comparators shared by tests/test_gpu_evalio.py and tests/test_host_evalio.py: the source geometries of the device
front / back end of evaluate.py and the existing host path they are pinned against."""
import numpy as np

from common import gold

OP_SHAPE = (240, 320)
TIE = 1e-9          # a float64 pre-rounding value closer than this to a half-integer is not held to either neighbour


def native_frames(n):
    """n frames of 640 x 240 (two eyes of 320 columns): the fixture pairs first, then seeded random frames."""
    eyes = gold("evaluate_real_frames")["eyes"]
    rng = np.random.RandomState(0)
    fr = [np.concatenate([eyes[0], eyes[1]], axis=1), np.concatenate([eyes[2], eyes[3]], axis=1)]
    while len(fr) < n:
        fr.append(rng.randint(0, 256, (240, 640)).astype(np.uint8))
    return np.stack(fr[:n])


def resize_cases():
    """name -> (frames uint8 [N,Hs,Ws], eyes, eye_width): what each exercises is in the name."""
    eyes = gold("evaluate_real_frames")["eyes"]
    rng = np.random.RandomState(1)
    big = np.kron(eyes[2], np.ones((2, 2), np.uint8))                                  # 480 x 640: downscale by 2
    return {
        "down2": (np.stack([np.concatenate([big, big[:, ::-1]], axis=1)]), 2, 640),
        "pad48": (rng.randint(0, 256, (2, 240, 800)).astype(np.uint8), 2, 400),        # -> 192 x 320 + 48 rows of padding
        "single_eye": (np.concatenate([eyes[0], eyes[1]], axis=1)[None], 1, 640),      # -> 120 x 320 + 120 rows of padding
        # centre crop of 60 rows, no resize; 3 columns beyond the eyes and a width that is no multiple of 4 (scalar kernels)
        "crop60": (rng.randint(0, 256, (2, 300, 643)).astype(np.uint8), 2, 320),
    }


def table_geometries():
    """(n1, n2) of every Lanczos pass the cases above run."""
    return [(480, 240), (640, 320), (240, 192), (400, 320), (240, 120)]


def host_u8(E, grey, op_shape=OP_SHAPE):
    """preprocess_frame up to the z-score: (uint8 image after resize / pad / crop, float64 pre-rounding values of the resize or None)."""
    pre = None
    img = grey
    if op_shape[1] != img.shape[1]:
        sc = op_shape[1] / img.shape[1]
        dsize = (int(img.shape[1] * sc), int(img.shape[0] * sc))
        pre = E.resize_lanczos4(img.astype(np.float64), dsize)
        img = E.resize_lanczos4(img, dsize)
    if op_shape[0] > img.shape[0]:
        pad = op_shape[0] - img.shape[0]
        img = np.pad(img, ((pad // 2, pad - pad // 2), (0, 0)))
    elif op_shape[0] < img.shape[0]:
        cut = img.shape[0] - op_shape[0]
        img = img[cut // 2: cut // 2 + op_shape[0]]
    return img, pre


def near_half(v):
    """Boolean mask: within TIE of a half-integer."""
    return np.abs((v - np.floor(v)) - 0.5) < TIE


def host_render(E, frames, eyes, ew, edge, seg, fit, ss):
    """The back end of evaluate.py's draw() for a batch: (overlay, edge frame [N,Hs,Ws,3] uint8, ellipses [N*eyes,2,5] float64 (iris,
    pupil)) from host arrays, with the host functions."""
    N = frames.shape[0]
    ov, ef, ell = [], [], np.zeros((N * eyes, 2, 5))
    for n in range(N):
        bgr = np.stack([frames[n]] * 3, axis=2)
        overlay, edge_frame = bgr.copy(), bgr.copy()
        for i in range(eyes):
            k = n * eyes + i
            grey = frames[n][:, ew * i: ew * (i + 1)]
            em = 255.0 - 255.0 * edge[k]
            sm, p, q, em = E.rescale_to_original(seg[k], fit[k, 1], fit[k, 0], ss, grey.shape, edge_map=em)
            ell[k, 0], ell[k, 1] = q, p
            overlay[:, ew * i: ew * (i + 1)] = E.plot_segmap_ellpreds(grey, sm, p, q)
            edge_frame[:, ew * i: ew * (i + 1)] = np.clip(em, 0, 255).astype(np.uint8)[..., None]
        ov.append(overlay)
        ef.append(edge_frame)
    return np.stack(ov), np.stack(ef), ell


def outline_ties(el, shape):
    """Samples of _draw_ellipse(el) whose pre-rounding coordinate is within TIE of a half-integer: (count, boolean pixel mask [H,W]
    of every pixel such a sample could be rounded to)."""
    mask = np.zeros(shape, bool)
    if np.all(np.asarray(el) == -1) or not np.all(np.isfinite(el)):
        return 0, mask
    cx, cy, a, b = (int(v) for v in el[:4])
    t = np.linspace(0, 2 * np.pi, 720, endpoint=False)
    ang = float(el[4])
    x = cx + a * np.cos(t) * np.cos(ang) - b * np.sin(t) * np.sin(ang)
    y = cy + a * np.cos(t) * np.sin(ang) + b * np.sin(t) * np.cos(ang)
    tie = near_half(x) | near_half(y)
    for xv, yv in zip(x[tie], y[tie]):
        for yy in (int(np.floor(yv)), int(np.ceil(yv))):
            for xx in (int(np.floor(xv)), int(np.ceil(xv))):
                if 0 <= yy < shape[0] and 0 <= xx < shape[1]:
                    mask[yy, xx] = True
    return int(tie.sum()), mask


def handmade_maps(n_eyes, seed=3):
    """Class maps, edge maps and ellipses at network geometry as tests/test_host_cpu.py::test_evaluate_front_and_back_end makes them:
    rectangles of class 1 and 2, edge values beyond [0, 1] too, ellipses partly outside the crop, one all -1, one with a NaN."""
    rng = np.random.RandomState(seed)
    H, W = OP_SHAPE
    seg = np.zeros((n_eyes, H, W), np.int64)
    edge = (rng.rand(n_eyes, H, W) * 1.4 - 0.2).astype(np.float32)
    pats = [
        ([150.3, 118.7, 95.2, 70.9, 0.2], [152.8, 121.1, 30.6, 24.2, 0.3]),
        ([300.5, 30.2, 60.7, 40.3, 0.3], [20.4, 200.9, 50.1, 45.6, 0.2]),           # partly outside the crop
        ([-1.0] * 5, [160.2, 120.6, 20.3, 10.8, 0.3]),                              # iris absent
        # integer centre, EVEN integer axes, no rotation: the samples at multiples of 30 degrees land on integers, none on a tie (odd
        # axes put a * cos(60 deg) on a half-integer); pupil not finite
        ([150.0, 120.0, 56.0, 36.0, 0.0], [150.0, np.nan, 12.0, 9.0, 0.0]),
        ([160.9, 4.2, 120.5, 80.7, 0.2], [310.1, 235.4, 14.9, 12.2, 0.3]),
    ]
    fit = np.zeros((n_eyes, 2, 5))
    for k in range(n_eyes):
        y0, x0 = 60 + 7 * (k % 5), 80 + 11 * (k % 7)
        seg[k, y0:y0 + 90, x0:x0 + 140] = 1
        seg[k, y0 + 25:y0 + 60, x0 + 40:x0 + 90] = 2
        seg[k, 0:3, 0:5] = 2                 # the first and last rows / columns: padding and cropping show there
        seg[k, H - 2:, W - 4:] = 1
        fit[k, 0], fit[k, 1] = pats[k % len(pats)]
    return seg, edge, fit
