#!/usr/bin/env python3
"""Record what the REFERENCE's data_augment.augment decides in its OpenCV branches (1 blur, 5 glint lines, 6 rotation).

    python tests/golden/make_golden_augment_cv2.py        # writes tests/golden/augment_cv2.npz

OpenCV is not installed, so the stub ``cv2`` module of _ref_shim gets recording stand-ins for GaussianBlur, line,
getRotationMatrix2D and warpAffine.  Everything the reference's own program text decides is then recorded from the reference itself:
order and count of the np.random draws (a hash of the generator's state after the call), the arguments it hands to OpenCV, and the
centre and ellipse parameters it returns (with its quirk that the (-1, -1) centre of an absent ellipse is rotated).
The stand-ins compute the PIXELS with the restatement in tests/augment_cv2_refs.py: the image / mask hashes and rows in the fixture
are restatement-derived, NOT OpenCV's (``pixels_from`` in the file says so).  Runs only where the reference is present; holds none of
its text.
"""
import hashlib
import io
import contextlib
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import _ref_shim  # noqa: E402
import egne_amd  # noqa: E402,F401
from egne_amd import data_augment as DA, synth  # noqa: E402
import augment_cv2_refs as R  # noqa: E402

INTER_NEAREST, INTER_LANCZOS4 = 0, 4         # OpenCV's documented enum values


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


class Recorder:
    def __init__(self):
        self.reset()

    def reset(self):
        self.sigma, self.ksize, self.lines, self.colour, self.thickness = -1, (0, 0), [], [], []
        self.centre, self.angle, self.scale, self.flags, self.dsize = (-1, -1), 0.0, 0.0, [], []

    def GaussianBlur(self, src, ksize, sigma):
        self.ksize, self.sigma = tuple(ksize), int(sigma)
        return R.gaussian_blur(src, sigma)

    def line(self, img, p1, p2, colour, thickness):
        self.lines.append((p1[0], p1[1], p2[0], p2[1]))
        self.colour.append(tuple(colour))
        self.thickness.append(int(thickness))
        return R.draw_lines(img, [(p1[0], p1[1], p2[0], p2[1])])

    def getRotationMatrix2D(self, centre, angle, scale):
        self.centre, self.angle, self.scale = tuple(centre), float(angle), float(scale)
        assert scale == 1.0
        return DA.rotation_matrix(centre, np.deg2rad(angle))

    def warpAffine(self, src, M, dsize, flags):
        self.flags.append(int(flags))
        self.dsize.append(tuple(dsize))
        assert tuple(dsize) == (src.shape[1], src.shape[0])
        return R.warp_affine_lanczos4(src, M) if flags == INTER_LANCZOS4 else R.warp_affine_nearest(src, M)


def main():
    _ref_shim.install()
    rec = Recorder()
    cv2 = sys.modules["cv2"]
    for name in ("GaussianBlur", "line", "getRotationMatrix2D", "warpAffine"):
        setattr(cv2, name, getattr(rec, name))
    cv2.INTER_LANCZOS4, cv2.INTER_NEAREST = INTER_LANCZOS4, INTER_NEAREST
    with contextlib.redirect_stdout(io.StringIO()):
        import data_augment as REF
    # (branch or -1 - branch for a drawn one, synth.augment_case seed, np.random seed); seed 9 has the absent pupil
    cases = [(1, 7, 200), (1, 9, 201), (5, 8, 202), (5, 9, 203), (6, 7, 204), (6, 9, 205)]
    want = {1: 1, 5: 1, 6: 1}
    for s in range(200):
        c = int(np.random.RandomState(s).randint(0, 8))
        if want.get(c, 0) > 0:
            want[c] -= 1
            cases.append((-1 - c, 7 + s % 3, s))
    assert not any(want.values())
    arrs = {"cases": np.array(cases),
            "pixels_from": np.array("tests/augment_cv2_refs.py (restatement of OpenCV's documented behaviour, NOT OpenCV): "
                                    "img_sha, img_rows, mask_sha, mask_rows"),
            "pinned_by_reference": np.array("sigma, ksize, lines, colour, thickness, centre, angle, scale, flags, dsize, pc, el, "
                                            "dtypes, rng")}
    for n, (choice, seed, npseed) in enumerate(cases):
        base, mask, pc, el = synth.augment_case(seed)
        rec.reset()
        np.random.seed(npseed)
        ob, om, opc, (op_, oi) = REF.augment(base.copy(), mask.copy(), pc.copy(), el.copy(), choice=choice if choice >= 0 else None)
        p = "c%d_" % n
        arrs[p + "rng"] = np.array(R.rng_state_hash())
        arrs[p + "sigma"] = np.array(rec.sigma)
        arrs[p + "ksize"] = np.array(rec.ksize)
        arrs[p + "lines"] = np.array(rec.lines, np.int64).reshape(-1, 4)
        arrs[p + "colour"] = np.array(rec.colour, np.int64).reshape(-1, 3)
        arrs[p + "thickness"] = np.array(rec.thickness, np.int64)
        arrs[p + "centre"] = np.array(rec.centre, np.int64)
        arrs[p + "angle"] = np.array(rec.angle, np.float64)
        arrs[p + "scale"] = np.array(rec.scale, np.float64)
        arrs[p + "flags"] = np.array(rec.flags, np.int64)
        arrs[p + "dsize"] = np.array(rec.dsize, np.int64).reshape(-1, 2)
        arrs[p + "pc"] = np.asarray(opc, np.float64)
        arrs[p + "el"] = np.stack([op_, oi]).astype(np.float64)
        arrs[p + "dtypes"] = np.array([str(ob.dtype), str(om.dtype), str(np.asarray(opc).dtype), str(op_.dtype), str(oi.dtype)])
        arrs[p + "img_sha"] = np.array(sha(ob))
        arrs[p + "img_rows"] = ob[::16]
        arrs[p + "mask_sha"] = np.array(sha(om.astype(np.int64)))
        arrs[p + "mask_rows"] = om[::16].astype(np.uint8)
    path = os.path.join(HERE, "augment_cv2.npz")
    np.savez_compressed(path, **arrs)
    print("wrote %s %.1f KB, %d cases" % (path, os.path.getsize(path) / 1024, len(cases)))


if __name__ == "__main__":
    main()
