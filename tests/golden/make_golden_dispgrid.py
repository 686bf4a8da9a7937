#!/usr/bin/env python3
"""Record what the REFERENCE's generateImageGrid (utils.py:206-399) computes on the seeded cases of tests/dispgrid_refs.py.

    python tests/golden/make_golden_dispgrid.py        # writes tests/golden/dispgrid.npz

OpenCV, scikit-image and torchvision are not installed, so the stub modules of _ref_shim get recording stand-ins for
cv2.equalizeHist, skimage.draw.ellipse_perimeter and torchvision.utils.make_grid; each calls the restatement of tests/dispgrid_refs.py
(include/egne_hip.h states its rules).  The reference's own program text then runs around them.

Pinned by the reference (``pinned_by_reference`` in the file): the uint8 array handed to equalizeHist; the four integers and the
orientation handed to ellipse_perimeter, per ellipse; and through the final grid both normalisations, the colours, the order of the
paints, the clip, min(4, B), the cond / override rule and the casts.  NOT pinned (``pixels_from``): the equalised pixels, the outline
pixels and the layout -- they come from the stand-ins.

The float32 ellipses are widened to float64 BEFORE the reference sees them, which is what egne_ellipse_init_from_pred does; handed
float32 arrays, the reference's param2mat rounds 1 / a ** 2 and the rotation's cos / sin to float32, and that is not reproduced
(make_golden_ellipse_scores.py has the same note).  The 240 x 320 case is stored as the uint8 form plus a hash of the float grid.

Runs only where the reference is present; holds none of its text, and the file it writes holds data only.
"""
import contextlib
import io
import os
import sys
import warnings

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import _ref_shim  # noqa: E402
import dispgrid_refs as R  # noqa: E402


class Recorder:
    def __init__(self):
        self.u8, self.perim, self.grids = [], [], []

    def equalizeHist(self, u):
        assert u.dtype == np.uint8 and u.ndim == 2
        self.u8.append(u.copy())
        return R.equalize(u)

    def ellipse_perimeter(self, r, c, r_radius, c_radius, orientation=0, shape=None):
        assert all(isinstance(v, int) for v in (r, c, r_radius, c_radius)) and shape is None
        self.perim.append((r, c, r_radius, c_radius, float(orientation)))
        return R.perimeter(r, c, r_radius, c_radius, orientation)

    def make_grid(self, t, nrow=8, **kw):
        assert not kw and t.dtype == torch.float32 and t.dim() == 4
        self.grids.append(tuple(t.shape))
        return torch.from_numpy(R.make_grid(t.numpy(), nrow))


def main():
    _ref_shim.install()
    with contextlib.redirect_stdout(io.StringIO()):
        import utils as U
    rec = Recorder()
    U.cv2.equalizeHist = rec.equalizeHist
    U.draw.ellipse_perimeter = rec.ellipse_perimeter
    U.make_grid = rec.make_grid
    warnings.simplefilter("ignore", category=RuntimeWarning)
    arrs = {"pixels_from": np.array("tests/dispgrid_refs.py, NOT OpenCV / scikit-image / torchvision: the equalised pixels (equalize: "
                                    "OpenCV's published rule), the outline pixels (perimeter: evaluate._draw_ellipse's 720 samples) and "
                                    "the layout (make_grid: torchvision's documented one)"),
            "pinned_by_reference": np.array("<case>_u8 (handed to equalizeHist), <case>_perimeter_args (r, c, r_radius, c_radius, "
                                            "orientation per ellipse, in call order), and through <case>_grid / _grid_sha both "
                                            "normalisations, the colours, the paint order, the clip, min(4, B), the cond / override rule "
                                            "and the casts")}
    for name, (B, H, W, seed, override, leave) in R.FIXTURE_CASES.items():
        inp, override = R.fixture_inputs(name)
        rec.u8, rec.perim, rec.grids = [], [], []
        with contextlib.redirect_stdout(io.StringIO()) as said:
            g = U.generateImageGrid(inp["img"], inp["mask"], inp["el"].astype(np.float64), None, inp["cond"], inp["el_gt"].astype(np.float64),
                                    override=override)
        assert "Warning" not in said.getvalue(), (name, said.getvalue())
        g = g.numpy()
        n = min(4, B)
        assert g.dtype == np.float32 and g.shape == (3,) + R.grid_shape(n, 4, H, W) and rec.grids == [(n, 3, H, W)]
        assert len(rec.u8) == n
        # the restatement gives the same grid, from its own uint8 arrays and its own integers
        want, want_u8, status = R.image_grid(inp["img"], inp["mask"], inp["el"], inp["cond"], inp["el_gt"], override=override)
        assert np.array_equal(want.view(np.uint32), g.view(np.uint32)), name
        assert not status.any(), (name, status)
        for i in range(n):
            assert np.array_equal(R.frame_u8(inp["img"][i])[0], rec.u8[i]), (name, i)
        p = name + "_"
        arrs[p + "u8"] = np.stack(rec.u8)
        arrs[p + "perimeter_args"] = np.array(rec.perim, np.float64).reshape(-1, 5)
        arrs[p + "grid_sha"] = np.array(R.sha(g))
        arrs[p + "grid_u8"] = want_u8
        if name not in R.HASHED:
            arrs[p + "grid"] = g
        arrs[p + "inputs_sha"] = np.array(R.sha(np.concatenate([inp[k].astype(np.float64).ravel() for k in ("img", "mask", "el", "el_gt", "cond")])))
        if leave:       # the clip rule bites: some outline pixel of the case lies outside the frame before the clip
            out = [np.any((rr < 0) | (rr >= H) | (cc < 0) | (cc >= W)) for rr, cc in (R.perimeter(*a) for a in rec.perim)]
            assert any(out), name
        vals = np.unique(g)
        assert np.all((vals == 255) | (vals == 102) | ((vals >= 0) & (vals <= 1)))
        print("%s: B %d, %dx%d, override %s: grid %s, %d perimeter calls" % (name, B, H, W, override, g.shape, len(rec.perim)))
    path = os.path.join(HERE, "dispgrid.npz")
    np.savez_compressed(path, **arrs)
    print("wrote %s %.1f KB" % (path, os.path.getsize(path) / 1024))


if __name__ == "__main__":
    main()
