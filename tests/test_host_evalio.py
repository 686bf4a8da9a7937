"""Host side of evaluate.py --device_io (no GPU): the flag, the Lanczos tap tables handed to the device, the shape arithmetic."""
import numpy as np

import egne_amd  # noqa: F401
from evalio_cases import OP_SHAPE, resize_cases, table_geometries


def test_device_io_flag_defaults_to_the_host_path():
    from egne_amd import evaluate as E
    assert E.parse_args([]).device_io == 0
    assert E.parse_args(["--device_io", "1"]).device_io == 1
    assert E.parse_args(["--device_io", "1", "--low_latency", "1"]).low_latency == 1
    assert E.parse_args([]).eye_width == 320


def test_lanczos_tables_are_resize_lanczos4s_own():
    """The cached tables equal the indices and weights resize_lanczos4 builds internally, to the bit: its response to unit impulses
    (float64 in, float64 out: no rounding) is the tables applied with the same NumPy expression, and the closed formula agrees."""
    from egne_amd import evaluate as E
    for n1, n2 in table_geometries():
        idx, w = E.lanczos4_table(n1, n2)
        assert idx.shape == (n2, 8) and idx.dtype == np.int32 and w.shape == (n2, 8) and w.dtype == np.float64
        assert idx.min() == 0 and idx.max() == n1 - 1
        assert E.lanczos4_table(n1, n2)[1] is w                                           # cached per (n1, n2)
        # the function's own expressions, restated
        pos = (np.arange(n2) + 0.5) * (n1 / n2) - 0.5
        base = np.floor(pos).astype(np.int64)
        x = (pos - base)[:, None] - np.arange(-3, 5)[None, :]
        with np.errstate(invalid="ignore", divide="ignore"):
            ref = np.where(np.abs(x) < 1e-12, 1.0, np.sin(np.pi * x) * np.sin(np.pi * x / 4) / (np.pi * np.pi * x * x / 4))
        ref = np.where(np.abs(x) < 4, ref, 0.0)
        ref /= ref.sum(1, keepdims=True)
        assert np.array_equal(w, ref)
        assert np.array_equal(idx, np.clip(base[:, None] + np.arange(-3, 5)[None, :], 0, n1 - 1))
        # what the function itself does with them, along either axis
        eye = np.eye(n1)
        want = (eye[idx] * w[..., None]).sum(1)
        assert np.array_equal(E.resize_lanczos4(eye, (n1, n2)), want)                     # rows resized
        cols = np.take(eye, idx.reshape(-1), axis=1).reshape(n1, n2, 8)                   # C-contiguous: NumPy sums its last axis pairwise
        assert np.array_equal(E.resize_lanczos4(eye, (n2, n1)), (cols * w[None]).sum(2))  # columns resized


def test_prep_geometry_is_preprocess_frames_arithmetic():
    from egne_amd import evaluate as E
    for name, (frames, eyes, ew) in resize_cases().items():
        grey = frames[0][:, :ew]
        t, ss = E.preprocess_frame(grey, OP_SHAPE)
        Hr, Wr, ss2 = E.prep_geometry(grey.shape, OP_SHAPE)
        assert ss2 == ss and type(ss2[0]) is type(ss[0]) and Wr == OP_SHAPE[1], name
    assert E.prep_geometry((240, 320), OP_SHAPE) == (240, 320, (1, 0))
