#!/usr/bin/env python3
"""Record five frames of the REFERENCE's example video as they lie in the file, for the device Motion-JPEG decoder's tests.

    python tests/golden/make_golden_mjpeg_frames.py [path/to/videos/example1.avi]     # writes tests/golden/mjpeg_example_frames.npz

The fixture holds the raw JPEG byte strings of frames 0, 1, 100, 225 and 450 (the SOI/EOI scan of evaluate.mjpeg_chunks): data the
reference's programs read, none of its text.  Runs only where the reference is present.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

import egne_amd  # noqa: E402,F401
from egne_amd import evaluate as E  # noqa: E402

FRAMES = (0, 1, 100, 225, 450)


def main():
    video = sys.argv[1] if len(sys.argv) > 1 else os.path.join(os.path.dirname(ROOT), "reference", "videos", "example1.avi")
    arrs = {}
    for k, chunk in enumerate(E.mjpeg_chunks(video)):
        if k in FRAMES:
            arrs["frame_%d" % k] = np.frombuffer(chunk, np.uint8)
    assert len(arrs) == len(FRAMES), sorted(arrs)
    path = os.path.join(HERE, "mjpeg_example_frames.npz")
    np.savez(path, **arrs)
    print("wrote %s %.1f KB" % (path, os.path.getsize(path) / 1024))


if __name__ == "__main__":
    main()
