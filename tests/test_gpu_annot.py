"""-m gpu: label maps from TEyeD annotations (csrc/annot.hip, dataprep.labels_from_annotations): the kernel's maps and status words
equal the NumPy restatement of its rules (tests/annot_refs.py) byte for byte, on the named corner cases of annot_refs.special_frames."""
import numpy as np
import pytest
import torch

import annot_refs as R

pytestmark = pytest.mark.gpu

CANVASES = ((5, 7), (37, 53), (64, 64), (65, 129), (240, 320))        # 64 x 64, 240 x 320: 16-byte stores; the others byte stores
SHAPES = [(r, c, B) for r, c in CANVASES for B in (1, 3, 5)] + [(480, 640, 2)]
FIRST = {s: sum(t[2] for t in SHAPES[:i]) for i, s in enumerate(SHAPES)}          # where a shape starts in the list of cases (wrapping)


@pytest.fixture(autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def test_the_shapes_cover_every_case():
    names = set()
    for (r, c, B), first in FIRST.items():
        names |= set(R.case_records(r, c, B, first)[0])
    assert names == {f[0] for f in R.special_frames(48, 64)}


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d_B%d" % s)
def test_kernel_equals_the_restatement(shape):
    from egne_amd import dataprep
    r, c, B = shape
    names, rec = R.case_records(r, c, B, FIRST[shape])
    other = R.case_records(r, c, B, FIRST[shape] + 7)[1]
    dev = torch.device("cuda", torch.cuda.current_device())
    bufs = [torch.full((B, r, c), 77, dtype=torch.int8, device=dev) for _ in range(2)]
    for hw in (None, R.ragged_hw(r, c, B)):
        want_ns, want_sk, want_st = R.paint(rec, r, c, hw)
        # new buffers, both maps
        (ns, sk), st = dataprep.labels_from_annotations(rec, (r, c), src_hw=hw, with_skin=True, return_status=True)
        assert ns.dtype == torch.int8 and tuple(ns.shape) == (B, r, c) and st.dtype == torch.int32
        assert np.array_equal(ns.cpu().numpy(), want_ns), names
        assert np.array_equal(sk.cpu().numpy(), want_sk), names
        assert np.array_equal(st.cpu().numpy(), want_st), (names, st.cpu().numpy(), want_st)
        # twice into the same buffers: other records first, then these -- nothing of the first run stays
        dataprep.labels_from_annotations(other, (r, c), src_hw=hw, with_skin=True, out=bufs)
        (ns2, sk2), st2 = dataprep.labels_from_annotations(torch.from_numpy(rec).to(dev), (r, c), src_hw=hw, with_skin=True, out=bufs, return_status=True)
        assert ns2 is bufs[0] and sk2 is bufs[1]
        assert np.array_equal(ns2.cpu().numpy(), want_ns) and np.array_equal(sk2.cpu().numpy(), want_sk) and np.array_equal(st2.cpu().numpy(), want_st)
        # Masks_noSkin alone
        only, st3 = dataprep.labels_from_annotations(rec, (r, c), src_hw=hw, with_skin=False, out=bufs[1], return_status=True)
        assert only is bufs[1] and np.array_equal(only.cpu().numpy(), want_ns) and np.array_equal(st3.cpu().numpy(), want_st)
        assert np.array_equal(bufs[0].cpu().numpy(), want_ns)          # (the other buffer is not touched)


def test_an_empty_frame_sets_its_status_bit():
    from egne_amd import dataprep
    names, rec = R.case_records(37, 53, len(R.special_frames(37, 53)), 0)
    (ns, sk), st = dataprep.labels_from_annotations(rec, (37, 53), return_status=True)
    st, ns = st.cpu().numpy(), ns.cpu().numpy()
    empty = (st & dataprep.ANNOT_EMPTY) != 0
    assert np.array_equal(empty, ~ns.reshape(len(rec), -1).any(1))
    assert {n for n, e in zip(names, empty) if e} == {"wholly_outside", "absent_all"}
    zero = {n for n, s in zip(names, st) if s & (dataprep.ANNOT_IRIS_ZERO_AXIS | dataprep.ANNOT_PUPIL_ZERO_AXIS)}
    assert zero == {"zero_axes"} and st[names.index("zero_axes")] & 3 == 3


def test_packing_limit_is_refused_before_any_launch():
    from egne_amd import dataprep
    ball, iris, pupil, lid = R.seeded_annotations(2, 3, 48, 64)
    for field, at, v in ((0, (1, 1), 2.0 ** 20 + 1), (1, (0, 2), -2.0 ** 20 - 0.5), (2, (1, 4), 2.0 ** 21 + 2), (3, (0, 7, 0), 3e6)):
        rows = [ball.copy(), iris.copy(), pupil.copy(), lid.copy()]
        rows[field][at] = v
        with pytest.raises(ValueError, match="2\\*\\*20"):
            dataprep.pack_annotations(*rows)
    with pytest.raises(ValueError):
        dataprep.labels_from_annotations(np.zeros((2, 149), np.int32), (8, 8))
    L = dataprep._lib.lib()
    assert L.egne_labels_from_annotations(256, None, 1, 0, 8, 256, None, 256, None) != 0          # refused by the entry point: no launch
    assert b"canvas" in L.egne_last_error()
