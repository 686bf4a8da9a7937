"""-m gpu: the two archive kinds give the same batch.  One set of seeded frames and annotations goes through make_archive twice:
--store masks (label planes rasterised by the tool, served by RawArchive, uploaded per batch) and --store annotations (served by
AnnotationArchive, painted on the device per batch); loader.device_batch of the two batches gives nine bit-equal tensors."""
import numpy as np
import pytest
import torch

import annot_refs as R

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _archives(tmp, tag, n, r, c, seed, empty=None):
    """(RawArchive, AnnotationArchive) of n seeded frames of r x c, written by the tool; frame ``empty`` paints nothing."""
    from egne_amd import loader, make_archive
    ball, iris, pupil, lid = R.seeded_annotations(n, seed, r, c)
    if empty is not None:          # accepted by annotation_keep (nothing is negative), but every shape lies beyond the frame
        ball[empty, 1:] += 50 * c
        iris[empty, 1:3] += 50 * c
        pupil[empty, 1:3] += 50 * c
    frames = R.write_frame_dir(str(tmp / (tag + "_frames")), R.seeded_frames(n, r, c, seed + 1))
    prefix = str(tmp / (tag + ".mp4"))
    R.write_annotation_files(prefix, ball, iris, pupil, lid)
    paths = {}
    for store in ("masks", "annotations"):
        paths[store] = str(tmp / ("%s_%s.npz" % (tag, store)))
        make_archive.main(["--frames", frames, "--annotations", prefix, "--out", paths[store], "--store", store, "--batch", "2"])
    raw, ann = loader.open_archive(paths["masks"]), loader.open_archive(paths["annotations"])
    assert isinstance(raw, loader.RawArchive) and isinstance(ann, loader.AnnotationArchive) and len(raw) == len(ann) == n
    return raw, ann


def _same(a, b):
    assert len(a) == len(b) == 9
    for k, (x, y) in enumerate(zip(a, b)):
        assert x.dtype == y.dtype and x.shape == y.shape, k
        assert torch.equal(x.view(torch.int32) if x.dtype == torch.float32 else x, y.view(torch.int32) if y.dtype == torch.float32 else y), k


@pytest.fixture(scope="module")
def mixed(tmp_path_factory):
    """B = 5 samples of two source sizes in one batch; sample 3 paints nothing."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from egne_amd import loader
    tmp = tmp_path_factory.mktemp("annot_loader")
    raw_a, ann_a = _archives(tmp, "a", 3, 120, 160, 40)
    raw_b, ann_b = _archives(tmp, "b", 2, 236, 316, 50, empty=1)
    order = ((0, 0), (1, 0), (0, 1), (1, 1), (0, 2))
    raws, anns = (raw_a, raw_b), (ann_a, ann_b)
    return loader.collate_raw([raws[s][i] for s, i in order]), loader.collate_annotated([anns[s][i] for s, i in order])


def test_plain_batches_are_bit_equal(mixed):
    from egne_amd import loader
    rb, ab = mixed
    assert isinstance(ab, loader.AnnotBatch) and np.array_equal(rb.images, ab.images) and np.array_equal(rb.src_hw, ab.src_hw)
    assert rb.labels.any(axis=(1, 2)).tolist() == [True, True, True, False, True]
    out_r, out_a = loader.device_batch(rb, augment=False), loader.device_batch(ab, augment=False)
    _same(out_r, out_a)
    assert tuple(out_a[1].shape) == (5, 240, 320) and set(torch.unique(out_a[1]).tolist()) == {0, 1, 2}


def test_cond1_is_the_empty_frame(mixed):
    from egne_amd import loader
    rb, ab = mixed
    assert not ab.cond[:, 1].any()          # undecided on the host
    cond = loader.device_batch(ab, augment=False)[7].cpu().numpy()
    assert cond[:, 1].tolist() == [False, False, False, True, False] and rb.cond[:, 1].tolist() == cond[:, 1].tolist()
    assert not cond[:, [0, 2, 3]].any()


def test_augmented_batches_are_bit_equal(mixed):
    from egne_amd import loader
    rb, ab = mixed
    choices = [0, 6, 7, 0, 6]          # flip, rotation, none, flip, rotation
    outs = []
    for batch in (rb, ab):
        np.random.seed(5)
        outs.append(loader.device_batch(batch, augment=True, choices=choices, on_cv2="device"))
    _same(*outs)
    plain = loader.device_batch(ab, augment=False)
    assert not torch.equal(outs[1][1], plain[1])


def test_scaled_480x640_batches_are_bit_equal(tmp_path):
    from egne_amd import loader
    raw, ann = _archives(tmp_path, "c", 2, 480, 640, 60)
    rb, ab = loader.collate_raw([raw[0], raw[1]]), loader.collate_annotated([ann[0], ann[1]])
    out_r = loader.device_batch(rb, size=(480, 640), scale=0.5, augment=False)
    out_a = loader.device_batch(ab, size=(480, 640), scale=0.5, augment=False)
    _same(out_r, out_a)
    assert tuple(out_a[0].shape) == (2, 1, 240, 320)
