"""Device-side training loader: raw (image, label, ellipse) samples in, the nine tensors of CurriculumLib.py:166 out.

The reference's Dataset builds every item on the host (CurriculumLib.py:94-166): pad2Size, the optional scaleFn, the augmentation,
the label remap, Canny / dilate weights, three distance transforms and the z-score, per frame.  Here the Dataset only READS a sample
(what readImage returns, :168-195); ``collate_raw`` stacks a batch, and ``device_batch`` runs the item path for the whole batch on
the GPU, in the reference's order of operations:

    1. stage     egne_loader_stage (csrc/loader.hip)   pad2Size, then scaleFn's two cv2.resize calls
    2. augment   data_augment.augment_batch            on the STORED labels 0..3 (the flip / rotation see the sclera class)
    3. finish    egne_loader_finish                    label remap 1 -> 0, 2 -> 1, 3 -> 2 and the z-score, one launch
    4. weights   dataprep.spatial_weights / dist_maps  on the remapped label
    5. geometry  centres and ellipses: pad2Size's shift, scaleFn's transform, the augmentation's flip and rotation, then
                 get_ellipse_info's normalisation (dataprep._ellipse_info) -- or, with ellipse="ransac", dataprep.ellipse_targets

Raw sample (tuple, what readImage returns): image uint8 [r,c]; label int8 [r,c] (stored classes 0..3, -1 everywhere when absent);
elParam float64 [2,5] (iris first, -1 when absent); pupil_center float64 [2]; cond bool [4]; imInfo int64 [3].

An archive may hold the TEyeD ANNOTATIONS instead of label planes (AnnotationArchive; ``python -m egne_amd.make_archive`` writes
either kind): ``collate_annotated`` then stacks an AnnotBatch, whose ~0.6 KB record per frame is uploaded in place of the int8 plane,
and ``device_batch`` paints the labels on the device (dataprep.labels_from_annotations) in front of the same five stages.

PARITY: the Lanczos resize of ``scale`` is frame_io.resize_lanczos4 (same device code as the evaluate.py front end), whose parity
with cv2.resize is UNPINNED (OpenCV quantises the tap weights, this float64 restatement does not); the nearest-neighbour label resize
and everything else of the stage are exact.  spatial_weights and the cv2 branches of the augmentation carry their own notes.
"""
import collections

import numpy as np
import torch

from . import _lib, data_augment, dataprep
from .engine import require_cuda

RawBatch = collections.namedtuple("RawBatch", "images labels src_hw elParam pupil_center cond imInfo")
RawBatch.__doc__ = """A collated batch of raw samples (host NumPy arrays): images uint8 and labels int8 [B,Rmax,Cmax], every frame in
the top-left corner of its slot and zero-padded; src_hw int32 [B,2] its (rows, columns); elParam float64 [B,2,5]; pupil_center
float64 [B,2]; cond bool [B,4]; imInfo int64 [B,3]."""

AnnotBatch = collections.namedtuple("AnnotBatch", "images records src_hw elParam pupil_center cond imInfo")
AnnotBatch.__doc__ = """A collated batch of annotated samples (host NumPy arrays): a RawBatch whose label planes are replaced by
``records`` int32 [B,150] (dataprep.pack_annotations); cond[:,1] is False here and decided on the device from the painted labels."""


def read_cond(pupil_center, mask, pupil_param, iris_param):
    """The four flags of readImage (CurriculumLib.py:189-193): no pupil centre, no mask (all -1 or all 0), no pupil ellipse, no iris
    ellipse."""
    return np.array([np.all(pupil_center == -1), np.all(mask == -1) or np.all(mask == 0), np.all(pupil_param == -1),
                     np.all(iris_param == -1)])


class SyntheticRawEyes(torch.utils.data.Dataset):
    """Raw samples rendered by synth.augment_case (seed + index): the raw-sample stand-in for datasets that do not ship.  ``sizes``: a
    list of (rows, columns) source sizes, used in turn; each must fit ``target`` with even differences (pad2Size).  Every third seed
    has no pupil annotation (augment_case)."""

    def __init__(self, n, seed=1234, sizes=None, target=(240, 320)):
        from . import synth
        sizes = [tuple(target)] if sizes is None else [tuple(s) for s in sizes]
        self.samples = []
        for i in range(n):
            r, c = sizes[i % len(sizes)]
            if r > target[0] or c > target[1]:
                raise ValueError("SyntheticRawEyes: source size %dx%d exceeds the target %dx%d" % (r, c, target[0], target[1]))
            base, mask, pc, el = synth.augment_case(seed + i, H=r, W=c)          # el = (pupil, iris)
            el = np.stack([el[1], el[0]]).astype(np.float64)                    # iris first, as readImage
            mask = mask.astype(np.int8)
            self.samples.append((base, mask, el, pc.astype(np.float64), read_cond(pc, mask, el[1], el[0]),
                                 np.array([i, 0, i % 4], np.int64)))
        self.imList = torch.from_numpy(np.stack([s[5] for s in self.samples])) if n else torch.zeros(0, 3, dtype=torch.long)

    def __len__(self):
        return len(self.samples)

    def __getitem__(self, i):
        return self.samples[i]


class RawArchive(torch.utils.data.Dataset):
    """An ``.npz`` file whose arrays carry the names of the reference's H5 archives (readImage, CurriculumLib.py:181-185): Images
    uint8 [N,r,c], Masks_noSkin [N,r,c], pupil_loc [N,2], Fits_pupil [N,5], Fits_iris [N,5] ('Fits/pupil' and 'Fits/iris' there).
    An EMPTY array means "absent for all frames", as in the reference: the sample then holds -1.  ``index``: the frame numbers to
    serve (default: all)."""

    NAMES = ("Images", "Masks_noSkin", "pupil_loc", "Fits_pupil", "Fits_iris")

    def __init__(self, path, index=None, dataset_id=0):
        with np.load(path) as z:
            missing = [k for k in self.NAMES if k not in z.files]
            if missing:
                raise ValueError("RawArchive %s: arrays %s are missing" % (path, ", ".join(missing)))
            self.a = {k: z[k] for k in self.NAMES}
        n = len(self.a["Images"])
        self.index = np.arange(n) if index is None else np.asarray(index, np.int64)
        if len(self.index) and (self.index.min() < 0 or self.index.max() >= n):
            raise ValueError("RawArchive %s: index outside its %d frames" % (path, n))
        self.imList = torch.zeros(len(self.index), 3, dtype=torch.long)
        self.imList[:, 0] = torch.from_numpy(self.index)
        self.imList[:, 2] = dataset_id

    def __len__(self):
        return len(self.index)

    def __getitem__(self, i):
        a, k = self.a, int(self.index[i])
        img = np.ascontiguousarray(a["Images"][k], dtype=np.uint8)
        pc = np.asarray(a["pupil_loc"][k], np.float64) if len(a["pupil_loc"]) else -np.ones(2)
        mask = np.asarray(a["Masks_noSkin"][k]) if len(a["Masks_noSkin"]) else -np.ones(img.shape[:2])
        pupil = np.asarray(a["Fits_pupil"][k], np.float64) if len(a["Fits_pupil"]) else -np.ones(5)
        iris = np.asarray(a["Fits_iris"][k], np.float64) if len(a["Fits_iris"]) else -np.ones(5)
        return (img, mask.astype(np.int8), np.stack([iris, pupil]), pc, read_cond(pc, mask, pupil, iris), self.imList[i].numpy().copy())


class AnnotationArchive(torch.utils.data.Dataset):
    """An ``.npz`` file that holds TEyeD annotations instead of label planes: Images uint8 [N,r,c], ann_ball [N,3] = (r, cx, cy),
    ann_iris and ann_pupil [N,5] = (angle in degrees, cx, cy, full width, full height), ann_lid [N,n,2], float64 as the annotation
    files hold them (``make_archive --store annotations``).  A sample is (image, record int32 [150], elParam [2,5] iris first,
    pupil_center [2], cond [4], imInfo [3]); the ellipses and the centre are dataprep.annotation_fits of the rows, the record is
    dataprep.pack_annotations of them.  ``index``: the frame numbers to serve (default: all)."""

    NAMES = ("Images", "ann_ball", "ann_iris", "ann_pupil", "ann_lid")

    def __init__(self, path, index=None, dataset_id=0):
        with np.load(path) as z:
            missing = [k for k in self.NAMES if k not in z.files]
            if missing:
                raise ValueError("AnnotationArchive %s: arrays %s are missing" % (path, ", ".join(missing)))
            self.a = {k: z[k] for k in self.NAMES}
        a, n = self.a, len(self.a["Images"])
        self.records = dataprep.pack_annotations(a["ann_ball"], a["ann_iris"], a["ann_pupil"], a["ann_lid"]) if n else np.zeros((0, 150), np.int32)
        self.pupil_loc, self.fits_pupil, self.fits_iris = dataprep.annotation_fits(a["ann_iris"], a["ann_pupil"])
        self.index = np.arange(n) if index is None else np.asarray(index, np.int64)
        if len(self.index) and (self.index.min() < 0 or self.index.max() >= n):
            raise ValueError("AnnotationArchive %s: index outside its %d frames" % (path, n))
        self.imList = torch.zeros(len(self.index), 3, dtype=torch.long)
        self.imList[:, 0] = torch.from_numpy(self.index)
        self.imList[:, 2] = dataset_id

    def __len__(self):
        return len(self.index)

    def __getitem__(self, i):
        k = int(self.index[i])
        img = np.ascontiguousarray(self.a["Images"][k], dtype=np.uint8)
        pc, pupil, iris = self.pupil_loc[k], self.fits_pupil[k], self.fits_iris[k]
        # (the label is painted on the device: "mask all 0" is decided there, device_batch)
        return (img, self.records[k], np.stack([iris, pupil]), pc, read_cond(pc, np.ones(1), pupil, iris), self.imList[i].numpy().copy())


def open_archive(path, index=None, dataset_id=0):
    """RawArchive or AnnotationArchive, by the array names of the file."""
    with np.load(path) as z:
        annotated = "ann_ball" in z.files
    return (AnnotationArchive if annotated else RawArchive)(path, index, dataset_id)


def collate_for(dataset):
    """The ``collate_fn`` that fits a raw Dataset: collate_annotated for an AnnotationArchive, collate_raw otherwise."""
    return collate_annotated if isinstance(dataset, AnnotationArchive) else collate_raw


def split_archive(path, every=10):
    """(training set, validation set) of one archive (of either kind, open_archive) for train.py: every ``every``-th frame validates,
    the rest train; an archive of fewer frames than that serves both."""
    n = len(open_archive(path))
    idx = np.arange(n)
    if n < every:
        return open_archive(path), open_archive(path)
    return open_archive(path, idx[idx % every != every - 1]), open_archive(path, idx[idx % every == every - 1])


def collate_raw(samples):
    """A list of raw samples -> RawBatch (the ``collate_fn`` of a DataLoader over a raw Dataset)."""
    B = len(samples)
    hw = np.array([s[0].shape for s in samples], np.int32).reshape(B, 2)
    R, C = int(hw[:, 0].max()), int(hw[:, 1].max())
    images, labels = np.zeros((B, R, C), np.uint8), np.zeros((B, R, C), np.int8)
    for b, s in enumerate(samples):
        if s[1].shape != s[0].shape:
            raise ValueError("collate_raw: sample %d has a %s label for a %s image" % (b, s[1].shape, s[0].shape))
        images[b, :hw[b, 0], :hw[b, 1]] = s[0]
        labels[b, :hw[b, 0], :hw[b, 1]] = s[1]
    return RawBatch(images, labels, hw, np.stack([np.asarray(s[2], np.float64) for s in samples]).reshape(B, 2, 5),
                    np.stack([np.asarray(s[3], np.float64) for s in samples]).reshape(B, 2),
                    np.stack([np.asarray(s[4], bool) for s in samples]).reshape(B, 4),
                    np.stack([np.asarray(s[5], np.int64) for s in samples]).reshape(B, 3))


def collate_annotated(samples):
    """A list of AnnotationArchive samples -> AnnotBatch."""
    B = len(samples)
    hw = np.array([s[0].shape for s in samples], np.int32).reshape(B, 2)
    R, C = int(hw[:, 0].max()), int(hw[:, 1].max())
    images = np.zeros((B, R, C), np.uint8)
    for b, s in enumerate(samples):
        images[b, :hw[b, 0], :hw[b, 1]] = s[0]
    return AnnotBatch(images, np.stack([np.asarray(s[1], np.int32) for s in samples]).reshape(B, -1), hw,
                      np.stack([np.asarray(s[2], np.float64) for s in samples]).reshape(B, 2, 5),
                      np.stack([np.asarray(s[3], np.float64) for s in samples]).reshape(B, 2),
                      np.stack([np.asarray(s[4], bool) for s in samples]).reshape(B, 4),
                      np.stack([np.asarray(s[5], np.int64) for s in samples]).reshape(B, 3))


def pad_offsets(src_hw, size):
    """pad2Size's (up_r, up_c) per frame, int64 [B,2]; odd or negative differences are refused as the reference asserts
    (helperfunctions.py:416-417)."""
    up = np.asarray(size, np.int64)[None, :] - np.asarray(src_hw, np.int64).reshape(-1, 2)
    bad = np.nonzero((up < 0).any(1) | (up % 2 != 0).any(1))[0]
    if len(bad):
        b = int(bad[0])
        raise ValueError("pad2Size: frame %d of %dx%d does not fit the %dx%d canvas with an even, non-negative difference"
                         % (b, src_hw[b][0], src_hw[b][1], size[0], size[1]))
    return up // 2


def scaled_size(size, scale):
    """scaleFn's dsize (CurriculumLib.py:79) as (rows, columns)."""
    return (int(scale * size[0]), int(scale * size[1])) if scale else (int(size[0]), int(size[1]))


def stage(images, labels, src_hw, size=(240, 320), scale=False):
    """pad2Size and the optional scaleFn for a batch, one launch (egne_loader_stage).  ``images`` uint8 and ``labels`` int8
    [B,Rmax,Cmax] on the device (RawBatch layout), ``src_hw`` [B,2] on the HOST (checked here, before the launch).  Returns the uint8
    image and the int64 label [B,Hs,Ws]: what data_augment.augment_batch takes.  With ``scale`` the image is
    frame_io.resize_lanczos4 of the padded canvas, byte for byte (PARITY WITH cv2.resize UNPINNED, as for resize_lanczos4 itself),
    the label frame_io.resize_nearest."""
    from . import frame_io
    require_cuda(images, "images")
    require_cuda(labels, "labels")
    if images.dtype != torch.uint8 or images.dim() != 3 or labels.dtype != torch.int8 or labels.shape != images.shape:
        raise ValueError("stage: images must be uint8 [B,R,C] and labels int8 of the same shape")
    images, labels = images.contiguous(), labels.contiguous()
    B, R, C = images.shape
    H, W = int(size[0]), int(size[1])
    hw = np.ascontiguousarray(np.asarray(src_hw, np.int32).reshape(B, 2))
    if (hw < 1).any() or (hw[:, 0] > R).any() or (hw[:, 1] > C).any():
        raise ValueError("stage: src_hw outside the %dx%d raw buffer" % (R, C))
    pad_offsets(hw, (H, W))
    Hs, Ws = scaled_size((H, W), scale)
    if Hs < 1 or Ws < 1:
        raise ValueError("stage: scale %r leaves no pixels of a %dx%d canvas" % (scale, H, W))
    dev = images.device
    none = (None, None)
    rows = cols = near = none
    if (Hs, Ws) != (H, W):
        table = frame_io.device_table
        rows = table(("lanczos", H, Hs), dev, lambda: frame_io.lanczos4_table(H, Hs)) if Hs != H else none
        cols = table(("lanczos", W, Ws), dev, lambda: frame_io.lanczos4_table(W, Ws)) if Ws != W else none
        near = table(("nearest", H, Hs, W, Ws), dev, lambda: (frame_io.nearest_table(H, Hs).astype(np.int32),
                                                              frame_io.nearest_table(W, Ws).astype(np.int32)))
    hw_d = torch.from_numpy(hw).to(dev)
    oimg = torch.empty((B, Hs, Ws), dtype=torch.uint8, device=dev)
    olab = torch.empty((B, Hs, Ws), dtype=torch.int64, device=dev)
    ptr = lambda t: None if t is None else t.data_ptr()       # noqa: E731
    _lib.check(_lib.lib().egne_loader_stage(images.data_ptr(), labels.data_ptr(), hw_d.data_ptr(), B, R, C, H, W, Hs, Ws, ptr(rows[0]),
                                            ptr(rows[1]), ptr(cols[0]), ptr(cols[1]), ptr(near[0]), ptr(near[1]), oimg.data_ptr(),
                                            olab.data_ptr(), _lib.stream_ptr()), "loader_stage")
    return oimg, olab


def finish(img, label):
    """After the augmentation, one launch (egne_loader_finish): ``img`` uint8 and ``label`` int64 [B,H,W] on the device -> (float32
    [B,1,H,W] z-score, bit-identical to dataprep.zscore(img.float()) with the same float64 statistics; int64 [B,H,W] label with
    1 -> 0, 2 -> 1, 3 -> 2 and every other value, -1 included, unchanged: CurriculumLib.py:123-125, :139).  No second launch is
    needed for the statistics: one workgroup per frame reduces and normalises, the remap runs in the launch's other workgroups."""
    require_cuda(img, "img")
    require_cuda(label, "label")
    if img.dtype != torch.uint8 or img.dim() != 3 or label.dtype != torch.int64 or label.shape != img.shape:
        raise ValueError("finish: img must be uint8 [B,H,W] and label int64 of the same shape")
    img, label = img.contiguous(), label.contiguous()
    B, H, W = img.shape
    x = torch.empty((B, 1, H, W), dtype=torch.float32, device=img.device)
    olab = torch.empty_like(label)
    _lib.check(_lib.lib().egne_loader_finish(img.data_ptr(), label.data_ptr(), x.data_ptr(), olab.data_ptr(), B, H * W, _lib.stream_ptr()),
               "loader_finish")
    return x, olab


def stage_geometry(elParam, pupil_center, src_hw, size, scale=False):
    """What pad2Size (helperfunctions.py:425-427) and scaleFn (CurriculumLib.py:80-88) do to the ellipses [B,2,5] and pupil centres
    [B,2] (float64, any of NumPy / torch; returns CPU float64 tensors): entries that are -1 throughout mark an absent annotation and
    stay."""
    el = torch.as_tensor(np.asarray(elParam, np.float64)).clone().reshape(-1, 2, 5)
    pc = torch.as_tensor(np.asarray(pupil_center, np.float64)).clone().reshape(-1, 2)
    up = pad_offsets(src_hw, size)
    shift = torch.from_numpy(np.stack([up[:, 1], up[:, 0]], axis=1).astype(np.float64))       # (up_c, up_r)
    has_el = ~(el == -1).all(dim=-1)
    has_pc = ~(pc == -1).all(dim=-1, keepdim=True)
    el[..., :2] = torch.where(has_el[..., None], el[..., :2] + shift[:, None, :], el[..., :2])
    pc = torch.where(has_pc, pc + shift, pc)
    if scale:
        s = float(scale)
        Hi = torch.tensor([[1.0 / s, 0, 0], [0, 1.0 / s, 0], [0, 0, 1]], dtype=torch.float64)       # inverse of scaleFn's H
        # scaleFn's quirk (CurriculumLib.py:85-86), kept: BOTH ellipses are tested with elParam[0], and when that first ellipse is
        # absent it REPLACES the second one as well.  (A second ellipse of -1 next to a present first one goes through the conic
        # like any other; cond masks what comes out of it.)
        has0 = has_el[:, 0:1]
        tr = dataprep._ellipse_transform(torch.where(has0[..., None], el, torch.ones_like(el)), Hi)
        el = torch.where(has0[..., None], tr, el[:, 0:1].expand(-1, 2, -1))
        pc = torch.where(has_pc, s * pc, pc)
    return el, pc


def device_batch(raw, size=(240, 320), scale=False, augment=False, choices=None, on_cv2="device", host_noise=False, ellipse="given",
                 device=None):
    """The reference's ``__getitem__`` (CurriculumLib.py:94-166) for a RawBatch or an AnnotBatch, on the device.  For an AnnotBatch
    the stored labels are painted on the device from the records (dataprep.labels_from_annotations, the Masks_noSkin map) in place of
    an uploaded plane, and cond[:,1] ("mask all 0") is its status bit, composed on the device; everything else is the same path.  Returns the nine tensors of :166
    with a leading batch axis, all on the GPU: img float32 [B,1,H,W], label int64 [B,H,W], spatialWeights float32 [B,H,W], distMap
    float32 [B,3,H,W], pupil_center and iris_center float32 [B,2], elNorm float32 [B,2,5], cond bool [B,4], imInfo int64 [B,3].

    ``size``: pad2Size's canvas.  ``scale``: scaleFn's factor (False: none).  ``augment``: data_augment.augment_batch between the
    stage and the label remap, with its ``choices`` / ``on_cv2`` / ``host_noise``.  ``ellipse``: "given" takes centres, elNorm and
    cond from the sample's annotation (pad shift, scale transform through the conic, flip / rotation, then get_ellipse_info's
    normalisation; iris_center = elParam[0][:2] if not cond[3] else pupil_center); "ransac" takes them from
    dataprep.ellipse_targets on the remapped label instead.

    Everything queues on the current stream.  Host work: the shape checks, the geometry of [B,2,5] numbers up to the augmentation
    (its rotation is host code already), and augment_batch's random draws.  No synchronisation is added to what the host-to-device
    copies of the batch and of the draws imply."""
    if ellipse not in ("given", "ransac"):
        raise ValueError("device_batch: ellipse must be \"given\" or \"ransac\", not %r" % (ellipse,))
    size = (int(size[0]), int(size[1]))
    el, pc = stage_geometry(raw.elParam, raw.pupil_center, raw.src_hw, size, scale)       # refuses frames that do not fit, first
    dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    annotated = isinstance(raw, AnnotBatch)
    images = torch.from_numpy(raw.images).to(dev)
    if annotated:
        labels, status = dataprep.labels_from_annotations(raw.records, raw.images.shape[1:], raw.src_hw, with_skin=False, return_status=True,
                                                          device=dev)
    else:
        labels = torch.from_numpy(raw.labels).to(dev)
    img, lab = stage(images, labels, raw.src_hw, size, scale)
    if augment:
        img, lab, pc, el, _ = data_augment.augment_batch(img, lab, pc, el, choices, host_noise=host_noise, on_cv2=on_cv2)
    x, lab = finish(img, lab)
    sw = dataprep.spatial_weights(lab)
    dm = dataprep.dist_maps(lab)
    info = torch.from_numpy(np.ascontiguousarray(raw.imInfo, dtype=np.int64)).to(dev)
    if ellipse == "ransac":
        pc_d, ic_d, eln, cond = dataprep.ellipse_targets(lab)
        return x, lab, sw, dm, pc_d, ic_d, eln, cond.bool(), info
    H, W = lab.shape[1:]
    cond = torch.from_numpy(np.ascontiguousarray(raw.cond, dtype=bool)).to(dev)
    if annotated:
        cond[:, 1] = (status & dataprep.ANNOT_EMPTY) != 0
    el, pc = el.to(dev), pc.to(dev)
    gone = cond[:, [3, 2]][..., None]                         # iris first: cond[3] is the iris ellipse, cond[2] the pupil's
    eln = torch.where(gone, -torch.ones_like(el), dataprep._ellipse_info(torch.where(gone, torch.ones_like(el), el), H, W))
    ic = torch.where(cond[:, 3:4], pc, el[:, 0, :2])
    return x, lab, sw, dm, pc.float(), ic.float(), eln.float(), cond, info
