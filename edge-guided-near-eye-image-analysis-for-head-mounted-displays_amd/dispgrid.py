"""Prediction overlay grids on the device (csrc/dispgrid.hip): the reference's generateImageGrid (utils.py:206-399)
for train.py / test.py --disp 1 -- the first frames of a batch, histogram-equalised, the predicted classes painted in, the predicted
ellipses outlined, tiled side by side.

    grid = image_grid(img, mask, el, None, cond, el_gt, override=True)             # float32 [3,Hg,Wg] on the device
    grid, u8 = image_grid(..., return_u8=True); save_grid("grid.jpg", u8)          # uint8 [Hg,Wg,3] BGR -> a JPEG file

Which pixels are the reference's: the uint8 image handed to equalizeHist, both normalisations around it, the colours, the order of
the paints, the clip of the outlines to [6, size - 6], min(count, B), the cond / override rule and the integers handed to
ellipse_perimeter (tests/golden/dispgrid.npz records them from the reference's own function).  Which are this project's rules, because
OpenCV, scikit-image and torchvision do the rest there: the equalisation (OpenCV's published rule), the outline pixels
(frame_io._draw_ellipse's 720 samples, not scikit-image's perimeter), the grid layout (make_grid's documented one) and the uint8 form.
include/egne_hip.h states all of them.
"""
import torch

STATUS_CONSTANT, STATUS_NONFINITE = 1, 2
STATUS_SKIP_IRIS, STATUS_SKIP_PUPIL, STATUS_SKIP_GT_IRIS, STATUS_SKIP_GT_PUPIL = 4, 8, 16, 32


def grid_shape(n, nrow, H, W):
    """(Hg, Wg) of a grid of n frames of H x W: make_grid(nrow=nrow, padding=2); one frame is not padded."""
    if n == 1:
        return H, W
    xm = min(nrow, n)
    ym = -(-n // xm)
    return ym * (H + 2) + 2, xm * (W + 2) + 2


def _check(t, what, dtype, shape):
    if not torch.is_tensor(t) or not t.is_cuda:
        raise ValueError("%s must be a tensor on the GPU: this package has no CPU path" % what)
    if t.dtype != dtype or t.dim() != len(shape) or any(s is not None and int(t.shape[k]) != s for k, s in enumerate(shape)):
        raise ValueError("%s must be a %s tensor of shape [%s], got %s %s" % (
            what, str(dtype).replace("torch.", ""), ",".join("*" if s is None else str(s) for s in shape), t.dtype, tuple(t.shape)))


def image_grid(img, mask, el, pupil_center=None, cond=None, el_gt=None, heatmaps=False, override=False, count=4, nrow=4, draw_gt=False,
               return_u8=False, return_status=False):
    """generateImageGrid(I, mask, elNorm, pupil_center, cond, elNorm_gt, heatmaps, override) on the device (egne_disp_grid), in the
    reference's argument order: ``img`` float32 [B,H,W] (or [B,1,H,W]), ``mask`` int64 [B,H,W] (model.predictions()), ``el`` / ``el_gt``
    float32 [B,2,5] normalised (iris, pupil) ellipses, ``cond`` float32 [B,>=2] or None.  ``pupil_center`` and ``heatmaps`` are accepted
    and unused, as in the reference.  A frame is painted if ``override`` is set or ``cond[i,1] == 0``; with ``cond=None`` and
    ``override=False`` none is.  ``count`` frames at most (the reference: 4), ``nrow`` per grid row; ``draw_gt``: also the ground-truth
    outlines, in the colour of the reference's commented-out lines.  Returns the float32 grid [3,Hg,Wg]; with ``return_u8`` also the
    uint8 BGR image [Hg,Wg,3] (rint(255 * clip(grid, 0, 1)): how imshow shows the grid), with ``return_status`` also the int32 status
    word of every drawn frame (STATUS_* bits).  Queues on the current stream, synchronises nothing, can be captured in a graph."""
    from egne_amd import _lib, frame_io
    if torch.is_tensor(img) and img.dim() == 4 and img.shape[1] == 1:
        img = img[:, 0]
    _check(img, "img", torch.float32, (None, None, None))
    B, H, W = (int(v) for v in img.shape)
    _check(mask, "mask", torch.int64, (B, H, W))
    _check(el, "el", torch.float32, (B, 2, 5))
    if el_gt is not None:
        _check(el_gt, "el_gt", torch.float32, (B, 2, 5))
    elif draw_gt:
        raise ValueError("draw_gt needs el_gt")
    if cond is not None:
        _check(cond, "cond", torch.float32, (B, None))
        if cond.shape[1] < 2:
            raise ValueError("cond needs at least two columns, got %s" % (tuple(cond.shape),))
    count, nrow = int(count), int(nrow)
    if B < 1 or count < 1 or nrow < 1:
        raise ValueError("B, count and nrow must be positive (got %d, %d, %d)" % (B, count, nrow))
    if H < 6 or W < 6:
        raise ValueError("frames of at least 6 x 6 (the outline's clip to [6, size - 6]), got %d x %d" % (H, W))
    n = min(count, B)
    # only the drawn frames are made contiguous (a strided batch is copied, a contiguous one is not)
    img, mask, el = img[:n].contiguous(), mask[:n].contiguous(), el[:n].contiguous()
    el_gt = None if el_gt is None else el_gt[:n].contiguous()
    cond = None if cond is None else cond[:n].contiguous()
    dev = img.device
    cs, = frame_io.device_table("outline", dev, frame_io.outline_table)
    Hg, Wg = grid_shape(n, nrow, H, W)
    L = _lib.lib()
    grid = torch.empty((3, Hg, Wg), dtype=torch.float32, device=dev)
    u8 = torch.empty((Hg, Wg, 3), dtype=torch.uint8, device=dev) if return_u8 else None
    status = torch.empty(n, dtype=torch.int32, device=dev)
    ws = torch.empty(int(L.egne_disp_grid_workspace_bytes(n)), dtype=torch.uint8, device=dev)
    ptr = lambda t: None if t is None else t.data_ptr()       # noqa: E731
    with torch.cuda.device(dev):
        _lib.check(L.egne_disp_grid(img.data_ptr(), mask.data_ptr(), el.data_ptr(), ptr(el_gt), ptr(cond), 0 if cond is None else int(cond.shape[1]),
                                    n, H, W, int(bool(override)), int(bool(draw_gt)), n, nrow, cs.data_ptr(), grid.data_ptr(), ptr(u8),
                                    status.data_ptr(), ws.data_ptr(), _lib.stream_ptr()), "disp_grid")
    out = (grid,) + ((u8,) if return_u8 else ()) + ((status,) if return_status else ())
    return out[0] if len(out) == 1 else out


def script_grid(model_name, img, mask, el_flat, cond, el_gt, override):
    """The grid train.py / test.py --disp 1 draw: the uint8 image of the first four frames, with the ten regressed numbers ``el_flat``
    [B,10] reshaped to (iris, pupil) ellipses.  DeepVOG predicts pupil / not pupil -- only class 1 exists in its map --, so only the
    pupil ellipse is drawn: the iris rows are handed over as NaN, which image_grid skips (their status bits are set)."""
    B = el_flat.shape[0]
    if model_name == 'deepvog' and el_flat.numel() != B * 10:
        # (train.py hands over the regressed vector, which DeepVOG does not have: its fifth output is the embedding.  No ellipse then)
        el = torch.full((B, 2, 5), float('nan'), dtype=torch.float32, device=el_flat.device)
    else:
        el = el_flat.detach().float().reshape(B, 2, 5)
    el_gt = None if el_gt is None else el_gt.detach().float().reshape(B, 2, 5)
    if model_name == 'deepvog':
        el = el.clone()
        el[:, 0] = float('nan')
    cond = None if cond is None else cond.detach().float()
    return image_grid(img.detach().float(), mask, el, None, cond, el_gt, override=override, return_u8=True)[1]


def save_grid(path, grid_u8, quality=90):
    """Write the uint8 BGR image of image_grid(..., return_u8=True) as a baseline JPEG file, encoded on the device
    (mjpeg.encode_jpeg_device).  Synchronises: the file's bytes come down here."""
    from egne_amd import mjpeg
    _check(grid_u8, "grid_u8", torch.uint8, (None, None, 3))
    out, lengths, flags = mjpeg.encode_jpeg_device(grid_u8[None], quality=quality)
    length, flag = int(lengths[0].item()), int(flags[0].item())
    if flag or length <= 0:
        raise RuntimeError("save_grid: the JPEG file of a %dx%d grid did not fit its slot" % (grid_u8.shape[0], grid_u8.shape[1]))
    with open(path, "wb") as f:
        f.write(out[0, :length].cpu().numpy().tobytes())
    return path
