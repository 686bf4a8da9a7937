"""Host-side mirror of the reference's ``utils.py`` for the hot path.

Same names, argument meaning and error behaviour as the reference functions the entry scripts
call (file:line cited per function).  Compute runs on the HIP path; the metric helpers stay on
the host with numpy exactly as in the reference (they define "mIoU").
"""
import copy
import ctypes as C

import numpy as np
import torch
import torch.nn as nn

from . import _lib
from .engine import require_cuda


# ---------------------------------------------------------------------------------------------
# parameter containers (same state_dict keys as the reference modules)
# ---------------------------------------------------------------------------------------------
class convBlock(nn.Module):
    """utils.py:1039-1050: conv3x3 -> leaky -> conv3x3 -> leaky -> BatchNorm2d (parameters only;
    executed by esf_engine)."""

    def __init__(self, in_c, inter_c, out_c, actfunc=None):
        super().__init__()
        self.conv1 = nn.Conv2d(in_c, inter_c, kernel_size=3, padding=1)
        self.conv2 = nn.Conv2d(inter_c, out_c, kernel_size=3, padding=1)
        self.bn = nn.BatchNorm2d(num_features=out_c)


class regressionModule(nn.Module):
    """utils.py:983-1011 (parameters only)."""

    def __init__(self, feature_channels):
        super().__init__()
        inC = feature_channels if isinstance(feature_channels, int) else int(feature_channels["enc"]["op"][-1])
        self.c1 = nn.Conv2d(inC, 128, kernel_size=(2, 3), bias=True)
        self.c2 = nn.Conv2d(128, 128, kernel_size=3, bias=True)
        self.c3 = nn.Conv2d(128, 32, kernel_size=3, bias=False)
        self.l1 = nn.Linear(32 * 3 * 5, 256, bias=True)
        self.l2 = nn.Linear(256, 10, bias=True)


class linStack(nn.Module):
    """utils.py:953-981 (parameters only; used for the dataset-identity head)."""

    def __init__(self, num_layers, in_dim, hidden_dim, out_dim, bias, actBool, dp):
        super().__init__()
        self.layersLin = nn.ModuleList([
            nn.Linear(hidden_dim if i > 0 else in_dim, hidden_dim if i < num_layers - 1 else out_dim, bias=bias)
            for i in range(num_layers)])
        self.actBool = actBool
        self.dp_p = dp


class LinearBlock(nn.Module):
    """utils.py:1051-1090 with norm='none' (the only form the path uses)."""

    def __init__(self, input_dim, output_dim, norm="none", activation="relu"):
        super().__init__()
        if norm not in ("none", "sn"):
            raise AssertionError("Unsupported normalization: {}".format(norm))
        self.fc = nn.Linear(input_dim, output_dim, bias=True)
        self.activation_name = activation


class Conv2dBlock(nn.Module):
    """utils.py:1092-1149 with norm='none' (StyleEncoder's form)."""

    def __init__(self, input_dim, output_dim, kernel_size, stride, padding=0, norm="none", activation="relu",
                 pad_type="zero"):
        super().__init__()
        if norm not in ("none", "sn"):
            raise AssertionError("Unsupported normalization: {}".format(norm))
        if pad_type not in ("reflect", "zero"):
            raise AssertionError("Unsupported padding type: {}".format(pad_type))
        self.conv = nn.Conv2d(input_dim, output_dim, kernel_size, stride, bias=True)
        self.padding, self.pad_type, self.activation_name = padding, pad_type, activation


# ---------------------------------------------------------------------------------------------
# small host helpers
# ---------------------------------------------------------------------------------------------
def create_meshgrid(height, width, normalized_coordinates=True):
    """utils.py:27-60: [1,H,W,2] grid, x = linspace(-1,1,W), y = linspace(-1,1,H)."""
    if normalized_coordinates:
        xs, ys = torch.linspace(-1, 1, width), torch.linspace(-1, 1, height)
    else:
        xs, ys = torch.linspace(0, width - 1, width), torch.linspace(0, height - 1, height)
    return torch.stack([xs[None, :].expand(height, width), ys[:, None].expand(height, width)], dim=-1)[None]


def get_nparams(model):
    return sum(p.numel() for p in model.parameters() if p.requires_grad)


def normPts(pts, sz):
    """utils.py:627-634."""
    o = copy.deepcopy(pts)
    shp = o.shape
    o = o.reshape(-1, 2)
    o[:, 0] = 2 * (o[:, 0] / sz[1]) - 1
    o[:, 1] = 2 * (o[:, 1] / sz[0]) - 1
    return o.reshape(shp)


def unnormPts(pts, sz):
    """utils.py:636-643."""
    o = copy.deepcopy(pts)
    shp = o.shape
    o = o.reshape(-1, 2)
    o[:, 0] = 0.5 * sz[1] * (o[:, 0] + 1)
    o[:, 1] = 0.5 * sz[0] * (o[:, 1] + 1)
    return o.reshape(shp)


def calc_edge(args, img, edge_model, device):
    """utils.py:645-656: grey -> 3 channels -> frozen BDCN -> fused map; optional >=0.1 -> 1
    (``args.edge_thres``), fused into the tail kernel here."""
    with torch.no_grad():
        x = torch.cat((img, img, img), dim=1).to(device).to(torch.float32)
        e = edge_model.forward_fuse(x, edge_thres=1 if getattr(args, "edge_thres", 0) == 1 else 0)
    return e.to(getattr(args, "prec", torch.float32))


def get_predictions(output):
    """utils.py:65-81: argmax over channels -> [B,H,W] int64 on the host (first max wins ties)."""
    bs, c, h, w = output.size()
    _, idx = output.cpu().max(1)
    return idx.view(bs, h, w)


def _jaccard(y_true, y_pred, labels):
    out = []
    for l in labels:
        t, p = y_true == l, y_pred == l
        union = np.count_nonzero(t | p)
        out.append(np.count_nonzero(t & p) / union if union else 0.0)
    return np.array(out)


def getSeg_metrics(y_true, y_pred, cond):
    """utils.py:120-150: per-sample Jaccard over the classes present in the ground truth, nan-mean."""
    assert y_pred.ndim == 3, "Incorrect number of dimensions"
    assert y_true.ndim == 3, "Incorrect number of dimensions"
    cond = cond.astype(bool)
    rows = []
    for i in range(y_true.shape[0]):
        present = np.unique(y_true[i])
        vals = np.full((3,), np.nan)
        if not cond[i]:
            sc = _jaccard(y_true[i].reshape(-1), y_pred[i].reshape(-1), present)
            for j, v in enumerate(present):
                vals[v] = sc[j]
        rows.append(vals)
    return seg_metrics_of_rows(np.stack(rows, axis=0), cond)


def seg_metrics_of_rows(rows, cond):
    """The reduction that ends getSeg_metrics (utils.py:146-150) on a finished ``score_list`` [B,3] and a boolean ``cond``; shared
    with egne_amd.scores, whose rows come from the device."""
    clean = rows[~cond, :]
    if len(clean) == 0:
        return np.nan, np.nan * np.ones(3), rows
    with np.errstate(all="ignore"):
        import warnings
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", category=RuntimeWarning)
            per = np.nanmean(clean, axis=0)
            mean = np.nanmean(per)
    return mean, per, rows


def getPoint_metric(y_true, y_pred, cond, sz, do_unnorm):
    """utils.py:152-162: mean euclidean distance over valid samples."""
    if do_unnorm:
        y_pred = unnormPts(y_pred, sz)
    flag = (~cond.astype(bool)).astype(float)
    dist = flag * np.sqrt(((np.asarray(y_true) - np.asarray(y_pred)) ** 2).sum(axis=1))
    return (np.sum(dist) / np.sum(flag) if np.any(flag) else np.nan, dist)


def getAng_metric(y_true, y_pred, cond):
    """utils.py:164-170."""
    flag = (~cond.astype(bool)).astype(float)
    dist = np.rad2deg(flag * np.abs(y_true - y_pred))
    return (np.sum(dist) / np.sum(flag) if np.any(flag) else np.nan, dist)


# ---------------------------------------------------------------------------------------------
# ellipse fit (evaluate.py's "fit" stage) on the device
# ---------------------------------------------------------------------------------------------
_mesh_cache = {}


def _mesh_axes(H, W, dev):
    key = (H, W, str(dev))
    if key not in _mesh_cache:
        _mesh_cache[key] = (torch.linspace(-1, 1, W).to(dev), torch.linspace(-1, 1, H).to(dev))
    return _mesh_cache[key]


def fit_ellipses(mask, frame_of, cls, init, return_evals=False):
    """Batched device form of search_proper_parameter_iou_for_our_data (utils.py:450-486).

    mask [F,H,W] int64 class maps on the GPU; frame_of / cls [n] which frame / class each fit
    uses; init [n,5] (cx,cy,a,b,theta) pixels.  Returns [n,5] float64 (cx,cy,a,b,theta)."""
    require_cuda(mask, "mask")
    L = _lib.lib()
    dev = mask.device
    F, H, W = mask.shape
    n = len(frame_of)
    fo_h = np.asarray(frame_of, dtype=np.int32)
    if n and (fo_h.min() < 0 or fo_h.max() >= F):
        raise ValueError("fit_ellipses: frame index %d outside the %d class maps given" % (int(fo_h.max()), F))
    fo = torch.as_tensor(fo_h).to(dev)
    cl = torch.as_tensor(np.asarray(cls, dtype=np.int32)).to(dev)
    ini = torch.as_tensor(np.asarray(init, dtype=np.float64).reshape(n, 5)).to(dev)
    out = torch.empty((n, 5), dtype=torch.float64, device=dev)
    ev = torch.zeros((n,), dtype=torch.int32, device=dev)
    xs, ys = _mesh_axes(H, W, dev)
    m = mask.contiguous()
    _lib.check(L.egne_ellipse_fit(m.data_ptr(), F, fo.data_ptr(), cl.data_ptr(), n, H, W, xs.data_ptr(), ys.data_ptr(),
                                  ini.data_ptr(), out.data_ptr(), ev.data_ptr(), _lib.stream_ptr()), "ellipse_fit")
    return (out.cpu().numpy(), ev.cpu().numpy()) if return_evals else out.cpu().numpy()


def ellipse_iou_counts(mask, frame_of, cls, ell, roww=1):
    """One evaluation of the search per ellipse, through the device functions the search kernel calls (csrc/fit.hip): the three
    counts of calc_ell_iou (utils.py:176-204) before the division.

    mask [F,H,W] int64 class maps on the GPU; frame_of / cls [n]; ell [n,5] (cx, cy, a, b) pixels and the angle in DEGREES (what one
    evaluation of the search is handed); roww 1 or 4 = waves that share the rows.  Returns uint32 [n,3] (nseg, nell, inter); a
    frame_of outside [0, F) gives 0xffffffff three times."""
    require_cuda(mask, "mask")
    L = _lib.lib()
    dev = mask.device
    F, H, W = mask.shape
    n = len(frame_of)
    fo = torch.as_tensor(np.asarray(frame_of, dtype=np.int32)).to(dev)
    cl = torch.as_tensor(np.asarray(cls, dtype=np.int32)).to(dev)
    el = torch.as_tensor(np.asarray(ell, dtype=np.float64).reshape(n, 5)).to(dev)
    out = torch.empty((n, 3), dtype=torch.int32, device=dev)
    xs, ys = _mesh_axes(H, W, dev)
    m = mask.contiguous()
    _lib.check(L.egne_ellipse_iou_counts(m.data_ptr(), F, fo.data_ptr(), cl.data_ptr(), n, H, W, xs.data_ptr(), ys.data_ptr(),
                                         el.data_ptr(), out.data_ptr(), int(roww), _lib.stream_ptr()), "ellipse_iou_counts")
    return out.cpu().numpy().view(np.uint32)


def ellipse_seeds_from_pred(elPred, H, W):
    """evaluate.py:135-151 on the device: elPred [F,10] float32 (normalised ellipses of the regression head)
    -> (init [2F,5] float64 pixel ellipses, frame_of [2F] int32, cls [2F] int32), all on the GPU.
    Fit 2f is the iris (class 1) of frame f, fit 2f+1 its pupil (class 2)."""
    require_cuda(elPred, "elPred")
    L = _lib.lib()
    F = elPred.shape[0]
    ep = elPred.detach().to(torch.float32).contiguous()
    init = torch.empty((2 * F, 5), dtype=torch.float64, device=ep.device)
    fo = torch.empty((2 * F,), dtype=torch.int32, device=ep.device)
    cl = torch.empty((2 * F,), dtype=torch.int32, device=ep.device)
    _lib.check(L.egne_ellipse_init_from_pred(ep.data_ptr(), F, H, W, init.data_ptr(), fo.data_ptr(), cl.data_ptr(),
                                             _lib.stream_ptr()), "ellipse_init_from_pred")
    return init, fo, cl


def fit_ellipses_from_pred(mask, elPred, out=None, classes=None):
    """The fit stage of evaluate.py:135-166 with no host hop: seeds from ``elPred`` on the device, both searches of
    every frame in one launch.  Returns a DEVICE tensor [F,2,5] float64 (iris, pupil) x (cx,cy,a,b,theta); nothing
    here synchronises -- the caller decides when to read it.  ``classes``: the class of the map the iris and the pupil are
    searched against (default (1, 2)); a negative one leaves that search out, its row is NaN."""
    require_cuda(mask, "mask")
    L = _lib.lib()
    F, H, W = mask.shape
    if elPred.shape[0] != F:
        raise ValueError("fit_ellipses_from_pred: %d ellipse rows for %d class maps" % (elPred.shape[0], F))
    init, fo, cl = ellipse_seeds_from_pred(elPred, H, W)
    if classes is not None and tuple(classes) != (1, 2):
        cl = torch.tensor([int(classes[0]), int(classes[1])], dtype=torch.int32, device=mask.device).repeat(F)
        fo = torch.where(cl < 0, torch.full_like(fo, -1), fo)
    if out is None:
        out = torch.empty((F, 2, 5), dtype=torch.float64, device=mask.device)
    xs, ys = _mesh_axes(H, W, mask.device)
    m = mask.contiguous()
    _lib.check(L.egne_ellipse_fit(m.data_ptr(), F, fo.data_ptr(), cl.data_ptr(), 2 * F, H, W, xs.data_ptr(), ys.data_ptr(),
                                  init.data_ptr(), out.data_ptr(), None, _lib.stream_ptr()), "ellipse_fit")
    return out


DEFAULT_SEED_REGIONS = ((0b110, 1), (0b100, 2))     # iris = classes 1 and 2 together, searched against class 1 as today; pupil = class 2
_region_cache = {}


def _region_rows(regions, F, dev):
    """frame_of / class_bits / search_cls [R*F] int32 on the device for ``regions`` repeated over F frames (row R*f + r).  Cached:
    the upload happens on the first (eager) call, so a captured graph only reads the tables."""
    regions = tuple((int(b), int(c)) for b, c in regions)
    if not regions:
        raise ValueError("regions: at least one (class_bits, search_cls) pair")
    for b, c in regions:
        if not 0 <= b < 1 << 32:
            raise ValueError("regions: class_bits %r is not a bitmask over class ids 0..31" % (b,))
    key = (regions, int(F), str(dev))
    if key not in _region_cache:
        R = len(regions)
        fo = np.repeat(np.arange(F, dtype=np.int32), R)
        cb = np.tile(np.array([b for b, _ in regions], dtype=np.uint32).view(np.int32), F)
        sc = np.tile(np.array([c for _, c in regions], dtype=np.int32), F)
        _region_cache[key] = tuple(torch.from_numpy(a).to(dev) for a in (fo, cb, sc))
    return _region_cache[key]


def ellipse_seeds_from_mask(mask, regions=DEFAULT_SEED_REGIONS, min_area=7, return_stats=False):
    """Seeds of the search from the class map itself (csrc/mask_seed.hip; not in the reference): per (frame, region) the largest
    8-connected component of the region and the ellipse of its second moments.

    mask [F,H,W] int64 class maps on the GPU; ``regions`` lists (class_bits, search_cls) per frame in output order -- a pixel belongs
    to the region iff bit mask[p] of class_bits is set; search_cls is the class the search scores against (None: the default).  Returns (init [R*F,5]
    float64, frame_of [R*F] int32, cls [R*F] int32) on the device, like ellipse_seeds_from_pred; row R*f + r is region r of frame f.
    An absent region (no pixel, or fewer than ``min_area`` -- ElliFit's "more than 6 points") has init = -1 five times and frame_of =
    -1.  With ``return_stats`` also stats int64 [R*F,8] = (N, Sx, Sy, Sxx, Sxy, Syy, components, region pixels) and the int32 status
    word (0 = every loop ended inside its bound).  Nothing here synchronises."""
    require_cuda(mask, "mask")
    if mask.dtype != torch.int64 or mask.dim() != 3:
        raise ValueError("mask must be an int64 [F,H,W] tensor")
    L = _lib.lib()
    dev = mask.device
    F, H, W = (int(v) for v in mask.shape)
    fo_in, cb, sc = _region_rows(DEFAULT_SEED_REGIONS if regions is None else regions, F, dev)
    return _seeds_from_mask_rows(L, mask.contiguous(), fo_in, cb, sc, int(min_area), return_stats)


def _seeds_from_mask_rows(L, m, fo_in, cb, sc, min_area, return_stats):
    dev = m.device
    F, H, W = (int(v) for v in m.shape)
    n = int(fo_in.shape[0])
    nbytes = int(L.egne_mask_seed_workspace_bytes(n, H, W))
    if nbytes < 0:
        raise ValueError("ellipse_seeds_from_mask: %d rows of %dx%d class maps (2..1024 rows and columns, at most 2^20 pixels)" % (n, H, W))
    ws = torch.empty((nbytes + 7) // 8, dtype=torch.int64, device=dev)
    init = torch.empty((n, 5), dtype=torch.float64, device=dev)
    fo = torch.empty((n,), dtype=torch.int32, device=dev)
    cl = torch.empty((n,), dtype=torch.int32, device=dev)
    stats = torch.empty((n, 8), dtype=torch.int64, device=dev)
    status = torch.empty((1,), dtype=torch.int32, device=dev)
    _lib.check(L.egne_ellipse_init_from_mask(m.data_ptr(), F, fo_in.data_ptr(), cb.data_ptr(), sc.data_ptr(), n, H, W, min_area,
                                             init.data_ptr(), fo.data_ptr(), cl.data_ptr(), stats.data_ptr(), status.data_ptr(),
                                             ws.data_ptr(), _lib.stream_ptr()), "ellipse_init_from_mask")
    return (init, fo, cl, stats, status) if return_stats else (init, fo, cl)


DEFAULT_CLEAN_LAYERS = ((0b110, 1, 3), (0b100, 2, 3))     # the iris blob of classes 1 | 2 (largest, holes filled), then the pupil blob over it
_layer_cache = {}


def _layer_rows(layers, F, dev):
    """frame_of / class_bits / paint_cls / flags [L*F] int32 on the device for ``layers`` repeated over F frames (row L*f + j), cached
    like the seeds' tables: the upload happens on the first (eager) call, so a captured graph only reads them."""
    try:
        layers = tuple(tuple(int(v) for v in r) for r in layers)
    except (TypeError, ValueError):
        raise ValueError("layers: (class_bits, paint_cls, flags) triples, got %r" % (layers,))
    if not layers:
        raise ValueError("layers: at least one (class_bits, paint_cls, flags) triple")
    for r in layers:
        if len(r) != 3:
            raise ValueError("layers: (class_bits, paint_cls, flags) triples, got %r" % (r,))
        if not 0 <= r[0] < 1 << 32:
            raise ValueError("layers: class_bits %r is not a bitmask over class ids 0..31" % (r[0],))
        if not -(1 << 31) <= r[1] < 1 << 31:
            raise ValueError("layers: paint_cls %r does not fit 32 bits" % (r[1],))
        if not 0 <= r[2] <= 3:
            raise ValueError("layers: flags %r (bit 0: largest component, bit 1: fill its holes)" % (r[2],))
    key = (layers, int(F), str(dev))
    if key not in _layer_cache:
        fo = np.repeat(np.arange(F, dtype=np.int32), len(layers))
        cb = np.tile(np.array([r[0] for r in layers], dtype=np.uint32).view(np.int32), F)
        pc = np.tile(np.array([r[1] for r in layers], dtype=np.int32), F)
        fl = np.tile(np.array([r[2] for r in layers], dtype=np.int32), F)
        _layer_cache[key] = tuple(torch.from_numpy(a).to(dev) for a in (fo, cb, pc, fl))
    return _layer_cache[key]


def clean_class_maps(mask, layers=DEFAULT_CLEAN_LAYERS, open3=True, min_area=1, fill_cls=0, out=None, return_stats=False):
    """Cleaned class maps (csrc/cleanup.hip; the contract is in include/egne_hip.h): per-class 3x3 opening (the
    reference's helperfunctions.clean_mask), then per layer the largest 8-connected blob with its holes filled, painted in layer order
    over ``fill_cls``.

    mask [F,H,W] int64 class maps on the GPU; ``layers`` lists (class_bits, paint_cls, flags) applied to every frame: a pixel belongs
    to the layer iff it survives the opening of its own class (``open3``; every id 0..31 survives without it) and bit mask[p] of
    class_bits is set; flags bit 0 keeps the largest component only, bit 1 fills the holes of what is kept; a layer with fewer than
    ``min_area`` pixels left paints nothing.  Returns the cleaned maps, int64 [F,H,W] on the device (``out`` if given: contiguous,
    same shape, not overlapping ``mask``).  With ``return_stats`` also stats int64 [L*F,4] = (pixels of the layer, its components,
    pixels kept, pixels added by filling; row L*f + j is layer j of frame f) and the int32 status word (0 = every loop ended inside
    its bound).  Nothing here synchronises."""
    require_cuda(mask, "mask")
    if mask.dtype != torch.int64 or mask.dim() != 3:
        raise ValueError("mask must be an int64 [F,H,W] tensor")
    L = _lib.lib()
    dev = mask.device
    F, H, W = (int(v) for v in mask.shape)
    min_area = int(min_area)
    if min_area < 1:
        raise ValueError("clean_class_maps: min_area %d (at least 1)" % min_area)
    fo, cb, pc, fl = _layer_rows(DEFAULT_CLEAN_LAYERS if layers is None else layers, F, dev)
    n = int(fo.shape[0])
    nbytes = int(L.egne_class_map_cleanup_workspace_bytes(n, H, W))
    if nbytes < 0:
        raise ValueError("clean_class_maps: %d rows of %dx%d class maps (2..1024 rows and columns, at most 2^20 pixels)" % (n, H, W))
    m = mask.contiguous()
    if out is None:
        out = torch.empty((F, H, W), dtype=torch.int64, device=dev)
    elif out.dtype != torch.int64 or tuple(out.shape) != (F, H, W) or not out.is_contiguous() or out.device != dev:
        raise ValueError("out must be a contiguous int64 [%d,%d,%d] tensor on the device of mask" % (F, H, W))
    span = F * H * W * 8
    if F and m.data_ptr() < out.data_ptr() + span and out.data_ptr() < m.data_ptr() + span:
        raise ValueError("clean_class_maps: out overlaps mask")
    ws = torch.empty((nbytes + 7) // 8, dtype=torch.int64, device=dev)
    stats = torch.empty((n, 4), dtype=torch.int64, device=dev)
    status = torch.empty((1,), dtype=torch.int32, device=dev)
    _lib.check(L.egne_class_map_cleanup(m.data_ptr(), F, fo.data_ptr(), cb.data_ptr(), pc.data_ptr(), fl.data_ptr(), n, H, W,
                                        1 if open3 else 0, min_area, int(fill_cls), out.data_ptr(), stats.data_ptr(), status.data_ptr(),
                                        ws.data_ptr(), _lib.stream_ptr()), "class_map_cleanup")
    return (out, stats, status) if return_stats else out


DEFAULT_RANSAC_REGIONS = ((0b110, 1, 0), (0b100, 2, 0b001))     # iris: boundary of classes 1 and 2 together; pupil: class 2 without
                                                                # background-adjacent points (getValidPoints' condPupil)
DEEPVOG_RANSAC_REGIONS = ((0, 1), (0b010, 1, 0))
_ransac_cache = {}


def _ransac_rows(regions, F, dev):
    """_region_rows for region tuples that may carry a third element exclude_bits (default 0): (frame_of, class_bits, search_cls,
    exclude_bits) [R*F] int32 on the device, cached like the seeds' tables."""
    regions = tuple(tuple(int(v) for v in r) + (0,) * (3 - len(r)) for r in regions)
    for r in regions:
        if len(r) != 3 or not 0 <= r[2] < 1 << 32:
            raise ValueError("regions: (class_bits, search_cls[, exclude_bits]) with bitmasks over class ids 0..31, got %r" % (r,))
    fo, cb, sc = _region_rows(tuple(r[:2] for r in regions), F, dev)
    key = (regions, int(F), str(dev))
    if key not in _ransac_cache:
        _ransac_cache[key] = torch.from_numpy(np.tile(np.array([r[2] for r in regions], dtype=np.uint32).view(np.int32), F)).to(dev)
    return fo, cb, sc, _ransac_cache[key]


def _draw_table(draws, n, K1, n_min, dev):
    """An explicit draw table as an int32 device tensor.  A device tensor is used as it is (the form for a captured graph: nothing
    is uploaded); anything else is uploaded by this call."""
    d = draws if torch.is_tensor(draws) else torch.from_numpy(np.ascontiguousarray(np.asarray(draws, dtype=np.int32)))
    d = d.to(device=dev, dtype=torch.int32).contiguous()
    if tuple(d.shape) != (n, K1, n_min):
        raise ValueError("draws: shape %r, expected [%d, %d, %d] (rows, iters + 1, n_min)" % (tuple(d.shape), n, K1, n_min))
    return d


def ellipse_ransac_from_mask(mask, regions=DEFAULT_RANSAC_REGIONS, n_min=15, iters=40, thres=5e-3, n_good=15, draws=None, seed=0,
                             max_pts=4096, return_stats=False):
    """The reference's ellipse estimator for masks on the device (csrc/ellifit.hip): per (frame, region) the boundary
    points of the region, helperfunctions.ElliFit under helperfunctions.ransac(pts, ElliFit, n_min, iters, thres, n_good).loop().

    mask [F,H,W] int64 class maps on the GPU; ``regions`` lists (class_bits, search_cls[, exclude_bits]) per frame in output order:
    a pixel is in the region iff bit mask[p] of class_bits is set, and a boundary point is dropped when a pixel of its 3x3
    neighbourhood has its bit set in exclude_bits.  ``draws``: None -- generated on the device from ``seed``, one stream per region, so
    a frame's result does not depend on its place in the batch -- or an int32 table
    [R*F, iters+1, n_min] of indices into each row's point list.  ``iters=-1``: the all-points fit only.  ``max_pts`` (even, at most
    16384) caps a row's point list; a row with more is absent and sets status bit 1.
    Returns (init [R*F,5] float64, frame_of [R*F] int32, cls [R*F] int32) on the device, the triple of ellipse_seeds_from_mask:
    init is the fitted ellipse in the search's convention, absent rows are -1 five times with frame_of = -1.  With
    ``return_stats`` also raw [R*F,5] (the reference's cx, cy, a, b, theta), stats_i int32 [R*F,4] (N, best iteration, inliers of the
    best, candidates), stats_f float64 [R*F,2] (best error, my_ellipse(raw).verify(points)), the int32 status word (bit 0: a bad
    draw, bit 1: more than max_pts points), points int16 [R*F,max_pts,2] (-1 past N) and the draws int32 [R*F,iters+1,n_min].
    Nothing here synchronises; the estimator is the reference's, with its tight threshold: no robustness to occlusion is claimed."""
    require_cuda(mask, "mask")
    if mask.dtype != torch.int64 or mask.dim() != 3:
        raise ValueError("mask must be an int64 [F,H,W] tensor")
    L = _lib.lib()
    dev = mask.device
    F, H, W = (int(v) for v in mask.shape)
    n_min, iters, n_good, max_pts = int(n_min), int(iters), int(n_good), int(max_pts)
    if not (1 <= n_min <= 64 and -1 <= iters < 4096 and n_good >= 0):
        raise ValueError("ellipse_ransac_from_mask: n_min 1..64, iters -1..4095, n_good >= 0")
    fo_in, cb, sc, eb = _ransac_rows(DEFAULT_RANSAC_REGIONS if regions is None else regions, F, dev)
    n = int(fo_in.shape[0])
    nbytes = int(L.egne_ellipse_ransac_workspace_bytes(n, H, W, max_pts))
    if nbytes < 0 or max_pts % 2:
        raise ValueError("ellipse_ransac_from_mask: %d rows of %dx%d class maps, max_pts %d (2..1024 rows and columns, max_pts even and "
                         "at most 16384)" % (n, H, W, max_pts))
    K1 = iters + 1
    table = None if draws is None else _draw_table(draws, n, K1, n_min, dev)
    m = mask.contiguous()
    ws = torch.empty((nbytes + 7) // 8, dtype=torch.int64, device=dev)
    init = torch.empty((n, 5), dtype=torch.float64, device=dev)
    raw = torch.empty((n, 5), dtype=torch.float64, device=dev)
    fo = torch.empty((n,), dtype=torch.int32, device=dev)
    cl = torch.empty((n,), dtype=torch.int32, device=dev)
    stats_i = torch.empty((n, 4), dtype=torch.int32, device=dev)
    stats_f = torch.empty((n, 2), dtype=torch.float64, device=dev)
    status = torch.empty((1,), dtype=torch.int32, device=dev)
    points = torch.full((n, max_pts, 2), -1, dtype=torch.int16, device=dev) if return_stats else None
    draws_out = torch.empty((n, K1, n_min), dtype=torch.int32, device=dev) if (return_stats and table is None and K1 > 0) else None
    _lib.check(L.egne_ellipse_ransac_from_mask(m.data_ptr(), F, fo_in.data_ptr(), cb.data_ptr(), sc.data_ptr(), eb.data_ptr(), n, H, W,
                                               max_pts, n_min, iters, float(thres), n_good,
                                               None if table is None else table.data_ptr(), int(seed) & 0xffffffff, n // F,
                                               None if draws_out is None else draws_out.data_ptr(), raw.data_ptr(), init.data_ptr(),
                                               fo.data_ptr(), cl.data_ptr(), stats_i.data_ptr(), stats_f.data_ptr(),
                                               None if points is None else points.data_ptr(), status.data_ptr(), ws.data_ptr(),
                                               _lib.stream_ptr()), "ellipse_ransac_from_mask")
    if not return_stats:
        return init, fo, cl
    used = table if table is not None else (draws_out if draws_out is not None else torch.empty((n, 0, n_min), dtype=torch.int32, device=dev))
    return init, fo, cl, raw, stats_i, stats_f, status, points, used


def fit_ellipses_from_mask(mask, regions=None, min_area=7, out=None, seed_kind="mask", **ransac_args):
    """fit_ellipses_from_pred with the seeds of ellipse_seeds_from_mask: seeds, then every search in one launch on the same stream.
    Returns a DEVICE tensor [F,R,5] float64, region order as in ``regions`` (default: iris, pupil); absent rows are -1 five times
    (the search reports NaN for them; a device-side select puts the seed's -1 back).  Nothing here synchronises.
    ``regions=None``: the default regions of the seed kind.  ``seed_kind="ransac"``: the seeds are those of
    ellipse_ransac_from_mask(mask, regions, **ransac_args); min_area is not used."""
    if seed_kind == "ransac":
        init, fo, cl = ellipse_ransac_from_mask(mask, regions, **ransac_args)
    elif seed_kind == "mask":
        if ransac_args:
            raise TypeError("fit_ellipses_from_mask: %r only with seed_kind='ransac'" % (sorted(ransac_args),))
        init, fo, cl = ellipse_seeds_from_mask(mask, regions, min_area)
    else:
        raise ValueError("fit_ellipses_from_mask: seed_kind %r (mask or ransac)" % (seed_kind,))
    L = _lib.lib()
    F, H, W = mask.shape
    R = init.shape[0] // F
    res = torch.empty((F * R, 5), dtype=torch.float64, device=mask.device)
    xs, ys = _mesh_axes(H, W, mask.device)
    m = mask.contiguous()
    _lib.check(L.egne_ellipse_fit(m.data_ptr(), F, fo.data_ptr(), cl.data_ptr(), F * R, H, W, xs.data_ptr(), ys.data_ptr(),
                                  init.data_ptr(), res.data_ptr(), None, _lib.stream_ptr()), "ellipse_fit")
    sel = torch.where((fo < 0)[:, None], init, res).view(F, R, 5)
    if out is None:
        return sel
    out.copy_(sel)
    return out


def search_proper_parameter_iou_for_our_data(seg, ell_para):
    """utils.py:450-486, same signature: seg [H,W] bool tensor on the GPU, ell_para (5,) pixels."""
    require_cuda(seg, "seg")
    res = fit_ellipses(seg.to(torch.int64)[None], [0], [1], np.asarray(ell_para, dtype=np.float64)[None, :5])
    return res[0]
