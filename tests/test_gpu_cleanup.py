"""-m gpu: class-map clean-up (csrc/cleanup.hip, utils.clean_class_maps, evaluate.py --clean_mask 1) against the NumPy restatement of
tests/cleanup_refs.py.  Integer work: every comparison -- cleaned map, statistics, status word -- is for exact equality."""
import numpy as np
import pytest
import torch

import cleanup_refs as R
import video_harness as V

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENTINEL = -77


@pytest.fixture(autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


@pytest.fixture(scope="module")
def nets():
    from common import bdcn_module, esf_module
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    dev = torch.device(DEV)
    return bdcn_module().to(dev), esf_module("baseline_edge").to(dev).eval()


def _i32(a):
    return torch.from_numpy(np.asarray(a, dtype=np.int64).astype(np.uint32).view(np.int32)).to(DEV)      # (bit patterns)


def _call(mask_t, out_t, frame_of, class_bits, paint_cls, flags, H, W, do_open=1, min_area=1, fill_cls=0, ws_bytes=None):
    """egne_class_map_cleanup on arbitrary rows and buffers -> (return code, stats, status); stats / status pre-filled with SENTINEL."""
    from egne_amd import _lib
    L = _lib.lib()
    n = len(frame_of)
    nbytes = int(L.egne_class_map_cleanup_workspace_bytes(n, H, W)) if ws_bytes is None else ws_bytes
    ws = torch.empty((max(nbytes, 8) + 7) // 8, dtype=torch.int64, device=DEV)
    stats = torch.full((n, 4), SENTINEL, dtype=torch.int64, device=DEV)
    status = torch.full((1,), SENTINEL, dtype=torch.int32, device=DEV)
    rows = [_i32(a) for a in (frame_of, class_bits, paint_cls, flags)]
    rc = L.egne_class_map_cleanup(mask_t.data_ptr(), int(mask_t.shape[0]), *(r.data_ptr() for r in rows), n, H, W, int(do_open),
                                  int(min_area), int(fill_cls), out_t.data_ptr(), stats.data_ptr(), status.data_ptr(), ws.data_ptr(),
                                  _lib.stream_ptr())
    torch.cuda.synchronize()
    return rc, stats.cpu().numpy(), status.cpu().numpy()


def _rows(mask, frame_of, class_bits, paint_cls, flags, **kw):
    F, H, W = mask.shape
    m = torch.from_numpy(np.ascontiguousarray(mask)).to(DEV)
    out = torch.full((F, H, W), SENTINEL, dtype=torch.int64, device=DEV)
    rc, stats, status = _call(m, out, frame_of, class_bits, paint_cls, flags, H, W, **kw)
    assert rc == 0
    return out.cpu().numpy(), stats, status


def _expect(got, want, what):
    out, stats, status = got
    w_out, w_stats = want
    assert int(status[0]) == 0, "%s: status %d" % (what, status[0])
    assert np.array_equal(stats, w_stats), "%s: stats\n%s\nwant\n%s" % (what, stats, w_stats)
    bad = np.argwhere(out != w_out)
    assert len(bad) == 0, "%s: %d pixels differ, first (frame, row, column) %s: %d, want %d" % (
        what, len(bad), bad[0].tolist(), out[tuple(bad[0])], w_out[tuple(bad[0])])


@pytest.mark.parametrize("shape", R.SHAPES, ids=lambda s: "%dx%d" % s)
def test_patterns(shape):
    """Every map that fits the shape, one frame each, in one call per setting: the pattern's class painted as 2, then the background
    class painted as 5 over it (with filling the second row covers the first one's blobs: the later row wins), fill_cls 9.  All four
    flag values, with and without the opening, min_area 1 and 7."""
    H, W = shape
    maps = R.maps(H, W)
    names = list(maps)
    mask = np.stack([maps[k] for k in names])
    F = len(names)
    cache = {}
    for flags in range(4):
        layers = tuple((b, c, flags) for b, c in R.TEST_ROWS)
        rows = R.layer_rows(layers, F)
        for do_open in (0, 1):
            for min_area in (1, 7):
                want = R.clean_rows(mask, *rows, do_open=bool(do_open), min_area=min_area, fill_cls=9, cache=cache)
                got = _rows(mask, *rows, do_open=do_open, min_area=min_area, fill_cls=9)
                _expect(got, want, "%dx%d flags %d open %d min_area %d (frames: %s)" % (H, W, flags, do_open, min_area, names))
    if "diag_ring" in maps:          # the restatement itself says: filled / not filled
        out, _ = R.clean(mask[[names.index("diag_ring"), names.index("diag_ring_gap")]], ((0b100, 2, 3),), do_open=False)
        assert np.count_nonzero(out[0] == 2) == 12 + 9 and np.count_nonzero(out[1] == 2) == 11


def _eye_maps(F, H, W, seed):
    """Class maps {0, 1, 2} with the look of a network's: a pupil disc inside an iris disc, speckle of all three classes, holes."""
    rng = np.random.RandomState(seed)
    yy, xx = np.mgrid[0:H, 0:W]
    out = np.zeros((F, H, W), np.int64)
    for f in range(F):
        cy, cx, r = rng.uniform(0.3, 0.7) * H, rng.uniform(0.3, 0.7) * W, rng.uniform(0.2, 0.4) * min(H, W)
        d = np.hypot(yy - cy, xx - cx)
        m = np.where(d < 0.45 * r, 2, np.where(d < r, 1, 0))
        noise = rng.rand(H, W)
        m = np.where(noise < 0.06, rng.randint(0, 3, (H, W)), m)
        out[f] = m
    return out


@pytest.mark.parametrize("F,H,W", [(3, 240, 320), (65, 61, 83)])
def test_batches_default_layers(F, H, W):
    from egne_amd.utils import DEFAULT_CLEAN_LAYERS, clean_class_maps
    assert DEFAULT_CLEAN_LAYERS == R.DEFAULT_LAYERS
    mask = _eye_maps(F, H, W, seed=F)
    out, stats, status = clean_class_maps(torch.from_numpy(mask).to(DEV), return_stats=True)
    assert out.dtype == torch.int64 and tuple(out.shape) == (F, H, W) and tuple(stats.shape) == (2 * F, 4)
    _expect((out.cpu().numpy(), stats.cpu().numpy(), status.cpu().numpy()), R.clean(mask), "default layers, %d frames" % F)
    assert set(np.unique(out.cpu().numpy())) <= {0, 1, 2} and not np.array_equal(out.cpu().numpy(), mask)
    again = torch.full((F, H, W), SENTINEL, dtype=torch.int64, device=DEV)
    assert clean_class_maps(torch.from_numpy(mask).to(DEV), out=again) is again and torch.equal(again, out)


def test_rows_of_every_kind():
    """Rows naming absent frames, class_bits = 0, two rows of one frame painting overlapping sets, a frame with no row, fill_cls 7."""
    H, W = 61, 83
    mask = _eye_maps(4, H, W, seed=9)
    mask[1, 5:9, 70:80] = 40                                  # an id outside 0..31: never eligible
    frame_of = [0, 0, -1, 4, 1000, 2, 2, 0, 2, 1]             # frame 3 has no row
    class_bits = [0b110, 0b100, 0b110, 0b110, 0b010, 0b111, 0b110, 0, 0b100, 1 << 31 | 0b001]
    paint_cls = [1, 2, 3, 3, 3, 4, 1, 6, 2, -5]
    flags = [3, 3, 3, 3, 3, 2, 1, 3, 0, 3]
    for do_open in (0, 1):
        want = R.clean_rows(mask, frame_of, class_bits, paint_cls, flags, do_open=bool(do_open), min_area=3, fill_cls=7)
        got = _rows(mask, frame_of, class_bits, paint_cls, flags, do_open=do_open, min_area=3, fill_cls=7)
        _expect(got, want, "mixed rows, open %d" % do_open)
        assert np.all(got[0][3] == 7) and np.all(got[1][[2, 3, 4, 7]] == 0)
        # frame 2: row 5 paints every class (the whole frame but what the opening drops) as 4, row 6 the iris blob over it, row 8 class 2
        assert {1, 2, 4} <= set(np.unique(got[0][2]))


@pytest.mark.parametrize("H,W", [(1025, 1024), (8, 1025), (8, 1)])
def test_refused_shapes_write_nothing(H, W):
    from egne_amd import _lib
    from egne_amd.utils import clean_class_maps
    assert _lib.lib().egne_class_map_cleanup_workspace_bytes(2, H, W) == -1
    m = torch.ones((1, H, W), dtype=torch.int64, device=DEV)
    out = torch.full((1, H, W), SENTINEL, dtype=torch.int64, device=DEV)
    rc, stats, status = _call(m, out, [0, 0], [0b110, 0b100], [1, 2], [3, 3], H, W, ws_bytes=64)
    assert rc != 0
    assert torch.all(out == SENTINEL) and np.all(stats == SENTINEL) and np.all(status == SENTINEL)
    with pytest.raises(ValueError):
        clean_class_maps(m)


def test_overlapping_out_is_refused_and_writes_nothing():
    from egne_amd import _lib
    from egne_amd.utils import clean_class_maps
    H, W = 16, 24
    for shift in (0, 1, H * W, 2 * H * W - 1):                # the same buffer .. the last pixel of mask = the first of out
        big = torch.ones(4 * H * W + 8, dtype=torch.int64, device=DEV)
        m, out = big[:2 * H * W].view(2, H, W), big[shift:shift + 2 * H * W].view(2, H, W)
        rc, stats, status = _call(m, out, [0, 1], [0b010, 0b010], [5, 5], [3, 3], H, W)
        assert rc != 0 and b"overlaps" in _lib.lib().egne_last_error()
        assert torch.all(big == 1) and np.all(stats == SENTINEL) and np.all(status == SENTINEL)
        with pytest.raises(ValueError):
            clean_class_maps(m, out=out)
    big = torch.ones(4 * H * W, dtype=torch.int64, device=DEV)
    m, out = big[:2 * H * W].view(2, H, W), big[2 * H * W:].view(2, H, W)          # adjacent: taken
    assert _call(m, out, [0, 1], [0b010, 0b010], [5, 5], [0, 0], H, W, do_open=0)[0] == 0
    assert torch.all(out == 5)


def test_argument_checks():
    from egne_amd.utils import clean_class_maps
    m = torch.zeros((1, 8, 8), dtype=torch.int64, device=DEV)
    for bad in ((), ((1, 2),), ((1 << 32, 1, 3),), ((-1, 1, 3),), ((1, 1, 4),), ((1, 1 << 31, 0),)):
        with pytest.raises(ValueError):
            clean_class_maps(m, layers=bad)
    with pytest.raises(ValueError):
        clean_class_maps(m, min_area=0)
    with pytest.raises(ValueError):
        clean_class_maps(m.to(torch.int32))
    with pytest.raises(ValueError):
        clean_class_maps(m[0])
    with pytest.raises(ValueError):
        clean_class_maps(m, out=torch.zeros((1, 8, 9), dtype=torch.int64, device=DEV))
    with pytest.raises(RuntimeError):          # (engine.require_cuda: the package has no CPU path)
        clean_class_maps(m.cpu())


@pytest.mark.parametrize("seed_kind", ["mask", "ransac"])
def test_downstream_fit_reads_the_cleaned_map(seed_kind):
    """fit_ellipses_from_mask on the device's cleaned map = the same call on the restatement's cleaned map uploaded as it is."""
    from egne_amd.utils import clean_class_maps, fit_ellipses_from_mask
    mask = _eye_maps(3, 240, 320, seed=21)
    got = fit_ellipses_from_mask(clean_class_maps(torch.from_numpy(mask).to(DEV)), seed_kind=seed_kind)
    want = fit_ellipses_from_mask(torch.from_numpy(R.clean(mask)[0]).to(DEV), seed_kind=seed_kind)
    assert tuple(got.shape) == (3, 2, 5) and torch.equal(got.view(torch.int64), want.view(torch.int64))          # bit for bit
    assert bool(torch.all(got[:, :, 2] > 0))


# ---- script level --------------------------------------------------------------------------------------------------------------------
def _video(vid, tmp_path, nets, monkeypatch, extra, method):
    """evaluate_ellseg_per_video with --clean_mask 1 -> (ellipse dictionary, equal to the one on disk, the frames handed to the two
    video writers, how many times the clean-up stage was called)."""
    import egne_amd.utils as U
    calls, real_clean = [], U.clean_class_maps

    def clean(mask, layers, *a, **k):
        calls.append(layers)
        return real_clean(mask, layers, *a, **k)
    monkeypatch.setattr(U, "clean_class_maps", clean)
    r = V.run(vid, tmp_path, nets, ["--clean_mask", "1"] + extra, method)
    monkeypatch.undo()
    V.same_ellipses(r.files[0], r.res, equal_nan=True)
    return r.res, r.written, calls


def _equal(res_a, res_b):
    V.same_ellipses(res_a, res_b, equal_nan=True)


@pytest.mark.parametrize("seed", ["pred", "mask"])
def test_video_clean_mask_same_results_through_every_path(tmp_path, nets, monkeypatch, seed):
    """--clean_mask 1 on the clip of test_evaluate_video_end_to_end: the batched loop, --low_latency 1 and --device_io 1 --low_latency 1
    (the stage inside the captured graph) write the same ellipses; --device_io 0 and 1 hand byte-identical frames to both video
    writers.  A first run calibrates the plans."""
    from egne_amd.utils import DEFAULT_CLEAN_LAYERS
    vid = V.clip(tmp_path)
    extra = ["--ellipse_seed", seed]
    _video(vid, tmp_path, nets, monkeypatch, extra, "warm")
    host, wr_h, calls_h = _video(vid, tmp_path, nets, monkeypatch, extra, "host")
    dev, wr_d, calls_d = _video(vid, tmp_path, nets, monkeypatch, extra + ["--device_io", "1"], "dev")
    live, wr_lh, calls_l = _video(vid, tmp_path, nets, monkeypatch, extra + ["--low_latency", "1"], "live")
    live_io, wr_l, calls_lio = _video(vid, tmp_path, nets, monkeypatch, extra + ["--device_io", "1", "--low_latency", "1"], "liveio")
    assert set(k for k in host if isinstance(k, int)) == {0, 1, 2, 3} and all((j, i) in host for j in range(4) for i in range(2))
    for calls in (calls_h, calls_d, calls_l, calls_lio):
        assert calls and all(c == DEFAULT_CLEAN_LAYERS for c in calls)
    _equal(host, dev)
    _equal(live, live_io)
    if seed == "mask":
        # seeds from the (integer) cleaned map: the batch size cannot show.  The regression head's float seeds differ in their last
        # bits between a batch of eight and a batch of two, with or without the clean-up, so 'pred' is compared at equal batching only
        _equal(host, live)
        _equal(host, live_io)
    for wr_0, wr in ((wr_h, wr_d), (wr_lh, wr_l)):          # --device_io 0 against 1, in the batched loop and under --low_latency 1
        assert [w[0] for w in wr_0] == [w[0] for w in wr] and len(wr) == 8
        for (kind, fa), (_, fb) in zip(wr_0, wr):
            assert fa.dtype == np.uint8 and fa.shape == fb.shape == (240, 640, 3)
            assert np.array_equal(fa, fb), "%s frame differs in %d bytes" % (kind, np.count_nonzero(fa != fb))


def test_video_flag_off_is_the_raw_map(tmp_path, nets, monkeypatch):
    """The flag left at its default never calls the stage; --clean_mask 1 does, and the maps the renderer draws change with it (seeded
    random weights give ragged maps)."""
    import egne_amd.utils as U
    from egne_amd import evaluate as E
    bd, net = nets
    calls = []
    real = U.clean_class_maps
    monkeypatch.setattr(U, "clean_class_maps", lambda *a, **k: calls.append(1) or real(*a, **k))
    from common import gold
    g = gold("evaluate_real_frames")
    x = torch.stack([E.preprocess_frame(e, (240, 320))[0] for e in g["eyes"][:2]]).to(DEV)
    E.evaluate_ellseg_on_image(x, net, bd, E.parse_args([]))          # (calibrates the plans)
    raw = E.evaluate_ellseg_on_image(x, net, bd, E.parse_args([]))
    assert not calls
    cleaned = E.evaluate_ellseg_on_image(x, net, bd, E.parse_args(["--clean_mask", "1"]))
    assert len(calls) == 1
    assert np.array_equal(cleaned[1], R.clean(raw[1])[0])          # what evaluate_ellseg_on_image returns IS the cleaned map
    assert np.array_equal(raw[0], cleaned[0])


def test_deepvog_cleans_with_its_own_layers(monkeypatch):
    """--model deepvog --clean_mask 1: the class maps {0, 1 = pupil} are cleaned with CLEAN_LAYERS['deepvog'] and returned cleaned."""
    import egne_amd.utils as U
    from egne_amd import evaluate as E
    seen, results = [], []
    real_clean, real_eval = U.clean_class_maps, E.evaluate_ellseg_on_image

    def clean(mask, layers, *a, **k):
        out = real_clean(mask, layers, *a, **k)
        seen.append((mask.cpu().numpy().copy(), layers, out.cpu().numpy().copy()))
        return out

    def spy(*a, **k):
        results.append(real_eval(*a, **k))
        return results[-1]
    monkeypatch.setattr(U, "clean_class_maps", clean)
    monkeypatch.setattr(E, "evaluate_ellseg_on_image", spy)
    E.main(["--synthetic", "2", "--model", "deepvog", "--ellipse_seed", "mask", "--clean_mask", "1"])
    raw, layers, cleaned = seen[-1]
    assert layers == E.CLEAN_LAYERS["deepvog"] == ((0b010, 1, 3),)
    assert set(np.unique(raw)) <= {0, 1}
    assert np.array_equal(cleaned, R.clean(raw, layers)[0])
    assert np.array_equal(results[-1][1], cleaned)


def test_capture_replays_equal_the_eager_call(nets):
    """graphed_runner(..., clean=...) replayed three times on different frames: what the eager call returns for them, bit for bit."""
    import argparse
    from egne_amd import synth
    from egne_amd.evaluate import _seg_and_fit, graphed_runner
    from egne_amd.utils import DEFAULT_CLEAN_LAYERS, calc_edge
    bd, net = nets
    ns = argparse.Namespace(prec=torch.float32, edge_thres=0)
    warm = synth.make_batch(2, seed=5)["img"].to(DEV)
    run = graphed_runner(warm, net, bd, seed="mask", clean=DEFAULT_CLEAN_LAYERS)
    for seed in (6, 7, 8):
        x = synth.make_batch(2, seed=seed)["img"].to(DEV)
        got = [t.clone() for t in run(x)]
        with torch.no_grad():
            want = _seg_and_fit(x, net, seed="mask", clean=DEFAULT_CLEAN_LAYERS)(calc_edge(ns, x, bd, DEV))
            raw = _seg_and_fit(x, net, seed="mask")(calc_edge(ns, x, bd, DEV))
        torch.cuda.synchronize()
        for a, b in zip(got, want):
            assert torch.equal(a.view(torch.int64) if a.dtype == torch.float64 else a, b.view(torch.int64) if b.dtype == torch.float64 else b)
        assert np.array_equal(got[1].cpu().numpy(), R.clean(raw[1].cpu().numpy())[0])
