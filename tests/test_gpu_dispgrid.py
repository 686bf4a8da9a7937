"""-m gpu: the prediction overlay grid on the device (egne_disp_grid, egne_amd.dispgrid.image_grid / save_grid): float grid, uint8 image
and status words bit for bit against the restatement of tests/dispgrid_refs.py (which tests/test_host_dispgrid.py holds against what
the reference's generateImageGrid recorded), the recorded grids themselves, the edge cases, graph capture and the JPEG file."""
import io
import os

import numpy as np
import pytest
import torch

import dispgrid_refs as R
import jpeg_refs as J

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "dispgrid.npz")


@pytest.fixture(autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _D():
    from egne_amd import dispgrid
    return dispgrid


def _dev(a):
    return None if a is None else torch.from_numpy(np.array(a, copy=True, order="C")).to(DEV)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _run(inp, **kw):
    """image_grid on the arrays of ``inp``: (grid, u8, status) as NumPy arrays."""
    g, u8, st = _D().image_grid(_dev(inp["img"]), _dev(inp["mask"]), _dev(inp["el"]), None, _dev(inp.get("cond")), _dev(inp.get("el_gt")),
                                return_u8=True, return_status=True, **kw)
    torch.cuda.synchronize()
    return g.cpu().numpy(), u8.cpu().numpy(), st.cpu().numpy()


def _same(got, want, what):
    g, u8, st = got
    wg, wu8, wst = want
    assert g.shape == wg.shape and u8.shape == wu8.shape and g.dtype == np.float32 and u8.dtype == np.uint8, what
    assert np.array_equal(st, wst), (what, st, wst)
    bad = np.argwhere(_bits(g) != _bits(wg))
    assert bad.size == 0, "%s: %d grid values differ, first at %s: %r, restatement %r" % (
        what, len(bad), bad[0], g[tuple(bad[0])], wg[tuple(bad[0])])
    assert np.array_equal(u8, wu8), what


_CACHE = {}


def _reference(key, inp, **kw):
    """The restatement of a case, computed once and shared."""
    if key not in _CACHE:
        _CACHE[key] = R.image_grid(inp["img"], inp["mask"], inp["el"], inp.get("cond"), inp.get("el_gt"), **kw)
    return _CACHE[key]


@pytest.mark.parametrize("name", sorted(R.FIXTURE_CASES))
def test_golden_cases(name):
    """Every case of the golden file: the device equals the restatement and the grid the reference's function returned, exactly."""
    G = np.load(GOLDEN, allow_pickle=False)
    inp, override = R.fixture_inputs(name)
    got = _run(inp, override=override)
    _same(got, _reference(("golden", name), inp, override=override), name)
    assert R.sha(got[0]) == str(G[name + "_grid_sha"])
    assert np.array_equal(got[1], G[name + "_grid_u8"])
    if name + "_grid" in G.files:
        assert np.array_equal(_bits(got[0]), _bits(G[name + "_grid"]))


@pytest.mark.parametrize("name", sorted(R.SEEDED_CASES))
def test_seeded_cases(name):
    B, H, W, seed, count, nrow = R.SEEDED_CASES[name]
    inp = R.inputs(B, H, W, seed)
    want = _reference(("seeded", name), inp, override=True, count=count, nrow=nrow)
    if name == "big_strided":       # every other frame of a batch twice as long
        D = _D()
        wide = {k: _dev(np.repeat(v, 2, axis=0)) for k, v in inp.items()}
        for k in ("img", "mask"):
            wide[k][1::2] = 0
        g, u8, st = D.image_grid(wide["img"][::2], wide["mask"][::2], wide["el"][::2], None, wide["cond"][::2], wide["el_gt"][::2],
                                 override=True, count=count, nrow=nrow, return_u8=True, return_status=True)
        assert not wide["img"][::2].is_contiguous()
        torch.cuda.synchronize()
        got = (g.cpu().numpy(), u8.cpu().numpy(), st.cpu().numpy())
    else:
        got = _run(inp, override=True, count=count, nrow=nrow)
    _same(got, want, name)
    assert got[0].shape == (3,) + R.grid_shape(min(count, B), nrow, H, W)
    if name == "two_rows":
        assert got[0].shape == (3, 102, 266) and not got[0][:, 52:, 68:].any()          # the cells behind the fifth frame stay zero
    # two calls give the same bytes
    again = _run(inp, override=True, count=count, nrow=nrow) if name != "big_strided" else got
    assert all(np.array_equal(a.view(np.uint8), b.view(np.uint8)) for a, b in zip(got, again))


def _edge_inputs():
    inp = R.inputs(4, 33, 47, 21)
    H, W = 33, 47
    rng = np.random.RandomState(3)
    inp["img"][0] = np.float32(0.375)                                           # constant
    inp["img"][1, 7, 9] = np.nan                                                # one NaN
    inp["img"][2] = np.where(rng.rand(H, W) < 0.4, np.float32(-1.5), np.float32(0.25))      # two grey levels
    inp["img"][3] = np.abs(inp["img"][3]); inp["img"][3, 5, 5] = -0.0; inp["img"][3, 6, 6] = 0.0     # the minimum is negative zero
    inp["el"][0, 0] = np.nan                                                    # degenerate ellipses: status bits 2-5
    inp["el"][2, 1, 2] = 1e-4                                                   # a pupil axis below one pixel
    inp["el_gt"][2, 0, 3] = np.nan
    inp["el_gt"][3, 1, 3] = 1e-5
    return inp


def test_edge_cases():
    inp = _edge_inputs()
    want = R.image_grid(inp["img"], inp["mask"], inp["el"], inp["cond"], inp["el_gt"], override=True, draw_gt=True)
    assert list(want[2]) == [R.ST_CONSTANT | R.ST_SKIP_IRIS, R.ST_NONFINITE, R.ST_SKIP_PUPIL | R.ST_SKIP_GT_IRIS, R.ST_SKIP_GT_PUPIL]
    got = _run(inp, override=True, draw_gt=True)
    assert np.array_equal(got[2], want[2]), (got[2], want[2])
    H, W = 33, 47
    for i in range(4):          # the pixels of the frame with a NaN are unspecified; every other frame and the padding are pinned
        r0, c0 = R.grid_origin(i, 4, 4, H, W)
        if i == 1:
            got[0][:, r0:r0 + H, c0:c0 + W] = want[0][:, r0:r0 + H, c0:c0 + W]
            got[1][r0:r0 + H, c0:c0 + W] = want[1][r0:r0 + H, c0:c0 + W]
    _same(got, want, "edge cases")
    r0, c0 = R.grid_origin(0, 4, 4, H, W)
    tile = got[0][:, r0:r0 + H, c0:c0 + W]
    assert set(np.unique(tile)) <= {0.0, 102.0, 255.0} and (tile[:, inp["mask"][0] == 0] != 0).sum() > 0       # grey 0 under the paints
    assert (want[0] == 102).any()                                               # the ground-truth colour is there


def test_draw_gt_off_and_cond_none():
    inp = R.inputs(3, 33, 47, 22)
    for kw in (dict(override=False), dict(override=True, draw_gt=False)):
        _same(_run(inp, **kw), R.image_grid(inp["img"], inp["mask"], inp["el"], inp["cond"], inp["el_gt"], **kw), str(kw))
    bare = {k: inp[k] for k in ("img", "mask", "el")}                            # cond=None, override=False: no frame is painted
    got = _run(bare, override=False)
    _same(got, R.image_grid(inp["img"], inp["mask"], inp["el"]), "cond None")
    assert got[0].max() <= 1.0 and np.array_equal(got[0][0], got[0][1]) and np.array_equal(got[0][0], got[0][2])


def test_graph_capture_and_replay():
    D = _D()
    inp = R.inputs(3, 33, 47, 23)
    t = {k: _dev(v) for k, v in inp.items()}
    want = R.image_grid(inp["img"], inp["mask"], inp["el"], inp["cond"], inp["el_gt"], override=True)

    def call():
        return D.image_grid(t["img"], t["mask"], t["el"], None, t["cond"], t["el_gt"], override=True, return_u8=True, return_status=True)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        call()                                  # (uploads the outline table outside the capture)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = call()
    for o in out:
        o.fill_(7)
    graph.replay()
    torch.cuda.synchronize()
    _same(tuple(o.cpu().numpy() for o in out), want, "replay")
    # new frames in the same buffers, replayed
    inp2 = R.inputs(3, 33, 47, 24)
    for k in t:
        t[k].copy_(_dev(inp2[k]))
    graph.replay()
    torch.cuda.synchronize()
    _same(tuple(o.cpu().numpy() for o in out), R.image_grid(inp2["img"], inp2["mask"], inp2["el"], inp2["cond"], inp2["el_gt"], override=True),
          "second replay")


def test_save_grid_decodes_within_the_encoders_quality_bound(tmp_path):
    """The JPEG file of save_grid has the grid's size, and its PSNR against the uint8 image is at least PIL's own encoder's at the same
    quality minus the margin the encoder is held to (jpeg_refs.PSNR_MARGIN_DB, tests/test_host_jpeg.py)."""
    from PIL import Image
    D = _D()
    inp, override = R.fixture_inputs("five")
    g, u8 = D.image_grid(_dev(inp["img"]), _dev(inp["mask"]), _dev(inp["el"]), None, _dev(inp["cond"]), _dev(inp["el_gt"]), override=override,
                         return_u8=True)
    path = str(tmp_path / "grid.jpg")
    assert D.save_grid(path, u8) == path
    src = u8.cpu().numpy()
    im = Image.open(path)
    im.load()
    assert im.size == (src.shape[1], src.shape[0]) and im.mode == "RGB" and im.format == "JPEG"
    mine = J.psnr(np.asarray(im)[..., ::-1], src)
    buf = io.BytesIO()
    Image.fromarray(np.ascontiguousarray(src[..., ::-1])).save(buf, format="JPEG", quality=90)
    pil = J.psnr(np.asarray(Image.open(io.BytesIO(buf.getvalue())))[..., ::-1], src)
    print("save_grid: PSNR %.2f dB, PIL %.2f dB" % (mine, pil))
    assert mine >= pil - J.PSNR_MARGIN_DB


def test_wrong_inputs_raise():
    D = _D()
    inp = R.inputs(2, 13, 17, 25)
    t = {k: _dev(v) for k, v in inp.items()}
    ok = lambda **kw: D.image_grid(kw.get("img", t["img"]), kw.get("mask", t["mask"]), kw.get("el", t["el"]), None, kw.get("cond", t["cond"]),      # noqa: E731
                                   kw.get("el_gt", t["el_gt"]), **{k: v for k, v in kw.items() if k not in t})
    assert tuple(ok().shape) == (3, 17, 40)
    for bad in (dict(img=t["img"].double()), dict(img=t["img"].cpu()), dict(mask=t["mask"].int()), dict(mask=t["mask"][:, :12]),
                dict(el=t["el"].reshape(2, 10)), dict(el_gt=t["el_gt"][:1]), dict(cond=t["cond"][:, :1]), dict(cond=t["cond"].cpu()),
                dict(count=0), dict(nrow=0), dict(img=t["img"][:, :5], mask=t["mask"][:, :5]), dict(el_gt=None, draw_gt=True)):
        with pytest.raises(ValueError):
            ok(**bad)
    with pytest.raises(ValueError):
        D.save_grid("nowhere.jpg", t["img"])
    # the C entry point checks for itself
    from egne_amd import _lib
    L = _lib.lib()
    assert L.egne_disp_grid(None, None, None, None, None, 0, 1, 13, 17, 1, 0, 4, 4, None, None, None, None, None, None) != 0
    assert b"null pointer" in L.egne_last_error()
    assert L.egne_disp_grid_workspace_bytes(4) == 4 * 258 * 4
