"""CPU: the planner's kernel chooser (engine.choose_conv) against the C side's (egne_conv2d_auto_kind, csrc/dispatch.hip).  Both are host
code: the library loads and answers without a GPU."""
import ctypes as C
import json
import os
import random

from egne_amd import _lib, engine

HERE = os.path.dirname(os.path.abspath(__file__))


def _both(q):
    """(kind, frames go to a flat tail, pooled second output, fused statistics) of the Python and of the C chooser."""
    L = _lib.lib()
    mine = engine.choose_conv(q, L)
    ch = _lib.ConvChoice()
    _lib.check(L.egne_conv2d_auto_kind(C.byref(q), C.byref(ch)), "conv2d_auto_kind")
    return ((mine.kind, bool(mine.tail_frames), mine.fused_pool, mine.fused_stats),
            (ch.name.decode(), bool(ch.tail_frames), bool(ch.fused_pool), bool(ch.fused_stats)))


def _query(**fields):
    q = _lib.ConvQuery()
    for k, v in fields.items():
        if isinstance(v, (list, tuple)):
            arr = getattr(q, k)
            for i, e in enumerate(v):
                arr[i] = e
        else:
            setattr(q, k, v)
    return q


def test_table_of_planned_convolutions_replays():
    """tests/dispatch_table.json: the de-duplicated queries of every convolution in the plans of
    test_gpu_nets.test_c_side_dispatch_agrees_with_the_planner (edge network and ESF-Net at B = 64 and B = 2, training plans in both
    storages), with what the planner chose for them before the chooser became a function of its own.  Both choosers must still say so."""
    with open(os.path.join(HERE, "dispatch_table.json")) as f:
        table = json.load(f)
    names, rows = table["fields"], table["rows"]
    assert len(rows) >= 150
    kinds = set()
    for row in rows:
        r = dict(zip(names, row))
        want = (r.pop("kind"), bool(r.pop("tail")), bool(r.pop("fused_pool")), bool(r.pop("fused_stats")))
        kinds.add(want[0])
        mine, theirs = _both(_query(**r))
        assert mine == want, (r, mine, want)
        assert theirs == want, (r, theirs, want)
    assert {"conv_f16x3:big", "conv_f16x3:rw", "conv_f16x3:halo", "conv_f16x3:msdil", "conv_f16x3:first", "conv_f16x3:stream1x1", "conv_f16x3:gemm1x1",
            "conv_f16x3:small", "conv3x3_narrow", "conv_igemm", "conv_bf16:3x3", "conv_bf16:1x1", "conv3x3_smallcin"} <= kinds, sorted(kinds)


FLAGS = ("has_residual", "has_post", "seg_affine", "want_stats", "want_pool", "up_add", "train", "dyn_scales", "split", "split1")


def _sweep_queries(n, seed):
    """Queries around every threshold the chooser names (map width, batch, slice width, output width, kernel, stride, dilation, groups,
    segments, every flag, products, storage type), drawn with a fixed seed."""
    rng = random.Random(seed)
    pad8 = engine.pad8
    for _ in range(n):
        W = rng.choice((19, 20, 29, 30, 59, 60, 119, 120, 320))
        Cp = rng.choice((8, 32, 40, 48, 64, 96, 128, 512, 544))
        Cout = rng.choice((3, 4, 32, 64, 96, 128, 256))
        # (the "same" 3x3 at stride 1 over fp32 tensors is where most of the kernels compete: drawn more often than the other values)
        k, pad = rng.choice(((1, 0), (3, 1), (3, 1), (3, 1), (3, 0), (7, 3)))
        groups = rng.choice(((1,), (1,), (4, 8, 12), (1, 2, 3)))
        dil = list(groups) if len(groups) == 3 else [rng.choice((1, 2))]
        nseg = rng.choice((1, 3)) if k == 1 else 1
        seg_Cp = [Cp] + [32] * (nseg - 1)
        seg_C = [4 if Cp == 8 else Cp] + [32] * (nseg - 1)
        # every flag on and off; half of the queries with the flags that take kernels away mostly off and the split-f16 permissions
        # mostly on, so that the rarer kernels are reached often too
        p_off, p_on = rng.choice(((0.5, 0.5), (0.15, 0.85)))
        flag = {f: int(rng.random() < (p_on if f in ("split", "split1") else p_off)) for f in FLAGS}
        affine = flag.pop("seg_affine")
        f = dict(dtype=rng.choice((0, 0, 1)), B=rng.choice((1, 2, 64)), H=3 * W // 4, W=W, kh=k, kw=k, stride=rng.choice((1, 1, 1, 2)), pad_h=pad, pad_w=pad,
                 ngroups=len(dil), dil=dil + [1] * (_lib.MAXGROUP - len(dil)), nseg=nseg, seg_C=seg_C, seg_Cp=seg_Cp,
                 seg_ch_off=[sum(seg_Cp[:i]) for i in range(nseg)], seg_pix_stride=[sum(seg_Cp)] * nseg, seg_affine=[affine] * nseg,
                 Cout=Cout, Cout_store=pad8(Cout), dst_Cp=pad8(Cout), dst_pix_stride=pad8(Cout), act=rng.choice((_lib.ACT_NONE, _lib.ACT_RELU)),
                 f16_products=rng.randint(0, 1), **flag)
        if f["has_residual"]:
            f["res_pix_stride"] = pad8(Cout)
        if f["want_pool"]:
            f["pool_Cp"], f["pool_pix_stride"] = pad8(Cout), pad8(Cout)
        yield f


def test_choosers_agree_around_every_threshold():
    n, kinds = 0, set()
    for f in _sweep_queries(50000, seed=20260101):
        mine, theirs = _both(_query(**f))
        assert mine == theirs, (f, mine, theirs)
        kinds.add(mine[0])
        n += 1
    # every kind the axes can describe (conv_bf16:narrow needs an answer of egne_conv_narrow_bf16_supported, which the sweep leaves at 0)
    assert n == 50000 and kinds == set(engine._KIND) - {"conv_bf16:narrow"}, sorted(kinds)
