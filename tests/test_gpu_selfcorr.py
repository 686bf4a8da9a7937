"""-m gpu: the self-consistency term (csrc/selfcorr.hip; ``model.selfCorr``, ``train.py --selfCorr 1``), one C-ABI call at a time and
through the networks.

Op level: egne_loss_fwd, then egne_selfcorr_fwd / egne_selfcorr_bwd, against float64 autograd of the stable restatement
(tests/selfcorr_refs.py, pinned to the reference by tests/test_host_selfcorr.py) under small_op_refs.bound (four times the CPU's fp32
error, floor 4 ulp).  egne_loss_fwd writes elPred with the soft-argmax centres of the logits; the cases need ellipses the soft-argmax
cannot produce (centres outside the frame), so the case's elPred is copied into the descriptor's buffer behind egne_loss_fwd.  The
term's three destinations are dense fp32 tensors without slice parameters: they are pre-filled with seeded values of the gradient's
size (so that the rounding of pre-fill + gradient stays at an ulp of the gradient's scale; the CPU yardstick takes the same sum) and
carry a POISON tail; the sliced logits destination belongs to egne_loss_bwd (test_gpu_small_ops.test_loss_head_backward).

Network level at 240x320, B = 2: loss and term against the reference's DenseNet2D with selfCorr = True (tests/golden/selfcorr.npz
part (b)), parameter gradients against the oracle's autograd of loss + 10 * term -- the reference's own are NaN."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest
import torch

import selfcorr_refs as S
import small_op_refs as R
from test_gpu_nets import _v1_args, _v1_model, bdcn, edge_of  # noqa: F401  (module-scoped fixtures and the comparator's builders)
from test_gpu_small_ops import BF, DEV, POISON, _buf, _check, _loss_inputs, _same32, _sync, lib  # noqa: F401

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "selfcorr.npz")
GSCALE = 0.7


@pytest.fixture(autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


OP_CASES = list(S.CASES)
OP_CASES += [((300, 4, 6), "some", "typical"), ((300, 4, 6), "none", "negative")]      # more samples than the combining block has threads
OP_CASES += [((2, 240, 320), "all", "typical")]                                       # the networks' size, once


def _prefill(ref64, seed):
    """Seeded non-zero pre-fill of a destination, of the gradient's own size."""
    g = torch.Generator().manual_seed(seed)
    scale = max(ref64.abs().max().item(), 1e-6)
    return ((0.25 + torch.rand(ref64.shape, generator=g)) * scale * (2 * torch.randint(0, 2, ref64.shape, generator=g) - 1)).float()


def _guarded(x):
    """x (CPU fp32) on the device with four POISON floats behind it."""
    t = torch.full((x.numel() + 4,), POISON, device=DEV)
    t[:x.numel()] = x.reshape(-1).to(DEV)
    return t


def _split_el(g_el):
    """d / d elPred [B,10] -> (d / d pred_c [B,2,2] (iris, pupil centres), d / d elOut [B,10] with the centre entries zero)."""
    pc = torch.stack((g_el[:, 0:2], g_el[:, 5:7]), 1)
    eo = g_el.clone()
    eo[:, 0:2] = 0
    eo[:, 5:7] = 0
    return pc, eo


@pytest.mark.parametrize("case", OP_CASES, ids=lambda c: S.case_key(*c))
def test_selfcorr_forward_and_backward(lib, case):
    """Both storages, two logits slices, forward and backward of one case.  MI355X, worst error over the 26 cases as a share of
    its bound: term 0.06, weight * term 0.11, increment of out_terms[0] 0.25, g_op 0.27, g_pred_c 0.73, g_elOut_up 0.86 (the last two on
    the 6 x 10 frame with negative angles: 8.4e-6 against the CPU's 2.4e-6; z = 64 (1 - q) multiplies the rounding of q by 64); the
    bf16 entry's fp32 outputs came back bit-identical to the fp32 entry's in every case."""
    _lib, L, st = lib
    shape, okp, es = case
    B, H, W = shape
    op, el, ok = S.case_inputs(shape, okp, es)
    t, _ = _loss_inputs(B, H, W, "none", 11 * B + W)
    t["op"] = op
    t["cond"][:, 1:] = (1 - ok)[:, None]
    r64 = S.value_and_grads(op.double(), el.double(), ok.double(), fn=S.weighted)
    r32 = S.value_and_grads(op, el, ok, fn=S.weighted)
    v64, v32 = S.term(op.double(), el.double(), ok.double()), S.term(op, el, ok)
    for x in r64 + r32:
        assert torch.isfinite(x).all()
    # upstream scale folded in: what the three destinations receive
    want64 = (GSCALE * r64[1],) + tuple(GSCALE * x for x in _split_el(r64[2]))
    want32 = (GSCALE * r32[1],) + tuple(GSCALE * x for x in _split_el(r32[2]))
    pre = [_prefill(w, 5 + i) for i, w in enumerate(want64)]
    cpu32 = [(p + w) - p for p, w in zip(pre, want32)]          # the yardstick rounds pre-fill + gradient as the kernel must

    dv = {k: v.to(DEV).contiguous() for k, v in t.items()}
    gx, gy = torch.linspace(-1, 1, W).to(DEV), torch.linspace(-1, 1, H).to(DEV)
    gsc = torch.tensor([GSCALE], device=DEV)
    outs = {}
    for dt in (torch.float32, BF):
        res = []
        for ps, co in ((8, 0), (16, 5)):
            logits = _buf(op.permute(0, 2, 3, 1), ps, co, dt)
            logits0 = logits.clone()
            part = torch.zeros(int(L.egne_loss_workspace_floats(B, H, W)), device=DEV)
            out_terms, pcd, elp = torch.zeros(8, device=DEV), torch.zeros(B, 2, 2, device=DEV), torch.zeros(B, 10, device=DEV)
            coef = torch.zeros(B, 32, device=DEV)
            d = _lib.LossDesc()
            d.B, d.H, d.W = B, H, W
            d.logits, d.pix_stride, d.ch_off, d.dtype = logits.data_ptr(), ps, co, (0 if dt == torch.float32 else 1)
            d.target, d.spatWts, d.distMap, d.cond = dv["tgt"].data_ptr(), dv["sw"].data_ptr(), dv["dist"].data_ptr(), dv["cond"].data_ptr()
            d.pupil_center, d.elNorm, d.elOut, d.alpha = dv["pc"].data_ptr(), dv["eln"].data_ptr(), dv["elOut"].data_ptr(), 0.3
            d.grid_x, d.grid_y = gx.data_ptr(), gy.data_ptr()
            d.partials, d.out_terms, d.pred_c, d.elPred = part.data_ptr(), out_terms.data_ptr(), pcd.data_ptr(), elp.data_ptr()
            d.coef = coef.data_ptr()
            _lib.check(L.egne_loss_fwd(C.byref(d), st), "loss")
            _sync()
            base = out_terms.cpu().clone()
            elp.copy_(el.to(DEV))
            nws = int(L.egne_selfcorr_workspace_floats(B, H, W))
            ws, sct = _guarded(torch.zeros(nws)), _guarded(torch.zeros(4))
            _lib.check(L.egne_selfcorr_fwd(C.byref(d), S.WEIGHT, ws.data_ptr(), sct.data_ptr(), st), "selfcorr_fwd")
            dst = [_guarded(p) for p in pre]
            _lib.check(L.egne_selfcorr_bwd(C.byref(d), S.WEIGHT, ws.data_ptr(), gsc.data_ptr(), dst[0].data_ptr(), dst[1].data_ptr(),
                                           dst[2].data_ptr(), st), "selfcorr_bwd")
            _sync()
            assert torch.equal(logits, logits0), "the logits are read only"
            for g in [ws, sct] + dst:
                assert (g[-4:] == POISON).all(), "a kernel wrote behind its buffer"
            after = out_terms.cpu()
            assert torch.equal(after[1:], base[1:]), "only out_terms[0] takes the term"
            got = [g[:-4].cpu().reshape(p.shape) for g, p in zip(dst, pre)]
            res.append((sct[:4].cpu(), after[0].double() - base[0].double(), base[0], got))
        a, b = res
        assert torch.equal(a[0], b[0]) and a[1] == b[1] and all(torch.equal(x, y) for x, y in zip(a[3], b[3])), \
            "the results must not depend on the logits' slice"
        outs[dt] = a
    sct, inc, base0, got = outs[torch.float32]
    tag = "selfcorr[%s]" % S.case_key(*case)
    for x in [sct] + got:
        assert torch.isfinite(x).all(), "non-finite output"
    n_ok = float(ok.sum())
    assert sct[1].item() == n_ok and sct[3].item() == 0.0
    if n_ok == 0:
        assert sct[0].item() == 0.0 and sct[2].item() == 0.0 and inc == 0.0
        for g, p in zip(got, pre):
            assert torch.equal(g, p), "ok none: every destination keeps its pre-fill"
    else:
        _check(tag + " term", sct[0:1], v64.reshape(1), v32.reshape(1))
        _check(tag + " weight * term", sct[2:3], r64[0].reshape(1), r32[0].reshape(1))
        inc32 = ((base0 + r32[0]) - base0).reshape(1)            # the fp32 sum out_terms[0] + 10 * term, as the CPU rounds it
        _check(tag + " increment of out_terms[0]", inc.reshape(1), r64[0].reshape(1), inc32)
        for name, g, p, w64, c32 in zip(("g_op", "g_pred_c", "g_elOut_up"), got, pre, want64, cpu32):
            _check("%s %s" % (tag, name), g.double() - p.double(), w64, c32)
        skip = (ok == 0)
        for g, p in zip(got, pre):
            assert torch.equal(g[skip], p[skip]), "a sample with ok = 0 keeps its pre-fill"
    assert torch.equal(got[2][:, 0:2], pre[2][:, 0:2]) and torch.equal(got[2][:, 5:7], pre[2][:, 5:7]), \
        "entries 0:2 and 5:7 of g_elOut_up belong to pred_c"
    # the bf16 entry reads the same (bf16-representable) logits: its fp32 outputs are held to the fp32 run's
    s16, i16, _, g16 = outs[BF]
    _same32(tag + " sc_terms", s16, sct)
    assert abs(i16 - inc) <= 1e-6 * max(abs(inc), 1e-30)
    for name, x16, x32 in zip(("g_op", "g_pred_c", "g_elOut_up"), g16, got):
        _same32("%s %s" % (tag, name), x16, x32)
    # where the reference's autograd gives NaN (fixture), the kernel gives the derivative
    key = "a_" + S.case_key(*case) + "_g_el_finite"
    gold = np.load(GOLD)
    if key in gold.files and es == "typical" and okp != "none":
        assert not gold[key][:, 5:].all(), "the fixture records NaN for the typical pupil ellipse"
        assert torch.isfinite(got[1]).all() and torch.isfinite(got[2]).all()


# ==== network level ====================================================================================================================
def _dev_args(b, edge):
    from common import batch_args
    return [a.to(DEV) if torch.is_tensor(a) else a for a in batch_args(b, edge)]


def _names(plan):
    return [n for _, _, n in plan.calls]


def test_loss_and_term_vs_reference(edge_of):
    """DenseNet2D (baseline_edge) with selfCorr = True in eval() and train() against the reference's returned loss and printed term
    (rtol 1e-3, the bound of test_gpu_nets for the loss); with selfCorr = False the loss of the existing fixture, and launch lists
    without a selfcorr entry that are one launch shorter."""
    from common import ESF_CASES, esf_module, gold
    g = np.load(GOLD)
    cfg, variant, kw = ESF_CASES["esf_edge_b2"]
    b, edge = edge_of(**dict(kw))
    args = _dev_args(b, edge)
    m = esf_module(cfg, variant).to(DEV)
    m.selfCorr = True
    m.eval()
    with torch.no_grad():
        loss = m(*args)[3]
    term = m.selfcorr_term()
    on_eval = _names(m._last_plan)
    print("eval: loss %.6f (reference %.6f), term %.6f (reference %.6f)" % (loss.item(), g["b_eval_loss"][0], term.item(), g["b_eval_term"]))
    np.testing.assert_allclose(loss.cpu().numpy(), g["b_eval_loss"], rtol=1e-3)
    np.testing.assert_allclose(term.item(), float(g["b_eval_term"]), rtol=1e-3)
    m.train()
    loss = m(*args)[3]
    term = m.selfcorr_term()
    on_train, on_bw = _names(m._last_plan), _names(m._last_plan.bw)
    print("train: loss %.6f (reference %.6f), term %.6f (reference %.6f)" % (loss.item(), g["b_train_loss"][0], term.item(), g["b_train_term"]))
    np.testing.assert_allclose(loss.detach().cpu().numpy(), g["b_train_loss"], rtol=1e-3)
    np.testing.assert_allclose(term.item(), float(g["b_train_term"]), rtol=1e-3)
    assert on_eval.count("selfcorr") == 1 and on_train.count("selfcorr") == 1 and on_bw.count("selfcorr.bwd") == 1
    assert on_eval.index("selfcorr") == on_eval.index("loss") + 1 and on_bw.index("selfcorr.bwd") + 1 == on_bw.index("loss.bwd")

    m = esf_module(cfg, variant).to(DEV).eval()
    with torch.no_grad():
        loss = m(*args)[3]
    np.testing.assert_allclose(loss.cpu().numpy(), gold("esf_edge_b2")["loss"], rtol=1e-3)
    off_eval = _names(m._last_plan)
    m.train()
    m(*args)
    off_train, off_bw = _names(m._last_plan), _names(m._last_plan.bw)
    for off, on in ((off_eval, on_eval), (off_train, on_train), (off_bw, on_bw)):
        assert not any("selfcorr" in n for n in off) and len(off) == len(on) - 1
        assert off == [n for n in on if "selfcorr" not in n]
    with pytest.raises(RuntimeError):
        m.selfcorr_term()


def _extra(op, elPred, latent, elOut):
    """The terms test_gpu_nets.test_gradients_through_the_outputs_vs_oracle puts on the outputs."""
    return (0.1 * op.square().mean() + 3.0 * (elPred * torch.linspace(-1, 1, 10, device=op.device)).sum(1).abs().mean()
            + 0.5 * latent.square().mean() + 2.0 * elOut.tanh().sum(1).mean())


def _oracle_grads(sd, b, edge, extra=False, selfcorr=True):
    """(objective, {name: gradient}) of the oracle's autograd of loss [+ 10 * term] [+ terms on the outputs] on the CPU."""
    from common import batch_args, setting
    from oracle import esfnet as oesf
    sdg = {k: v.clone().requires_grad_(v.dtype.is_floating_point and "running" not in k) for k, v in sd.items()}
    ref = oesf.esf_forward(sdg, setting("baseline_edge"), *batch_args(b, edge.cpu()), training=True)
    lref = ref[3].sum()
    if selfcorr:
        lref = lref + S.WEIGHT * S.term(ref[0], ref[1], 1 - b["cond"][:, 1].float())
    if extra:
        lref = lref + _extra(ref[0], ref[1], ref[2], ref[4])
    lref.backward()
    assert all(torch.isfinite(v.grad).all() for v in sdg.values() if v.grad is not None)
    return lref.item(), {k: v.grad for k, v in sdg.items() if v.grad is not None}


@pytest.fixture(scope="module")
def oracle_grads(edge_of):
    """The oracle's autograd of loss + 10 * term, and of the same plus terms on the outputs: computed once, shared, never modified."""
    from common import esf_module
    b, edge = edge_of(B=2, seed=77)
    sd = {k: v.clone() for k, v in esf_module("baseline_edge", seed=5).state_dict().items()}
    return sd, b, edge, {extra: _oracle_grads(sd, b, edge, extra) for extra in (False, True)}


def _step(sd, b, edge, storage, extra=False, selfcorr=True):
    """One training forward + backward on the HIP path: (objective, parameters, plan)."""
    from common import esf_module
    m = esf_module("baseline_edge").to(DEV)
    m.load_state_dict(sd)
    m = m.to(storage)
    m.selfCorr = selfcorr
    m.train()
    op, elPred, latent, loss, elOut = m(*_dev_args(b, edge))
    lhip = loss.sum() + (_extra(op, elPred, latent, elOut) if extra else 0.0)
    lhip.backward()
    torch.cuda.synchronize()
    params = dict(m.named_parameters())
    assert all(torch.isfinite(p.grad).all() for p in params.values() if p.grad is not None)
    return lhip.item(), params, m._last_plan


def _norm_rel(params, gref):
    names = sorted(gref)
    ref = np.array([gref[n].double().norm().item() for n in names])
    got = np.array([params[n].grad.double().norm().item() for n in names])
    return np.abs(got - ref) / np.maximum(ref, 1e-6 * ref.max())


@pytest.mark.parametrize("case", ["loss", "loss_and_outputs"])
def test_parameter_gradients_vs_oracle(oracle_grads, case):
    """loss.backward() with selfCorr = True against the oracle's autograd of esf_forward(...)[3] + 10 * selfcorr_refs.term(op, elPred,
    1 - cond[:, 1]): the counts and bounds of test_gradients_through_the_outputs_vs_oracle; once with that test's terms on the
    outputs added (the caller's upstream gradients and the term's must add in the plan's buffers)."""
    sd, b, edge, refs = oracle_grads
    extra = case == "loss_and_outputs"
    lref, gref = refs[extra]
    lhip, params, pl = _step(sd, b, edge, torch.float32, extra)
    assert all(t.abs().max().item() == 0.0 for t in pl.up_grads), "the plan's upstream buffers are cleared after the run"
    lerr = abs(lhip - lref) / abs(lref)
    assert lerr < 1e-3, "objective differs by %.2e" % lerr
    scale = max(v.norm().item() for v in gref.values())
    worst, n, num, den = 0.0, 0, 0.0, 0.0
    for name, p in params.items():
        if name not in gref:
            continue
        r, g = gref[name].double(), p.grad.double().cpu()
        num, den = num + (r - g).square().sum().item(), den + r.square().sum().item()
        if r.norm().item() < 1e-4 * scale:
            continue
        n += 1
        worst = max(worst, (r - g).norm().item() / r.norm().item())
    whole = (num / den) ** 0.5
    print("%s: %d tensors, worst per-tensor relative L2 %.2e, whole gradient %.2e" % (case, n, worst, whole))
    assert n > 50 and worst < 3e-2 and whole < 1e-2


@pytest.fixture(scope="module")
def exact_edge_b2(bdcn):
    """Batch and edge map of the esf_edge_b2 case from the exact-fp32 BDCN kernels (as test_gpu_nets.edge_of_exact: split-f16 trunk off)."""
    import types
    from common import ESF_CASES, bdcn_module
    from egne_amd import engine, synth
    from egne_amd.utils import calc_edge
    kw = dict(ESF_CASES["esf_edge_b2"][2])
    b = synth.make_batch(kw.pop("B"), **kw)
    old = engine.F16X3_ENABLED
    engine.F16X3_ENABLED = False
    try:
        net = bdcn_module().to(DEV)
        edge = calc_edge(types.SimpleNamespace(prec=torch.float32, edge_thres=0), b["img"].to(DEV), net, DEV)
    finally:
        engine.F16X3_ENABLED = old
    return b, edge


def test_parameter_gradients_bf16_storage_vs_oracle(exact_edge_b2):
    """The same with bf16 activation storage, at the limits tests/test_gpu_bf16.py states for a whole network's gradients
    (test_esf_train_step_bf16_storage_vs_reference: loss 1e-2; per-parameter gradient norms, median 3e-2 and 90th percentile 1.5e-1)
    and in the setting it states them for: the batch and seeded weights of its esf_edge_b2 case, edge maps from the exact-fp32
    kernels."""
    from common import esf_module
    b, edge = exact_edge_b2
    sd = {k: v.clone() for k, v in esf_module("baseline_edge").state_dict().items()}
    lref, gref = _oracle_grads(sd, b, edge)
    lhip, params, pl = _step(sd, b, edge, torch.bfloat16)
    assert pl.bf16 and "selfcorr.bwd" in _names(pl.bw)
    lerr = abs(lhip - lref) / abs(lref)
    rel = _norm_rel(params, gref)
    print("bf16 storage: loss rel %.2e, grad-norm rel median %.2e p90 %.2e" % (lerr, np.median(rel), np.sort(rel)[int(0.9 * len(rel))]))
    assert lerr < 1e-2
    assert np.median(rel) < 3e-2 and np.sort(rel)[int(0.9 * len(rel))] < 1.5e-1


def test_ritnet_v1_loss_and_gradient_norms_vs_oracle():
    """The comparator with selfCorr = True (the reference adds the term there too, models/RITnet_v1.py:286-287): fp32 storage, loss
    (rtol 1e-3) and the gradient-norm check of test_ritnet_v1_train_step_vs_reference (1e-2) against the oracle with the term added."""
    from common import batch_args
    from egne_amd import synth
    from oracle import ritnet_v1 as ov1
    m = _v1_model()
    sd = {k: v.detach().cpu().clone() for k, v in m.state_dict().items()}
    b = synth.make_batch(2, seed=1234)
    sdg = {k: v.clone().requires_grad_(v.dtype.is_floating_point and "running" not in k) for k, v in sd.items()}
    ref = ov1.ritnet_v1_forward(sdg, *batch_args(b, torch.zeros_like(b["img"])), training=True)
    lref = ref[3].sum() + S.WEIGHT * S.term(ref[0], ref[1], 1 - b["cond"][:, 1].float())
    lref.backward()
    m.selfCorr = True
    m.train()
    loss = m(*_v1_args())[3]
    np.testing.assert_allclose(loss.item(), lref.item(), rtol=1e-3)
    assert "selfcorr" in _names(m._last_plan)
    loss.sum().backward()
    torch.cuda.synchronize()
    params = dict(m.named_parameters())
    names = [k for k, v in sdg.items() if v.grad is not None]
    refn = np.array([sdg[k].grad.double().norm().item() for k in names])
    got = np.array([params[k].grad.double().norm().item() for k in names])
    rel = np.abs(got - refn) / np.maximum(refn, 1e-6 * refn.max())
    print("ritnet_v1 + selfCorr: loss %.5f (oracle %.5f), grad-norm rel median %.2e max %.2e (%s)"
          % (loss.item(), lref.item(), np.median(rel), rel.max(), names[int(np.argmax(rel))]))
    assert len(names) > 50 and rel.max() < 1e-2


def test_flipping_selfcorr_builds_a_second_plan(edge_of):
    """The plan cache key holds bool(selfCorr): off -> on -> off gives base, base + 10 * term, base again.  out_terms[0] takes one fp32
    addition of weight * term (itself one fp32 product), so the difference is 10 * term within an ulp of the larger loss."""
    from common import ESF_CASES, esf_module
    cfg, variant, kw = ESF_CASES["esf_edge_b2"]
    b, edge = edge_of(**dict(kw))
    args = _dev_args(b, edge)
    m = esf_module(cfg, variant).to(DEV).eval()
    with torch.no_grad():
        for flag in (False, True):          # each plan's first run calibrates its f16 pre-scales: measure from the second on
            m.selfCorr = flag
            m(*args)
        m.selfCorr = False
        l0 = m(*args)[3].item()
        m.selfCorr = True
        l1 = m(*args)[3].item()
        term = m.selfcorr_term().item()
        m.selfCorr = False
        l2 = m(*args)[3].item()
    assert len(m._plans) == 2
    assert l2 == l0
    assert term > 0 and abs((l1 - l0) - 10.0 * term) <= 2.0 ** -23 * abs(l1), (l0, l1, term)


def test_train_py_with_selfcorr(tmp_path, monkeypatch, capsys):
    """train.py --selfCorr 1 runs an epoch with finite losses (before the term existed the first step raised NotImplementedError)."""
    monkeypatch.chdir(tmp_path)
    from egne_amd import train as TR
    m = TR.main(["--synthetic", "8", "--batchsize", "4", "--selfCorr", "1", "--epochs", "1", "--setting", "configs/baseline_edge.yaml",
                 "--expname", "sc", "--pipeline", "0"])      # (back to back: the loop then logs the first batch's own loss)
    assert m.selfCorr is True and "selfcorr" in _names(m._last_plan)
    out = capsys.readouterr().out
    vals = [float(v) for v in re.findall(r"Loss: ([-+.\w]+)", out) + re.findall(r"valid loss ([-+.\w]+)", out)]
    assert len(vals) >= 2 and all(math.isfinite(v) for v in vals), out
    assert math.isfinite(m.selfcorr_term().item())
    bad = [k for k, v in m.state_dict().items() if v.dtype.is_floating_point and not torch.isfinite(v).all()]
    assert not bad, bad[:5]
