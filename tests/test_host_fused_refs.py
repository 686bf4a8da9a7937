"""tests/fused_refs.py on the CPU: (1) the table reaches every one of the 34 instantiations the fused launchers can choose and holds the
maps, slices and epilogues it is meant to; (2) for every row and each of its four exact generators, under the scales the plan will use,
the conditions that make the run exact hold (fused_refs.conditions) and the float64 emulation of the two split-f16 stages equals the
reference bit for bit; (3) the data tells right from wrong: each of the seven mistakes of fused_refs.wrong changes at least one stored
output of every row it applies to, and more than 1 % of them in the rows named for it.  (3) stands in for any fault injection on the
GPU: it shows what tests/test_gpu_fused_pair_sweep.py would see if the kernel did that."""
import pytest
import torch
import torch.nn.functional as F

import fused_refs as R

D = torch.float64
ROW_RUNS = [(r, k) for r in R.FUSED_SWEEP for k in R.RUNS]
ROW_RUN_IDS = ["%s-%s" % (r["id"], k) for r, k in ROW_RUNS]
ROW_MISTAKES = [(r, m) for m in R.MISTAKES for r in R.FUSED_SWEEP if R.applies(r, m)]
ROW_MISTAKE_IDS = ["%s-%s" % (m, r["id"]) for r, m in ROW_MISTAKES]


def test_required_lists_the_34_instantiations_and_every_one_has_a_row():
    assert len(R.REQUIRED) == 34
    have = {r["form"] for r in R.FUSED_SWEEP}
    missing = sorted(R.REQUIRED - have)
    assert not missing, "no row reaches %s" % missing
    assert have <= R.REQUIRED
    for r in R.FUSED_SWEEP:
        assert R.fused_form(r) == r["form"], (r["id"], R.fused_form(r))
    assert len(set(R.FUSED_IDS)) == len(R.FUSED_IDS)


def test_the_launch_rule_on_shapes_production_uses():
    """ESF-Net's dense blocks (G = 4 / 6 / 8 and 7 / 11 in one buffer), an up block with the folded addend, the convBlock head."""
    f = R.form
    assert R.launch_form(4, True, 32, 32, False) == f(1, 1, 8, 1, "UNI", "GL4") == (1, 1, 8, 1, False, False, True, 4, False)
    assert R.launch_form(8, True, 32, 32, False) == f(1, 1, 8, 2, "UNI", "GL4") and R.launch_form(7, True, 32, 32, False) == f(1, 1, 8, 2, "UNI")
    assert R.launch_form(7, True, 64, 64, False) == f(2, 2, 4, 4, "UNI", "GL1") and R.launch_form(11, True, 64, 64, False) == f(2, 2, 4, 6, "UNI", "GL1")
    assert R.launch_form(7, True, 64, 32, False) == f(2, 1, 4, 4) and R.launch_form(12, False, 64, 64, False) == f(2, 2, 4, 6)
    assert R.launch_form(6, True, 32, 32, True) == f(1, 1, 8, 2, "UPADD", "UNI", "GL2") and R.launch_form(8, True, 32, 32, True) == f(1, 1, 8, 2, "UPADD", "UNI")
    assert R.launch_form(0, False, 32, 32, False, c4=True, c1v=True) == (1, 1, 8, 1, True, False, False, 3, True)


def test_the_table_holds_what_it_is_meant_to():
    rows = {r["id"]: r for r in R.FUSED_SWEEP}
    tiles = {i: R.tiles_of(r)[3] for i, r in rows.items()}
    big = [i for i, n in tiles.items() if n > R.MAX_GRID]
    assert {(rows[i]["B"], rows[i]["H"], rows[i]["W"]) for i in big} == {(3, 72, 320), (2, 36, 480)} and all(tiles[i] == 270 for i in big)
    assert {rows[i]["form"][2] for i in big} == {8, 4} and any(rows[i]["up"] for i in big) and any(rows[i]["planar"] for i in big)
    for i in big:          # 256 workgroups, a multiple of 8: 14 of them walk a second tile, in runs of 32 tiles per XCD
        walks = R.tile_walk(rows[i])
        assert len(walks) == 256 and sum(len(w) == 2 for w in walks) == 14 and walks[8][0] == walks[0][0][:2] + (walks[0][0][2] + R.TW,)
    assert tiles[R.STRIDED] == 12 and all(len(w) == 1 for w in R.tile_walk(rows[R.STRIDED]))
    assert any((r["B"], r["H"], r["W"]) == (1, 3, 5) for r in rows.values())
    assert sum(r["W"] == 32 and r["H"] == r["form"][2] for r in rows.values()) >= 2
    assert sum(r["far"] is not None and r["form"][6] for r in rows.values()) >= 2
    assert {(r["H"], r["W"]) for r in rows.values() if r["up"]} == {(26, 34), (16, 64), (72, 320)}
    pair = [r for r in rows.values() if r["kind"] == "pair"]
    assert {24, 40} <= {c for r in pair for c in r["chans"]} and {30, 62} <= {r["C1"] for r in pair} and {30, 38} <= {r["C2"] for r in pair}
    assert any(r["form"] == R.form(2, 1, 4, 2) and r["split"] is None for r in pair), "one buffer with 32 outputs on the non-UNI build"
    for key in ("post", "residual", "stats"):
        assert sum(bool(r[key]) for r in rows.values()) >= 6
    assert {r["act"] for r in rows.values()} == {R.ACT_NONE, R.ACT_RELU, R.ACT_LEAKY}
    assert {R.stats_nchunk(r) // (R.tiles_of(r)[1] * R.tiles_of(r)[2]) for r in rows.values() if r["stats"]} == {2, 4}
    c4 = [r for r in rows.values() if r["kind"] == "c4"]
    assert sorted(r["chans"][0] for r in c4 if not r["planar"]) == [2, 3, 4] and sum(r["planar"] and not r["c1v"] for r in c4) == 1
    assert all(r["B"] * r["H"] * r["W"] % 4 == 0 for r in c4 if r["planar"]), "the planar input is measured as rows of four"
    for r in rows.values():        # two buffers must differ in pixel pitch, or UNI would depend on where the allocator puts them
        if r["split"] is not None:
            a, b = r["chans"][:r["split"]], r["chans"][r["split"]:]
            assert sum(R.pad8(c) + 8 for c in a) != sum(R.pad8(c) + 8 for c in b), r["id"]
    for m, ids in R.NAMED.items():
        assert all(R.applies(rows[i], m) for i in ids), m


def test_upsample2_is_the_interpolation_of_the_model():
    P = 16 * torch.randint(-8, 9, (2, 3, 13, 17), generator=torch.Generator().manual_seed(5)).double()
    want = F.interpolate(P, scale_factor=2, mode="bilinear", align_corners=False)
    assert torch.equal(R.upsample2(P), want) and torch.equal(want.float().double(), want)
    assert not torch.equal(R.upsample2(P, clamp=False), want) and not torch.equal(R.upsample2(P, shift=1), want)


@pytest.mark.parametrize("row,run", ROW_RUNS, ids=ROW_RUN_IDS)
def test_exact_runs_are_exact(row, run):
    """Every product and every partial sum of both stages is an fp32 value, t * a2 splits into two normal f16 halves, at most one operand
    of each product carries lo halves -- and the emulation of that arithmetic equals the float64 reference."""
    data, want, scales = R.exact_case(row, run)
    u1, u2 = R.conditions(row, run, data, want, scales)
    got = R.emulate(row, data, scales)
    assert torch.equal(got, want), "%s %s: the emulation differs in %d outputs" % (row["id"], run, int((got != want).sum()))
    print("%s %s: scales %s, densities %s, partial sums up to %.3g / %.3g units" % (row["id"], run, scales, data["density"], u1, u2))


@pytest.mark.parametrize("row,mistake", ROW_MISTAKES, ids=ROW_MISTAKE_IDS)
def test_the_data_tells_a_wrong_kernel_from_a_right_one(row, mistake):
    for run in R.MISTAKE_RUNS[mistake]:
        data, want, scales = R.exact_case(row, run)
        bad = R.wrong(row, data, scales, mistake)
        share = (bad != want).double().mean().item()
        print("%s in %s %s: %.2f %% of the outputs differ" % (mistake, row["id"], run, 100 * share))
        assert share > 0, "%s goes unnoticed in %s %s" % (mistake, row["id"], run)
        if row["id"] in R.NAMED[mistake]:
            assert share > 0.01, "%s changes only %.3f %% of %s %s" % (mistake, 100 * share, row["id"], run)
