"""What makes the bars of the GEMM family's GPU parity test legitimate, and what shows that they bite: on the CPU, from the restatement
alone.  For every run of tests/gemm_cases.py the fp32 restatement (ref_lo) is held against the fp64 one (ref_hi) by the rule the device
is held to (tests/grad_parity.py over the tiles a workgroup owns): every slice is known to a quarter of its bar or better, nothing lies
in between, no slice is zero but the named ones.  A run whose reference cannot meet this is changed in the table, not loosened here.

Then the stand-ins.  The split arithmetic modelled on the host (six bf16 x bf16 part products per k-block of 16 onto an fp32
accumulator) passes every fp32 run with K <= 512; the same with the sixth part product (a2 b0) left out sits 2.3e-6 .. 2.5e-6 from fp64
-- inside the former 2e-5 of the largest entry, and inside test_gpu_split.py's 3e-6 -- and fails every one of them.  So do one row of an
edge tile that holds its neighbour's values and one k-block of 16 missing from one tile."""
import pytest
import torch

from tests import gemm_cases as GC

# fp32 storage, no activation, K <= 512: where the tight bar is the point
TIGHT = [r["id"] for r in GC.RUNS if all(GC.rule_of(p) == "f32" and not p["bf16"] and p["K"] + p["K1"] <= 512 for p in r["probs"])]
BF16_OUT = [r["id"] for r in GC.RUNS if any(p["bf16out"] for p in r["probs"])]


def _lo(r):
    return [GC.reference(r, i, torch.float32) for i in range(len(r["probs"]))]


@pytest.mark.parametrize("rid", GC.IDS)
def test_reference_knows_every_slice(rid):
    r = GC.by_id(rid)
    res, _ = GC.judge(r, _lo(r), what=rid + ", fp32 restatement as the device")
    for i in range(len(r["probs"])):
        for t in GC.reference(r, i).values():
            assert t.dtype == torch.float64
    assert not res.between and not res.nosignal
    assert set(res.zero) == {z for i in range(len(r["probs"])) for z in GC.zero_slices(r, i)}
    for k, e in res.e_ref.items():
        assert e <= res.bars[k] / 4, (k, e, res.bars[k])
    print("gemm parity %s: %d slices, e_ref worst %.3g" % (rid, len(res), max(res.e_ref.values())))


def test_the_table_holds_the_tight_runs():
    """the stand-in tests below run over something: every fp32 entry point has runs with the tight bar"""
    assert len(TIGHT) >= 60
    assert {GC.by_id(i)["entry"] for i in TIGHT} == {"f32", "group", "p3", "rows", "dx"}


@pytest.mark.parametrize("rid", TIGHT)
def test_six_part_products_pass_and_five_fail(rid):
    r = GC.by_id(rid)
    n = len(r["probs"])
    six = [GC.standin(r, i) for i in range(n)]
    res, _ = GC.judge(r, six, what=rid + ", six part products")
    five = [GC.standin(r, i, parts=GC.SIX[:5]) for i in range(n)]
    with pytest.raises(AssertionError, match="own-norm gradient error"):
        GC.judge(r, five, what=rid + ", without a2 b0")


def _edge_tile(r):
    """(problem, tile row, tile column) of the last tile of the largest problem -- the ragged one where the shape has one; of the last
    tile row with a valid row where frame_dx zeroes the rows behind a sample's length"""
    i = max(range(len(r["probs"])), key=lambda j: r["probs"][j]["M"] * r["probs"][j]["N"])
    p = r["probs"][i]
    bm, bn = r["tile"]
    valid = torch.nonzero(~GC.zero_rows(p))
    return i, int(valid[-1]) // bm, (p["N"] - 1) // bn


@pytest.mark.parametrize("rid", [i for i in TIGHT if not GC.by_id(i)["probs"][0]["fold"] and max(p["M"] for p in GC.by_id(i)["probs"]) > 1])
def test_a_neighbour_row_in_an_edge_tile_fails(rid):
    r = GC.by_id(rid)
    i, ta, tb = _edge_tile(r)
    tb = 0          # (the first tile column: the last may be one column wide, and a c_mask_y may zero that element in both rows)
    got = [GC.standin(r, j, swap_row=(ta, tb) if j == i else None) for j in range(len(r["probs"]))]
    with pytest.raises(AssertionError, match=r"C\[%d,%d\]: own-norm gradient error" % (ta, tb)):
        GC.judge(r, got, what=rid + ", one row from its neighbour")


@pytest.mark.parametrize("rid", [i for i in TIGHT if not GC.by_id(i)["probs"][0]["fold"]])
def test_a_missing_k_block_in_one_tile_fails(rid):
    r = GC.by_id(rid)
    i, ta, tb = _edge_tile(r)
    p = r["probs"][i]
    last = (p["K"] + p["K1"] - 1) // 16
    got = [GC.standin(r, j, skip_block=(ta, tb, last) if j == i else None) for j in range(len(r["probs"]))]
    with pytest.raises(AssertionError, match=r"C\[%d,%d\]: own-norm gradient error" % (ta, tb)):
        GC.judge(r, got, what=rid + ", one k-block left out")


_BF16_SEEN = []


@pytest.mark.parametrize("rid", BF16_OUT)
def test_bf16_rounded_references(rid):
    """bf16 outputs: both restatements start from the same bf16 operands and end in a bf16 rounding; the rounded fp32 restatement
    against the rounded fp64 one per slice.  The worst slice over all runs is what tests/gemm_cases.BF16_E_REF records."""
    r = GC.by_id(rid)
    res, _ = GC.judge(r, _lo(r), what=rid + ", rounded restatements")
    for i, p in enumerate(r["probs"]):
        I, hi, lo = GC.operands(r, i), GC.reference(r, i)["C"], GC.reference(r, i, torch.float32)["C"]
        assert torch.equal(I["Ae"], I["Ae"].bfloat16().float()) and torch.equal(I["Be"], I["Be"].bfloat16().float())
        assert torch.equal(hi, hi.bfloat16().double()) and torch.equal(lo, lo.bfloat16().float())
    e = max(res.e_ref.values())
    print("gemm parity bf16 output %s: rounded e_ref worst slice %.3g" % (rid, e))
    _BF16_SEEN.append(e)
    assert e <= GC.BF16_E_REF and not res.between
    if len(_BF16_SEEN) == len(BF16_OUT):
        assert GC.BF16_E_REF <= 1.5 * max(_BF16_SEEN), "BF16_E_REF is not the measured one: worst %.3g" % max(_BF16_SEEN)
