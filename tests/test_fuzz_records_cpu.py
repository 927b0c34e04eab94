"""The record-mode fuzz (tests/fuzz_records.py) without a GPU: draw and expected over the schedule tests/test_gpu_fuzz_records.py
commits, with the models alone.  Four things are asserted: the generator is deterministic; the schedule COVERS what it was chosen for
(every branch below at least three times -- a branch that is never drawn is a branch that is never tested); the models agree with
their naive restatements on the new input classes; and the wide cases are not vacuous.  Wide case (b)'s and (c)'s tiling is the GPU
test's.  Indels mode is one of the modes: its branches are in BRANCHES, its comparison in test_the_comparison_can_fail.

Measured here (CPU): TIMING below."""
import collections

import numpy as np
import pytest

from tests import fuzz_records as fz
from tests.align_model import oriented_codes
from tests.extend_model import naive_extension
from tests.placement_model import masked_mates
from tests.splice_model import expected_alignments_spliced, naive_candidates
from tests.spliced_model import expected_spliced_depth
from tests.test_gpu_fuzz_records import SCHEDULE, WIDE_A_SEED, WIDE_B_SEED, WIDE_C_SEED

# TIMING: the whole file takes about 60 s on the CPU it was written on (52 s before indels mode and the `indel` bias, in the same session):
# the schedule's 102 cases 40 s (among them one batch of 1 520 pairs tied over six genes, 10 s), wide case (a)'s 8 257 pairs and the blocks
# and remainders of wide cases (b) and (c) 13 s, the naive restatements 5 s

AT_LEAST = 3
# every branch the schedule must reach AT_LEAST times (a counter of events, or of cases where the thing is a property of the case)
BRANCHES = (
    ["align." + s for s in ("trimmed", "closed", "open_insertion", "dropped", "closed_r64", "open_r65")]
    + ["ext." + s for s in ("left", "right", "bonus_decided")]
    + ["splice." + s for s in ("left_placed", "right_placed", "left_shortened", "any_ambiguous", "any_too_costly", "any_no_candidate", "range_over_64")]
    + ["rescue.state%d" % s for s in range(6)] + ["pairs.cls%d" % s for s in range(6)] + ["n_blocks.%d" % b for b in (1, 2, 3, 4)]
    + ["strand.0", "strand.1", "tie.2", "tie.over_inline", "single_end", "masked", "pileup.other_floor", "variant_site"]
    + ["class." + c for c in fz.CLASSES]
    + ["inst.%d%d%d.stored" % (e, a, s) for e in (0, 1) for a in (0, 1) for s in (0, 1)]
    + ["inst.%d1%d.unstored" % (e, s) for e in (0, 1) for s in (0, 1)]
    + ["seg_m.%d" % m for m in (1, 2, 3, 4)] + ["family." + f for f in fz.FAMILIES] + ["k.%d" % k for k in fz.KS]
    + ["indels." + s for s in fz.INDEL_COUNTERS]
    + ["indels." + s for s in ("fwd", "rev", "shift_ge_1", "shift_over_len", "floor_same", "floor_other", "without_alignments", "third_launch", "tied",
                               "single_end", "masked", "gap_eq_min_intron", "intron_as_deletion", "before_rescue", "with_length_repair")]
)
# reached once by design, not three times, and why
ONCE = {
    "repair.overflow": "a batch whose associations overflow the slot's first reservation needs more than 1 481 reads tied over six genes: "
                       "18 000 mate records through every model, 8 s of this file and 3 s of the GPU file per case",
    "repair.length.submit_device": "(at least once; the resident family behind a bound that does not hold -- in fact drawn more often)",
    "indels.with_overflow": "repair.overflow's reason: the one overflow batch, which therefore always has indels mode on",
    "indels.with_length_repair.submit_device": "(at least once: what tests/test_gpu_fuzz_records.py's last test asks of the device)",
}


@pytest.fixture(scope="module")
def schedule(oracle):
    """[(case, expected)] over the schedule, computed once"""
    out = []
    for bias, seed0, count in SCHEDULE:
        for seed in range(seed0, seed0 + count):
            case = fz.draw(seed, bias)
            out.append((case, fz.expected(case, oracle)))
    return out


def same_case(a, b):
    for key in a:
        if key == "batch":
            for part in a["batch"]:
                x, y = a["batch"][part], b["batch"][part]
                assert (x is None and y is None) or (x.dtype == y.dtype and x.tobytes() == y.tobytes()), part
        elif key == "records":
            assert [bytes(r) for r in a["records"]] == [bytes(r) for r in b["records"]]
        else:
            assert a[key] == b[key], key


def test_draw_is_deterministic():
    for bias, seed0, count in SCHEDULE:
        for seed in (seed0, seed0 + count - 1):
            same_case(fz.draw(seed, bias), fz.draw(seed, bias))
    a, b = fz.draw_wide_depth(WIDE_B_SEED), fz.draw_wide_depth(WIDE_B_SEED)
    c, d = fz.draw_wide_indels(WIDE_C_SEED), fz.draw_wide_indels(WIDE_C_SEED)
    for a, b in ((a, b), (c, d)):
        for part in ("block", "rest"):
            assert all((a[part][x] is None and b[part][x] is None) or a[part][x].tobytes() == b[part][x].tobytes() for x in a[part])
    # and another seed or another bias is another case
    assert fz.draw(SCHEDULE[0][1], "")["batch"]["seq1"].tobytes() != fz.draw(SCHEDULE[0][1] + 1, "")["batch"]["seq1"].tobytes()
    assert fz.draw(SCHEDULE[0][1], "")["batch"]["seq1"].tobytes() != fz.draw(SCHEDULE[0][1], "rescue")["batch"]["seq1"].tobytes()


def test_the_schedule_covers_every_branch(schedule):
    total = collections.Counter()
    for case, want in schedule:
        for key, v in want["coverage"].items():
            if isinstance(v, (int, np.integer)) and not isinstance(v, bool) and key not in ("widest", "indels.largest_shift"):
                total[key] += int(v)
    print("coverage over %d cases: %s" % (len(schedule), dict(sorted(total.items()))))
    print("indels mode on in %d cases; the largest left shift of a tabled event: %d bases" % (
        sum(1 for case, _ in schedule if case["modes"]["indels"]), max(want["coverage"].get("indels.largest_shift", 0) for _, want in schedule)))
    missing = {b: total[b] for b in BRANCHES if total[b] < AT_LEAST}
    assert not missing, "drawn fewer than %d times: %s" % (AT_LEAST, missing)
    for b in ONCE:
        assert total[b] >= 1, b
    assert max(want["coverage"]["widest"] for _, want in schedule) > fz.SHK_INLINE_IDS
    # the hostile mates reach what random reads never do: rescue_kernel's placing path, from several cases
    assert sum(1 for _, want in schedule if want["coverage"].get("rescue.state4", 0) + want["coverage"].get("rescue.state5", 0)) >= AT_LEAST


def test_the_models_agree_with_their_naive_restatements(schedule, oracle):
    """on the drawn cases, whose input classes the models' authors did not have: step 3b's ranged candidate search against the one
    that tries every site, step 3a's scorer against the one that prices every e from scratch, the aligned pileup's total against the
    base-bearing block bases counted from the records, the owned pileup's channel sums (plus the owned bytes that are no base) against
    spliced depth at the same floor; indels mode's two redundancies: deletions + insertions is the table's total of fwd + rev, and mates
    is the number of records with a block at the mode's floor"""
    n_spliced = n_extended = n_aligned = n_owned = n_indels = 0
    for case, want in schedule:
        md, batch, q = case["modes"], case["batch"], case["min_quality"]
        sm, rows4, goff, gids = want["model"], want["rows4"], want["goff"], want["gids"]
        if md["indels"]:
            table, stats = want["indels"]
            assert stats["deletions"] + stats["insertions"] == int(table["fwd"].sum(dtype=np.uint64) + table["rev"].sum(dtype=np.uint64)), fz.describe(case)
            # (the overflow batch is primed: its first reads went through every slot of the context once before it)
            primed = fz.capi.SHK_PIPE_DEPTH * int((want["indel_records"][:int(want["primer"]["goff"][-1])]["n_blocks"] >= 1).sum()) if "primer" in want else 0
            assert stats["mates"] == case["times"] * int((want["indel_records"]["n_blocks"] >= 1).sum()) + primed and stats["dropped"] == 0, fz.describe(case)
            n_indels += stats["deletions"] + stats["insertions"] > 0
        if case["n"] > 400:
            continue                                             # (the overflow batch: its content is 300-pair cases' many times over)
        if md["al_floor"] and (md["splice"] or md["ext"][0]):
            P, B = md["ext"]
            again = expected_alignments_spliced(sm, batch, goff, gids, rows4, md["al_floor"], case["sites"] if md["splice"] else [], md["splice"] or (0, 0, 0),
                                                P, B, q, None, naive_candidates, naive_extension)
            assert again.tobytes() == want["before_rescue"].tobytes(), fz.describe(case)
            n_spliced += bool(md["splice"])
            n_extended += bool(P)
        if md["pileup"][0] == "aligned":
            recs = want["pileup_records"]
            bearing = 0
            for i, pair in enumerate(masked_mates(batch, q)):
                for j in range(int(goff[i]), int(goff[i + 1])):
                    for t, mate in enumerate(pair):
                        r = recs[j, t]
                        if mate is not None and int(r["n_blocks"]):
                            codes = oriented_codes(mate, int(r["strand"]))
                            bearing += sum(int((codes[int(b[1]):int(b[1]) + int(b[2])] < 4).sum()) for b in r["block"][:int(r["n_blocks"])])
            assert int(want["pileup"][0].astype(np.uint64).sum()) == bearing * case["times"] == want["bearing"], fz.describe(case)
            n_aligned += 1
        else:
            depth, mates = expected_spliced_depth(sm, batch, goff, gids, rows4, md["pileup"][1])
            total = want["pileup"][0].sum(axis=1, dtype=np.uint64) + np.uint64(case["times"]) * want["pileup_lost"]
            assert np.array_equal(total, np.uint64(case["times"]) * depth) and want["pileup"][1] == case["times"] * mates, fz.describe(case)
            n_owned += 1
    assert min(n_spliced, n_extended, n_aligned, n_owned, n_indels) >= 10, (n_spliced, n_extended, n_aligned, n_owned, n_indels)


def test_the_wide_cases_are_not_vacuous(oracle):
    case = fz.draw(WIDE_A_SEED, "wide")
    assert case["n"] == fz.WIDE_A_PAIRS == 8257 and case["paired"] and case["modes"]["seg_m"] == 4 and case["modes"]["pileup"][0] == "owned"
    assert case["modes"]["ext"][0] and case["modes"]["splice"] and case["longest"] <= 100
    want = fz.expected(case, oracle)
    goff = want["goff"]
    second_trip = want["alignments"][int(goff[fz.PL_MAX_BLOCKS * fz.PL_WAVES]):]
    assert int((second_trip["n_blocks"] >= 2).any(axis=1).sum()) >= 50
    cov = want["coverage"]
    assert cov["splice.left_placed"] > 100 and cov["splice.right_placed"] > 100 and cov["ext.left"] > 100
    first = {bytes(m) for pair in list(masked_mates(case["batch"], 0))[:8192] for m in pair}
    # every read of the second trip holds mates that no read of the first trip holds
    assert all(pair[0] not in first and pair[1] not in first for pair in list(masked_mates(case["batch"], 0))[8192:])
    # the single-end variant is another batch: mate 2 is gone
    single = fz.variant(case, pileup=("aligned", case["modes"]["al_floor"]), single_end=True)
    assert single["batch"]["seq2"] is None and not single["paired"] and case["batch"]["seq2"] is not None
    # (b): the second trip lies wholly in the remainder, and its reads cover bases the block does not
    b = fz.draw_wide_depth(WIDE_B_SEED)
    assert len(b["block"]["off1"]) - 1 == 1021 and len(b["rest"]["off1"]) - 1 == 836 and 513 * 1021 <= fz.DEPTH_LANES < fz.WIDE_B_PAIRS
    wb = fz.expected_wide_depth(b, oracle)
    assert wb["rest_only"] > 50 and wb["rest_only_spliced"] > 50
    assert len(wb["goff"]) == fz.WIDE_B_PAIRS + 1 and int(wb["plain"][1]) > fz.DEPTH_LANES
    assert len(wb["junctions"]) >= 3 and max(r[4] for r in wb["junctions"]) > 513
    # (a) has indels mode on at alignments mode's floor, so its single-end variant runs indel_kernel without a second mate at 8 257 reads
    assert case["modes"]["indels"] and case["modes"]["indels"][0] == case["modes"]["al_floor"] and single["modes"]["indels"] == case["modes"]["indels"]
    assert want["indels"][1]["deletions"] > 100 and cov["indels.fwd"] > 50 and cov["indels.rev"] > 50
    # (c): the same shape; what the second trip's 321 pairs show, from the models alone -- conditions on the input
    c = fz.draw_wide_indels(WIDE_C_SEED)
    assert len(c["block"]["off1"]) - 1 == 1021 and len(c["rest"]["off1"]) - 1 == 836
    wc = fz.expected_wide_indels(c, oracle)
    table, stats = wc["tail"]
    print("wide case (c): the second trip's pairs show %s, %d keys, %d of them nowhere else; the whole batch %d keys, %s" % (
        stats, len(table), len(wc["tail_only"]), len(wc["indels"][0]), wc["indels"][1]))
    assert stats["deletions"] + stats["insertions"] >= 30 and len(wc["tail_only"]) >= 10
    assert sum(f for f, r in table.values()) > 0 and sum(r for f, r in table.values()) > 0
    assert stats["insertions"] >= 1 and stats["deletions"] >= 1
    assert len(wc["goff"]) == fz.WIDE_B_PAIRS + 1 and wc["indels"][1]["mates"] > fz.DEPTH_LANES and wc["indels"][1]["dropped"] == 0


def test_the_comparison_can_fail(schedule):
    """the device's part played by the model's own records with one byte flipped, kind by kind: each is reported under its name with
    the record it lies in, and the untouched records pass"""
    case, want = next((c, w) for c, w in schedule if c["modes"]["rescue"] and c["paired"] and c["modes"]["cand_m"] and int(w["goff"][-1]) > 20)
    kinds = {"evidence": want["evidence"], "candidate reads": want["candidates"][0], "candidate entries": want["candidates"][1],
             "placement": want["placement"], "segment keys": want["segments"][0], "segment entries": want["segments"][1],
             "alignments": want["alignments"], "rescue": want["rescue"], "pairs": want["pairs"]}
    goff, gids = want["goff"].astype(np.uint32), want["gids"].astype(np.uint16)
    assert fz.compare_records(kinds, want, goff, gids) is None
    for kind, a in kinds.items():
        bad = np.array(a, copy=True)
        bad.reshape(len(bad), -1).view(np.uint8)[len(bad) - 1, 0] ^= 1
        said = fz.compare_records(dict(kinds, **{kind: bad}), want, goff, gids)
        assert said and said.startswith(kind + ": record %d:" % (len(bad) - 1)), (kind, said)
    g2 = gids.copy()
    g2[3] ^= 1
    assert fz.compare_records(kinds, want, goff, g2).startswith("gene_ids: record 3")
    # indels mode's state: one count of one entry, one counter
    case, want = next((c, w) for c, w in schedule if c["modes"]["indels"] and len(w["indels"][0]) > 5)
    table, stats = want["indels"]
    assert fz.compare_indels(table.copy(), dict(stats), want["indels"]) is None
    for field in ("fwd", "rev", "x"):
        bad = table.copy()
        bad[field][len(bad) - 2] += 1
        said = fz.compare_indels(bad, dict(stats), want["indels"])
        assert said and said.startswith("indel table: record %d:" % (len(bad) - 2)), (field, said)
    assert fz.compare_indels(table[:-1], dict(stats), want["indels"]).startswith("indel table: dtype / shape")
    for name in stats:
        said = fz.compare_indels(table.copy(), dict(stats, **{name: stats[name] + 1}), want["indels"])
        assert said and said.startswith("indel counter %s:" % name), (name, said)
