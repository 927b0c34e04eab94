#!/usr/bin/env python3
"""(test infrastructure)  Randomised differential test of SESSIONS of one context: tests/fuzz_records.py's cases are one batch through a
fresh context each; here one context takes 5 to 7 batches of different content and size, in groups of up to SHK_PIPE_DEPTH tickets in
flight (host and resident tickets mixed, every ticket another batch), with mode switches, resets, changes of kind and the two merge
calls (shk_pileup_add, shk_indels_add) between the groups.  Every hand-out's records are compared byte for byte with its own batch's
models, and every accumulated state -- depth, the junction table, pileup and the variants read from it, fragments, the indel table and
its counters -- element for element after EVERY group, whether its mode is on at that moment or not.  No tolerances: a read's records
depend on the read, its associations and the modes alone, every accumulator is a sum over mates, the variants are a function of the
summed pileup; so a session's expected state is the sum of the per-batch models since the state's last reset, plus what was added.

The parts, as in tests/fuzz_records.py, with the comparison split from the device access:

  draw_session(seed)               the context (reference, k, -q), two site lists and the steps, from numpy alone.  A step is a batch, its
                                   entry family and bound, the slot it will lie in, the modes in force and -- for the first step of a
                                   group -- the calls made in front of it, as (method of SharkHip, arguments)
  expected_session(session, ora)   fuzz_records.expected per step (times = 1, no primer), the states folded over the steps, one snapshot
                                   per group, and a `coverage` dictionary of what the session exercised
  model_results(session, want)     what a faultless device would hand back, made from the model: tests/test_fuzz_sessions_cpu.py plants
                                   faults into it
  check_hand_out, check_states     the comparison: one hand-out against its step, one read-out of the states against its group
  run_session(session, ora, want)  the device: after each wait the records through *_last (a host batch) or the *_from_device helpers
                                   (a resident one); after each group every state.  Stops at the first mismatch

What a session is drawn to meet.  A context hands its SHK_PIPE_DEPTH slots out in turn to shk_classify, shk_classify_submit and
shk_classify_device_submit; shk_classify_device has a slot of its own behind them (slots[SHK_PIPE_DEPTH]), which the steps' `slot` says.
The record arrays of a slot are sized by the slot's capacity, not by the batch, so behind a small batch's last association they hold the
records of the slot's earlier, larger batch: every session has a slot that a batch of 1 to 65 reads reuses behind one of 200 to 700
(three hand-outs later), and one that a batch of 700 reuses behind a small one, which grows its reservation.  Sizes come from {1, 63, 64,
65, 200, 300, 700}.  A session of the `overflow` flavour (twelve records of one gene) sends a batch of 700 pairs whose associations
exceed the slot's grown reservation: the overflow repair inside a session, the arrays full of other batches' records.  Five steps are
the fewest with both reuses (five hand-outs of the turning slots), so no session has four.  Paired and single-end batches alternate
freely, inside a group too: the library does not refuse it.

Only legal calls are drawn (include/shark_hip.h; tests/test_gpu_state_messages.py has the refusals): every call is made while no ticket
is outstanding; a state changes its kind (plain / spliced depth, owned / aligned pileup, the junction table's capacity, n_bins, indels
mode's min_intron) only directly behind its reset; pairs and rescue mode are set only while alignments mode is on.

By hand on a GPU box:
    timeout -k 10 600 python tests/fuzz_sessions.py [iterations] [seed]
prints one line per session, stops at the first mismatch and prints the line that replays it (`python tests/fuzz_sessions.py 1 SEED`)
and the step."""
import copy
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

from shark_amd import capi
from tests import fuzz_records as fz
from tests import synth
from tests.indels_model import table_array
from tests.spliced_model import table_rows
from tests.variants_model import expected_summary, expected_variants

SESSION_KEY = 8                                  # default_rng([seed, 8]): a stream no case of tests/fuzz_records.py draws from
assert SESSION_KEY not in set(fz.BIAS_KEY.values()) | {fz.WIDE_B_KEY, fz.WIDE_C_KEY}
FLAVOURS = ("spliced", "indel", "tie", "overflow")          # a session's is FLAVOURS[seed % 4]
SIZES = (1, 63, 64, 65, 200, 300, 700)
SMALL, LARGE = (1, 63, 64, 65), (200, 300, 700)
OVERFLOW_TWINS = 12
# the groups of a session of 5, 6 or 7 steps: three or four groups, so that a mode can be off for one of them and on again
PATTERNS = {5: [(2, 1, 2), (1, 3, 1), (1, 2, 1, 1), (2, 1, 1, 1), (1, 1, 2, 1)],
            6: [(1, 2, 3), (3, 1, 2), (2, 1, 1, 2), (1, 2, 1, 2), (1, 1, 3, 1), (3, 1, 1, 1)],
            7: [(3, 1, 3), (1, 3, 1, 2), (2, 1, 1, 3), (3, 2, 1, 1), (2, 1, 2, 2), (1, 2, 3, 1)]}
JUNCTION_CAPACITIES = (fz.JUNCTION_CAPACITY, 2 * fz.JUNCTION_CAPACITY)
INDEL_CAPACITY = fz.JUNCTION_CAPACITY
N_BINS = (2, 64, 1024, 4096)
STATES = ("depth", "junctions", "pileup", "fragments", "indels")
STATE_KINDS = ("depth.plain", "depth.spliced", "junctions", "pileup.owned", "pileup.aligned", "fragments", "indels")


def grown(need):
    """the capacity a growable array of the library takes when it must hold `need` entries (Array::reserve)"""
    return need + need // 4 + 64


# ---------------------------------------------------------------------------
# draw_session
# ---------------------------------------------------------------------------
class Plan:
    """the modes in force while a session is drawn, the calls that lead there, and what the header's rules need to be known: which states
    hold something since their last reset (`dirty`: the kind, or True)"""

    def __init__(self, rng, md, sites, junc_cap, turn):
        self.turn = self.shape = turn
        self.rng, self.md, self.lists, self.which, self.junc_cap = rng, md, sites, "a", junc_cap
        self.calls = []
        self.dirty = {s: None for s in STATES}
        self.n_bins = md["pairs"][2]
        self.back_on = []                        # (what, value) switched off in front of the last group

    def call(self, name, *args):
        self.calls.append((name, tuple(args)))

    # ---- one setter per mode: the call and the model's modes together
    def set_depth(self, v):
        self.md["depth"] = v
        if v is None:
            self.call("depth_enable", 0)
        else:
            self.call("depth_enable" if v[0] == "plain" else "depth_enable_spliced", v[1])

    def set_junctions(self, floor):
        self.md["junc_floor"] = floor
        self.call("junctions_enable", floor, self.junc_cap)

    def set_pileup(self, v):
        self.md["pileup"] = v
        if v is None:
            self.call("pileup_enable", 0)
        else:
            self.call("pileup_enable" if v[0] == "owned" else "pileup_enable_aligned", v[1])

    def set_alignments(self, floor):
        self.md["al_floor"] = floor
        self.call("alignments_enable", floor)

    def set_pairs(self, v):
        self.md["pairs"] = v
        if v is None:
            self.call("pairs_enable", 20, 1000, 0)
        else:
            self.call("pairs_enable", *v)
            self.n_bins = v[2]

    def set_rescue(self, v):
        self.md["rescue"] = v
        self.call("rescue_enable", *(v if v else (20, 0, 8, 4)))

    def set_indels(self, v):
        self.md["indels"] = v
        if v is None:
            self.call("indels_enable", 0, 20, INDEL_CAPACITY)
        else:
            self.call("indels_enable", v[0], v[1], INDEL_CAPACITY)

    def on(self, what):
        md = self.md
        return bool({"depth": md["depth"], "junctions": md["junc_floor"], "pileup": md["pileup"], "fragments": md["al_floor"] and md["pairs"],
                     "indels": md["indels"], "alignments": md["al_floor"], "rescue": md["rescue"]}[what])

    def submitted(self):
        """a batch was submitted with the modes as they stand"""
        md = self.md
        if md["depth"]:
            self.dirty["depth"] = md["depth"][0]
        if md["junc_floor"]:
            self.dirty["junctions"] = True
        if md["pileup"]:
            self.dirty["pileup"] = md["pileup"][0]
        if md["al_floor"] and md["pairs"]:
            self.dirty["fragments"] = True
        if md["indels"]:
            self.dirty["indels"] = True


def other_floor(rng, *taken):
    left = [f for f in fz.FLOORS if f not in taken]
    return int(left[int(rng.integers(0, len(left)))])


FLOOR_SHAPES = ("shared", "pileup apart", "indels apart", "three")


def draw_floors(p):
    """alignments mode's floor, aligned pileup's and indels mode's, equal or apart: one align_kernel launch serves what shares a floor.
    The shapes come in turn -- all three at one floor, aligned pileup at another, indels mode at another, three floors -- so that launches
    split and merge on the live context"""
    rng, md = p.rng, p.md
    was = md["al_floor"]
    if not was:
        return
    p.shape += 1
    shape = FLOOR_SHAPES[p.shape % len(FLOOR_SHAPES)]
    al = int(rng.choice(fz.FLOORS)) if rng.random() < 0.3 else was
    if al != was:
        p.set_alignments(al)
    if md["pileup"] and md["pileup"][0] == "aligned":
        p.set_pileup(("aligned", other_floor(rng, al) if shape in ("pileup apart", "three") else al))
    pile = md["pileup"][1] if md["pileup"] and md["pileup"][0] == "aligned" else 0
    if md["indels"]:
        p.set_indels((other_floor(rng, al, pile) if shape in ("indels apart", "three") else al, md["indels"][1]))
    if rng.random() < 0.3 and md["depth"]:
        p.set_depth((md["depth"][0], int(rng.choice([1, 3, 8]))))
    if rng.random() < 0.3 and md["junc_floor"]:
        p.set_junctions(int(rng.choice([1, 3, 8])))
    if rng.random() < 0.3 and md["pileup"] and md["pileup"][0] == "owned":
        p.set_pileup(("owned", int(rng.choice([1, 3, 8]))))


def draw_pairs(rng, n_bins):
    return (int(rng.choice([1, 20, 30, 1000])), int(rng.choice([1, 50, 300, 611, 1000, 4096, 100000])), n_bins)


def draw_rescue(rng):
    return (int(rng.choice([1, 20, 30])), int(rng.choice([1, 90, 200, 611, 1000, 4096])), int(rng.choice([0, 1, 2, 4, 8, 8, 16, 255])), int(rng.choice([0, 1, 4, 4, 255])))


def draw_reset(p, back):
    """one state reset and, mostly, the other kind behind it; not a state whose mode has just come back on (it goes on as it was)"""
    rng, md = p.rng, p.md
    can = [s for s in STATES if p.on(s) and p.dirty[s] and s not in back]
    if not can:
        return
    s = can[int(rng.integers(0, len(can)))]
    p.call(s + "_reset")
    p.dirty[s] = None
    if rng.random() < 0.2:
        return
    if s == "depth":
        p.set_depth(("spliced" if md["depth"][0] == "plain" else "plain", md["depth"][1]))
    elif s == "junctions":
        p.junc_cap = JUNCTION_CAPACITIES[1 - JUNCTION_CAPACITIES.index(p.junc_cap)]
        p.set_junctions(md["junc_floor"])
    elif s == "pileup":
        p.set_pileup(("aligned", md["al_floor"] or md["pileup"][1]) if md["pileup"][0] == "owned" else ("owned", int(rng.choice([1, 3, 8]))))
    elif s == "fragments":
        p.set_pairs(draw_pairs(rng, int(rng.choice([b for b in N_BINS if b != p.n_bins]))))
    else:
        lengths = sorted({a - d for g, d, a in p.lists["a"]}) or [20]
        edge = int(lengths[int(rng.integers(0, len(lengths)))]) + int(rng.integers(0, 2))
        new = [m for m in (2, 3, 20, 65535, min(edge, 65535)) if m != md["indels"][1]]
        p.set_indels((md["indels"][0], int(new[int(rng.integers(0, len(new)))])))


def draw_off(p):
    """two modes off for the next group; the group after it gets them back"""
    rng = p.rng
    can = [w for w in ("depth", "junctions", "pileup", "fragments", "indels", "alignments", "rescue") if p.on(w)]
    if p.md["pileup"] and p.md["pileup"][0] == "aligned" and "alignments" in can and rng.random() < 0.5:
        can.remove("alignments")
    # the states that hold something first, in an order that turns with the seed and the group, so that every state gets its turn
    p.turn += 1
    order = [STATES[(p.turn + t) % len(STATES)] for t in range(len(STATES))]
    can = [w for w in order if w in can and p.dirty[w]] + [str(w) for w in rng.permutation(can) if not (w in STATES and p.dirty[w])]
    for w in can[:2]:
        w, md = str(w), p.md
        if w == "depth":
            p.back_on.append((w, md["depth"]))
            p.set_depth(None)
        elif w == "junctions":
            p.back_on.append((w, md["junc_floor"]))
            p.set_junctions(0)
        elif w == "pileup":
            p.back_on.append((w, md["pileup"]))
            p.set_pileup(None)
        elif w == "fragments":
            p.back_on.append((w, md["pairs"]))
            p.set_pairs(None)
        elif w == "indels":
            p.back_on.append((w, md["indels"]))
            p.set_indels(None)
        elif w == "alignments":
            p.back_on.append((w, md["al_floor"]))
            p.set_alignments(0)
        else:
            p.back_on.append((w, md["rescue"]))
            p.set_rescue(None)


def draw_back_on(p):
    order = sorted(p.back_on, key=lambda e: e[0] != "alignments")            # (pairs and rescue mode are set while alignments mode is on)
    p.back_on = []
    for w, v in order:
        {"depth": p.set_depth, "junctions": p.set_junctions, "pileup": p.set_pileup, "fragments": p.set_pairs, "indels": p.set_indels,
         "alignments": p.set_alignments, "rescue": p.set_rescue}[w](v)


def draw_edits(p, steps, last):
    """the calls in front of a group that is not the session's first.  last: no group follows this one"""
    rng, md = p.rng, p.md
    back = [w for w, _ in p.back_on]
    draw_back_on(p)
    for chance in (0.9, 0.5):
        if rng.random() < chance:
            draw_reset(p, back)
    if rng.random() < 0.7:
        md["seg_m"] = int(rng.integers(1, 4)) if md["seg_m"] == 4 else (4 if rng.random() < 0.75 else int(rng.integers(1, 4)))
        p.call("segments_enable", md["seg_m"])
    if rng.random() < 0.4:
        md["cand_m"] = int(rng.integers(0, capi.SHK_MAX_CANDIDATES + 1))
        p.call("candidates_enable", md["cand_m"])
    if rng.random() < 0.3:
        md["evidence"] = not md["evidence"]
        p.call("evidence_enable", md["evidence"])
    if rng.random() < 0.3:
        md["placement"] = not md["placement"]
        p.call("placement_enable", md["placement"])
    if rng.random() < 0.9:
        draw_floors(p)
    if rng.random() < 0.4:
        md["ext"] = (0, 0) if rng.random() < 0.3 else (int(rng.integers(1, 16)), int(rng.integers(0, 16)))
        p.call("alignments_extend", *md["ext"])
    if p.lists["a"] and rng.random() < 0.5:
        p.which = "b" if p.which == "a" else "a"
        p.call("splice_sites_set", p.which)
    if p.lists["a"] and rng.random() < 0.4:
        md["splice"] = None if (md["splice"] and rng.random() < 0.3) else \
            (int(rng.choice([1, 2, 3, 3, 8, 20, 48])), int(rng.integers(0, 9)), int(rng.integers(0, 7)))
        p.call("alignments_splice", *(md["splice"] or (0, 2, 2)))
    if md["al_floor"] and md["pairs"] and rng.random() < 0.4:
        p.set_pairs(draw_pairs(rng, p.n_bins))
    if md["al_floor"] and md["rescue"] and rng.random() < 0.4:
        p.set_rescue(draw_rescue(rng))
    # the merge calls: an earlier step's own contribution, as the model has it, added once more
    for what, name in (("pileup", "pileup_add"), ("indels", "indels_add")):
        src = [i for i, s in enumerate(steps) if s["modes"][what]]
        if src and p.on(what) and rng.random() < 0.3:
            p.call(name, int(src[int(rng.integers(0, len(src)))]))
            p.dirty[what] = p.dirty[what] or (md["pileup"][0] if what == "pileup" else True)
    if not last:
        draw_off(p)


def draw_batch(rng, ctx, md, n, paired, heavy):
    """n reads (pairs) of tests/fuzz_records.py's hostile classes; heavy: nearly every read a clean transcript read (the overflow batch)"""
    k, q, long = ctx["k"], ctx["min_quality"], ctx["long"]
    weights = dict(transcript=0.42, record=0.08, deleted=0.05, repeated=0.05, random=0.04, insertion=0.10, empty=0.02, short=0.03, exact_k=0.03,
                   long=0.06 if long is not None else 0.0, silenced=0.12 if paired else 0.0)
    if ctx["flavour"] == "indel":
        weights["indel"] = 0.8
    if heavy:
        weights = dict(transcript=0.85, record=0.05, deleted=0.05, insertion=0.05)
    s_floor = md["al_floor"] or (md["pileup"][1] if md["pileup"] else 8)
    max_frag = md["rescue"][1] if md["rescue"] else 1000
    sub = float(rng.choice([0.0, 0.01, 0.03]))
    m1s, m2s, classes = fz.draw_mates(rng, ctx["panel"], long, n, k, s_floor, max_frag, weights, sub)
    n_rate, other, lower = float(rng.choice([0.0, 0.002, 0.05])), float(rng.choice([0.0, 0.0, 0.005])), float(rng.choice([0.0, 0.0, 0.1]))
    if heavy:
        n_rate = other = 0.0
    m1s = [fz.spoil(rng, m, n_rate, other, lower) for m in m1s]
    m2s = [fz.spoil(rng, m, n_rate, other, lower) for m in m2s]
    for lst in (m1s, m2s):
        if not sum(len(m) for m in lst):
            lst[0] = synth.random_seq(rng, 30)
    q1 = [fz.qualities(rng, m) for m in m1s] if q else None
    q2 = [fz.qualities(rng, m) for m in m2s] if q else None
    batch = synth.batch_from_lists(m1s, m2s if paired else None, q1, q2 if paired else None)
    longest = max(max(len(m) for m in m1s), max(len(m) for m in m2s) if paired else 0)
    return batch, sorted(classes), longest


def draw_session(seed):
    """a session: plain Python numbers, lists and numpy arrays, deterministic in the seed"""
    rng = np.random.default_rng([int(seed), SESSION_KEY])
    flavour = FLAVOURS[int(seed) % len(FLAVOURS)]
    k = int(rng.choice(fz.KS))
    q = int(rng.choice([0, 0, 0, 2, 20]))
    hostile = float(rng.choice([0.0, 0.0, 0.02]))
    # ---- the context
    n_genes = 1 if flavour == "overflow" else int(rng.integers(2, 5))
    if flavour == "indel":
        panel = [fz.indel_gene(rng, int(rng.integers(0, 4)), k + max(fz.FLOORS) + 3, hostile) for _ in range(n_genes)]
    else:
        panel = [fz.spliced_gene(rng, int(rng.integers(1, 5)), k, hostile) for _ in range(n_genes)]
    twins = {"tie": int(rng.integers(2, 7)), "overflow": OVERFLOW_TWINS}.get(flavour, 0)
    genes_of_record = [panel[0]] * max(twins, 1) + panel[1:]
    long = fz.long_gene(rng) if flavour != "overflow" and rng.random() < 0.4 else None
    if long is not None:
        genes_of_record.append(long)
    records = [g["rec"] for g in genes_of_record]
    if flavour != "overflow" and rng.random() < 0.2:
        records.append(synth.random_seq(rng, int(rng.integers(max(k, 20), 64))))
        genes_of_record.append(None)
    lengths = [len(r) for r in records]
    sites_a = fz.draw_sites(rng, genes_of_record, lengths, crowded=bool(rng.random() < 0.2))
    # the other list: drawn anew and without gene 0's sites, so a mate of gene 0 whose end list `a` places stays clipped under `b`
    sites_b = [s for s in fz.draw_sites(rng, genes_of_record, lengths, crowded=False) if s[0] != 0] or sites_a[len(sites_a) // 2:]
    if not sites_a or not sites_b:
        sites_a = sites_b = []
    ctx = dict(k=k, min_quality=q, panel=panel, long=long, flavour=flavour)
    # ---- the modes of the first group: everything on
    al_floor = int(rng.choice(fz.FLOORS))
    md = dict(evidence=True, cand_m=int(rng.integers(1, capi.SHK_MAX_CANDIDATES + 1)), placement=True, seg_m=4 if rng.random() < 0.7 else int(rng.integers(1, 4)))
    md["depth"] = ("plain", int(rng.choice([1, 3, 8]))) if rng.random() < 0.5 else ("spliced", int(rng.choice([1, 3, 6, 8, 12])))
    md["junc_floor"] = int(rng.choice([1, 3, 8]))
    u = rng.random()
    md["pileup"] = ("owned", int(rng.choice([1, 3, 8]))) if u < 0.4 else ("aligned", al_floor if u < 0.7 else other_floor(rng, al_floor))
    md["al_floor"] = al_floor
    md["ext"] = (0, 0) if rng.random() < 0.3 else (int(rng.integers(1, 16)), int(rng.integers(0, 16)))
    md["splice"] = (int(rng.choice([1, 2, 3, 3, 8, 20, 48])), int(rng.integers(0, 9)), int(rng.integers(0, 7))) if sites_a and rng.random() < 0.8 else None
    md["pairs"] = draw_pairs(rng, int(rng.choice(N_BINS)))
    md["rescue"] = draw_rescue(rng)
    pile = md["pileup"][1] if md["pileup"][0] == "aligned" else 0
    v = rng.random()
    introns = sorted({a - d for g in panel for d, a, _ in g["introns"]})
    edge = int(introns[int(rng.integers(0, len(introns)))]) + int(rng.integers(0, 2)) if introns else 20
    md["indels"] = (al_floor if v < 0.4 else (pile if v < 0.6 and pile else other_floor(rng, al_floor, pile)), int(rng.choice([2, 3, 20, 20, 65535, edge])))
    plan = Plan(rng, md, dict(a=sites_a, b=sites_b), JUNCTION_CAPACITIES[int(rng.integers(0, 2))], turn=int(seed) // len(FLAVOURS))
    first_calls = [("evidence_enable", (True,)), ("candidates_enable", (md["cand_m"],)), ("placement_enable", (True,)), ("segments_enable", (md["seg_m"],))]
    plan.set_depth(md["depth"])
    plan.set_junctions(md["junc_floor"])
    plan.set_pileup(md["pileup"])
    plan.set_alignments(al_floor)
    plan.call("alignments_extend", *md["ext"])
    if sites_a:
        plan.call("splice_sites_set", "a")
    if md["splice"]:
        plan.call("alignments_splice", *md["splice"])
    plan.set_pairs(md["pairs"])
    plan.set_rescue(md["rescue"])
    plan.set_indels(md["indels"])
    plan.calls = first_calls + plan.calls
    # ---- the groups, the families, the slots
    n_steps = int(rng.integers(5, 8))
    pattern = PATTERNS[n_steps][int(rng.integers(0, len(PATTERNS[n_steps])))]
    families = []
    for size in pattern:
        if size == 1:
            families.append([str(rng.choice(fz.FAMILIES, p=[0.2, 0.2, 0.4, 0.2]))])
        else:
            families.append([str(rng.choice(["submit", "submit_device"])) for _ in range(size)])
    flat = [f for fam in families for f in fam]
    while sum(f != "classify_device" for f in flat) < 5:                        # (five hand-outs of the rotating slots: two reuses apart)
        i = flat.index("classify_device")
        flat[i] = "classify"
    turning = [i for i, f in enumerate(flat) if f != "classify_device"]         # step turning[r] lies in slot r % SHK_PIPE_DEPTH
    D = capi.SHK_PIPE_DEPTH
    # ---- the sizes: one slot reused by a smaller batch, another by a larger one that grows it
    sizes = [int(rng.choice(SMALL if flavour == "overflow" else SIZES)) for _ in flat]
    starts = [int(r) for r in rng.permutation(len(turning) - D)[:2]]
    if len(starts) == 2 and abs(starts[0] - starts[1]) == D:
        starts[1] = [r for r in range(len(turning) - D) if abs(r - starts[0]) != D and r != starts[0]][0]
    shrink, grow = starts
    sizes[turning[shrink]] = int(rng.choice(SMALL[1:] if flavour == "overflow" else LARGE))
    sizes[turning[shrink + D]] = 1 if flavour == "overflow" else int(rng.choice(SMALL))
    sizes[turning[grow]] = int(rng.choice(SMALL))
    sizes[turning[grow + D]] = 700
    heavy = turning[grow + D] if flavour == "overflow" else -1
    # ---- the steps
    steps, at = [], 0
    for g, size in enumerate(pattern):
        if g:
            draw_edits(plan, steps, last=g == len(pattern) - 1)
        for t in range(size):
            i = at + t
            family = flat[i]
            paired = True if i == heavy else bool(rng.random() < 0.65)
            batch, classes, longest = draw_batch(rng, ctx, plan.md, sizes[i], paired, heavy=i == heavy)
            bound = 0
            if family == "classify_device":
                bound = int(rng.choice([longest, 0, max(1, longest // 3)]))
            elif family == "submit_device":
                bound = min(int(rng.choice([longest, longest, max(1, longest // 3)])), fz.largest_submit_bound(k, paired))
            steps.append(dict(group=g, family=family, slot=D if family == "classify_device" else turning.index(i) % D, n=sizes[i], paired=paired,
                              batch=batch, classes=classes, longest=longest, bound=bound, modes=copy.deepcopy(plan.md), sites=plan.which,
                              calls=plan.calls if t == 0 else [], n_bins=plan.n_bins, junc_cap=plan.junc_cap))
            plan.calls = []
            plan.submitted()
        at += size
    return dict(seed=int(seed), flavour=flavour, k=k, c=0.0, min_quality=q, records=records, lengths=lengths, twins=twins, has_long=long is not None,
                intron_lengths=[sorted({a - d for d, a, _ in g["introns"]}) if g else [] for g in genes_of_record],
                sites=dict(a=sites_a, b=sites_b), pattern=pattern, steps=steps)


def step_case(session, step, **changes):
    """the step as a case of tests/fuzz_records.py: what expected, host_records and device_records take"""
    case = {key: session[key] for key in ("seed", "k", "c", "min_quality", "records", "lengths", "twins", "has_long", "intron_lengths")}
    case.update(bias="", times=1, sites=session["sites"][step["sites"]], **{key: step[key] for key in ("modes", "paired", "n", "batch", "classes", "longest", "family", "bound")})
    case.update(changes)
    return case


def describe_session(session):
    return "seed=%d %s k=%d records=%d twins=%d q=%d groups=%s steps=[%s]" % (
        session["seed"], session["flavour"], session["k"], len(session["records"]), session["twins"], session["min_quality"], "+".join(str(s) for s in session["pattern"]),
        " ".join("%s:%d%s@%d" % (s["family"], s["n"], "x2" if s["paired"] else "", s["slot"]) for s in session["steps"]))


# ---------------------------------------------------------------------------
# expected_session
# ---------------------------------------------------------------------------
class States:
    """the five accumulated states as the model holds them; add() takes one step's contribution out of fuzz_records.expected's result"""

    def __init__(self, total, n_bins):
        self.total = total
        self.depth = [np.zeros(total, np.uint32), 0]
        self.junctions = {}
        self.pileup = [np.zeros((total, 4), np.uint32), 0]
        self.fragments = [np.zeros(n_bins, np.uint64), np.zeros(6, np.uint64)]
        self.indels = [{}, {name: 0 for name in capi.INDEL_STAT_NAMES}]

    def reset(self, what, n_bins=None):
        fresh = States(self.total, n_bins or len(self.fragments[0]))
        setattr(self, what, getattr(fresh, what))

    def add(self, w, only=STATES):
        if "depth" in w and "depth" in only:
            self.depth = [self.depth[0] + w["depth"][0], self.depth[1] + int(w["depth"][1])]
        if "junctions" in w and "junctions" in only:
            for g, d, a, intron, n in w["junctions"]:
                e = self.junctions.setdefault((g, d, a), [intron, 0])
                e[0], e[1] = min(e[0], intron), e[1] + n
        if "pileup" in w and "pileup" in only:
            self.add_pileup(*w["pileup"])
        if "fragments" in w and "fragments" in only:
            self.fragments = [self.fragments[0] + w["fragments"][0], self.fragments[1] + w["fragments"][1]]
        if "indels" in w and "indels" in only:
            self.add_indels(*w["indels"])

    def bins(self, n_bins, planted=False):
        """the fragments state at the step's n_bins: another one is only ever taken behind a reset, and the state is allocated anew
        (planted: a fold with a fault in it, where the reset may be the fault)"""
        if n_bins != len(self.fragments[0]):
            assert planted or self.empty("fragments")
            self.reset("fragments", n_bins)

    def add_pileup(self, counts, mates):
        self.pileup = [self.pileup[0] + counts, self.pileup[1] + int(mates)]

    def add_indels(self, arr, stats):
        for e in arr:
            t = self.indels[0].setdefault(tuple(int(e[f]) for f in ("gene", "x", "kind", "len", "seq")), [0, 0])
            t[0], t[1] = t[0] + int(e["fwd"]), t[1] + int(e["rev"])
        for name, v in stats.items():
            self.indels[1][name] += int(v)

    def empty(self, what):
        return {"depth": not self.depth[1], "junctions": not self.junctions, "pileup": not self.pileup[1], "fragments": not self.fragments[1].any(),
                "indels": not self.indels[1]["mates"] and not self.indels[0]}[what]

    def snapshot(self, sm, gene_start):
        """the states as the read-outs hand them out"""
        counts = self.pileup[0].copy()
        return dict(depth=(self.depth[0].copy(), int(self.depth[1])), junctions=table_rows(self.junctions), pileup=(counts, int(self.pileup[1])),
                    variants=[(expected_variants(counts, sm.records, gene_start, prm), expected_summary(counts, sm.records, gene_start, prm)) for prm in fz.VARIANT_PARAMS],
                    fragments=(self.fragments[0].copy(), self.fragments[1].copy()), indels=(table_array(self.indels[0]), dict(self.indels[1])),
                    empty={s: self.empty(s) for s in STATES})


def kinds_on(md):
    """which of STATE_KINDS a batch submitted under these modes adds to"""
    on = set()
    if md["depth"]:
        on.add("depth." + md["depth"][0])
    if md["junc_floor"]:
        on.add("junctions")
    if md["pileup"]:
        on.add("pileup." + md["pileup"][0])
    if md["al_floor"] and md["pairs"]:
        on.add("fragments")
    if md["indels"]:
        on.add("indels")
    return on


def launches(md):
    """the floors of alignments mode, aligned pileup and indels mode (0: off): equal floors share one align_kernel launch"""
    return (md["al_floor"], md["pileup"][1] if md["pileup"] and md["pileup"][0] == "aligned" else 0, md["indels"][0] if md["indels"] else 0)


def there_and_back(seq, is_a, is_b):
    """how often the sequence goes from an a to one or more b and back to an a"""
    n = 0
    for a in range(len(seq)):
        b = a + 1
        while is_a(seq[a]) and b < len(seq) and is_b(seq[b]):
            b += 1
        n += b > a + 1 and b < len(seq) and bool(is_a(seq[b]))
    return n


def apply_calls(states, calls, wants):
    """what a group's calls do to the states: the resets and the two merge calls"""
    for name, args in calls:
        if name.endswith("_reset"):
            states.reset(name[:-len("_reset")])
        elif name == "pileup_add":
            states.add_pileup(*wants[args[0]]["pileup"])
        elif name == "indels_add":
            states.add_indels(*wants[args[0]]["indels"])


def fold_states(session, wants, skip=(), unapplied=(), extra=None):
    """the snapshots behind each group from the steps' models -- and, for tests/test_fuzz_sessions_cpu.py, with a fault planted:
    skip: (step, state) whose contribution goes missing; unapplied: (step, position in its calls) of calls that are not made;
    extra: {step: a contribution in fuzz_records.expected's form} counted on top"""
    steps = session["steps"]
    sm, gs = wants[0]["model"], wants[0]["gene_start"]
    states = States(int(gs[-1]), steps[0]["n_bins"])
    snapshots = []
    for i, (s, w) in enumerate(zip(steps, wants)):
        apply_calls(states, [c for j, c in enumerate(s["calls"]) if (i, j) not in unapplied], wants)
        states.bins(s["n_bins"], planted=bool(skip or unapplied or extra))
        states.add(w, only=[st for st in STATES if (i, st) not in skip])
        if extra and i in extra:
            states.add(extra[i])
        if i + 1 == len(steps) or steps[i + 1]["group"] != s["group"]:
            snapshots.append(states.snapshot(sm, gs))
    return snapshots


def expected_session(session, oracle):
    """dict(steps: fuzz_records.expected per step, snapshots: the states behind each group, slots: per step (the slot's capacity in
    associations in front of the step, the associations of the slot's batch before, or None), coverage)"""
    steps = session["steps"]
    wants = [fz.expected(step_case(session, s), oracle, primed=False) for s in steps]
    sm, gs = wants[0]["model"], wants[0]["gene_start"]
    states = States(int(gs[-1]), steps[0]["n_bins"])
    cov = {}
    bump = fz._bump
    snapshots, slots = [], []
    cap, held = {}, {}
    for i, (s, w) in enumerate(zip(steps, wants)):
        md = s["modes"]
        before = {st: states.empty(st) for st in STATES}
        apply_calls(states, s["calls"], wants)
        for name, args in (s["calls"] if i else []):
            if name.endswith("_reset"):
                st = name[:-len("_reset")]
                bump(cov, "reset." + st, not before[st])
                was, now = steps[i - 1]["modes"], md
                other = {"depth": was["depth"] and now["depth"] and was["depth"][0] != now["depth"][0],
                         "pileup": was["pileup"] and now["pileup"] and was["pileup"][0] != now["pileup"][0],
                         "junctions": s["junc_cap"] != steps[i - 1]["junc_cap"], "fragments": s["n_bins"] != steps[i - 1]["n_bins"],
                         "indels": was["indels"] and now["indels"] and was["indels"][1] != now["indels"][1]}[st]
                bump(cov, "kind_after_reset." + st, bool(other) and not before[st])
            bump(cov, name, name in ("pileup_add", "indels_add"))
        # ---- the slot: its capacity as the library grows it, and what it held
        n_assoc, slot = int(w["goff"][-1]), s["slot"]
        c0 = cap.get(slot, 0)
        c1 = max(c0, grown(2 * s["n"] + 4096)) if 2 * s["n"] + 4096 > c0 else c0
        overflow = n_assoc > c1
        c2 = grown(n_assoc + 8) if overflow else c1
        slots.append(dict(cap=c1, held=held.get(slot), overflow=overflow))
        if slot in held:
            if n_assoc < held[slot]:
                for kind in kinds_on(md):
                    bump(cov, "fewer_in_slot." + kind)
                bump(cov, "fewer_in_slot")
            bump(cov, "slot_grown", c2 > c0)
        cap[slot], held[slot] = c2, n_assoc
        too_long = w["expect_long"]
        bump(cov, "repair.overflow.inside", overflow and i > 0)
        bump(cov, "repair.length.inside", too_long and i > 0)
        bump(cov, "repair.length.inside.submit_device", too_long and i > 0 and s["family"] == "submit_device")
        bump(cov, "family." + s["family"])
        states.bins(s["n_bins"])
        states.add(w)
        if i + 1 == len(steps) or steps[i + 1]["group"] != s["group"]:
            snapshots.append(states.snapshot(sm, gs))
        # ---- a replaced site list that decides a record
        if i and s["sites"] != steps[i - 1]["sites"] and md["splice"] and md["al_floor"] and n_assoc <= 4096:       # (not the overflow batch: its models twice over)
            old = fz.expected(step_case(session, s, sites=session["sites"][steps[i - 1]["sites"]]), oracle, primed=False)
            bump(cov, "sites_replaced.changes_a_record", old["before_rescue"].tobytes() != w["before_rescue"].tobytes())
    # ---- the groups
    groups = [[i for i, s in enumerate(steps) if s["group"] == g] for g in range(len(session["pattern"]))]
    for idx in groups:
        different = len({steps[i]["batch"]["seq1"].tobytes() for i in idx}) == len(idx)
        bump(cov, "group.%d" % len(idx), len(idx) > 1 and different)
        bump(cov, "group.mixed", len({steps[i]["family"] for i in idx}) > 1)
    gm = [steps[idx[0]]["modes"] for idx in groups]
    segs = [m["seg_m"] for m in gm]
    bump(cov, "seg_m.4_below_4", there_and_back(segs, lambda m: m == 4, lambda m: m < 4))
    # floors that merge and split launches on the live context: each group against the last one before it that ran the same modes
    last = {}
    for m in gm:
        al1, p1, i1 = launches(m)
        for key, other in (("pileup", p1), ("indels", i1)):
            if al1 and other:
                if key in last:
                    bump(cov, "launches.%s.merged" % key, not last[key] and al1 == other)
                    bump(cov, "launches.%s.split" % key, last[key] and al1 != other)
                last[key] = al1 == other
        if al1 and p1 and i1:
            three = len({al1, p1, i1}) == 3
            bump(cov, "launches.three", three and "three" in last and not last["three"])
            last["three"] = three
    # a mode off for a group and on again, its state holding something meanwhile
    for kind in STATE_KINDS:
        on = [kind in kinds_on(m) for m in gm]
        for g in range(1, len(gm) - 1):
            if on[g - 1] and not on[g] and on[g + 1] and not snapshots[g]["empty"][kind.split(".")[0]]:
                bump(cov, "off_on." + kind)
    ends = [s["paired"] for s in steps]
    bump(cov, "paired_single_paired", there_and_back(ends, lambda e: e, lambda e: not e))
    return dict(steps=wants, snapshots=snapshots, slots=slots, groups=groups, coverage=cov)


# ---------------------------------------------------------------------------
# the comparison
# ---------------------------------------------------------------------------
def model_records(w, md):
    """a step's records as a faultless device hands them out: fuzz_records.host_records' dictionary, from the model"""
    rec = {}
    if md["evidence"]:
        rec["evidence"] = w["evidence"]
    if md["cand_m"]:
        rec["candidate reads"], rec["candidate entries"] = w["candidates"]
    if md["placement"]:
        rec["placement"] = w["placement"]
    rec["segment keys"], rec["segment entries"] = w["segments"]
    if md["al_floor"]:
        rec["alignments"] = w["alignments"]
        if md["rescue"]:
            rec["rescue"] = w["rescue"]
        if md["pairs"]:
            rec["pairs"] = w["pairs"]
    return rec


def model_results(session, want):
    """dict(hand_outs: per step (gene_off, gene_ids, records), states: per group the read-outs), copies the caller may spoil"""
    hand_outs = [(w["goff"].astype(np.uint32), w["gids"].astype(np.uint16), {key: copy.deepcopy(v) for key, v in model_records(w, s["modes"]).items()})
                 for s, w in zip(session["steps"], want["steps"])]
    return dict(hand_outs=hand_outs, states=[copy.deepcopy({key: v for key, v in snap.items() if key != "empty"}) for snap in want["snapshots"]])


def check_hand_out(session, want, i, hand_out):
    """None, or how step i's hand-out differs from step i's model"""
    goff, gids, rec = hand_out
    md = session["steps"][i]["modes"]
    wanted = set(model_records(want["steps"][i], md))
    if set(rec) != wanted:
        return "step %d: record kinds %s, model %s" % (i, sorted(rec), sorted(wanted))
    bad = fz.compare_records(rec, want["steps"][i], goff, gids)
    return "step %d (%s, %d reads, slot %d): %s" % (i, session["steps"][i]["family"], session["steps"][i]["n"], session["steps"][i]["slot"], bad) if bad else None


def check_states(session, want, g, got):
    """None, or how the states read behind group g differ from the model's snapshot"""
    snap = want["snapshots"][g]
    bad = fz.first_difference("depth", got["depth"][0], snap["depth"][0]) or fz.first_difference("depth mates", np.uint64(got["depth"][1]), np.uint64(snap["depth"][1]))
    if not bad and [tuple(r) for r in got["junctions"]] != snap["junctions"]:
        a, b = [tuple(r) for r in got["junctions"]], snap["junctions"]
        j = next((x for x, (u, v) in enumerate(zip(a, b)) if u != v), min(len(a), len(b)))
        bad = "junction table: row %d: got %s, model %s (%d rows, model %d)" % (j, a[j:j + 1], b[j:j + 1], len(a), len(b))
    bad = bad or fz.first_difference("pileup", got["pileup"][0], snap["pileup"][0]) or \
        fz.first_difference("pileup mates", np.uint64(got["pileup"][1]), np.uint64(snap["pileup"][1]))
    for prm, (gv, gsum), (wv, wsum) in zip(fz.VARIANT_PARAMS, got["variants"], snap["variants"]):
        bad = bad or fz.first_difference("variants %s" % (prm,), gv, wv) or fz.first_difference("variants summary %s" % (prm,), gsum, wsum)
    bad = bad or fz.first_difference("fragment classes", got["fragments"][1], snap["fragments"][1]) or \
        fz.first_difference("fragment histogram", got["fragments"][0], snap["fragments"][0])
    bad = bad or fz.compare_indels(got["indels"][0], got["indels"][1], snap["indels"])
    return "behind group %d (steps %s): %s" % (g, want["groups"][g], bad) if bad else None


def check_session(session, want, results):
    """the first mismatch of a whole session's results in the order the device meets them, or None"""
    for g, idx in enumerate(want["groups"]):
        for i in idx:
            bad = check_hand_out(session, want, i, results["hand_outs"][i])
            if bad:
                return bad
        bad = check_states(session, want, g, results["states"][g])
        if bad:
            return bad
    return None


# ---------------------------------------------------------------------------
# run_session
# ---------------------------------------------------------------------------
def make_calls(h, session, want, calls):
    for name, args in calls:
        if name == "splice_sites_set":
            h.splice_sites_set(np.array(session["sites"][args[0]], dtype=np.int64).reshape(-1, 3))
        elif name == "pileup_add":
            h.pileup_add(*want["steps"][args[0]]["pileup"])
        elif name == "indels_add":
            h.indels_add(*want["steps"][args[0]]["indels"])
        else:
            getattr(h, name)(*args)


def read_states(h, n_bins):
    """every state of the context, its mode on or off"""
    stats = h.indels_stats()
    return dict(depth=(h.depth_all(), h.depth_mates()), junctions=[tuple(int(v) for v in r) for r in h.junctions_get()], pileup=(h.pileup_all(), h.pileup_mates()),
                variants=[(h.variants(prm[0], prm[1], (prm[2], prm[3])), h.variants_summary(prm[0], prm[1], (prm[2], prm[3]))) for prm in fz.VARIANT_PARAMS],
                fragments=h.fragments(n_bins), indels=(None if stats["dropped"] else h.indels_get(0), stats))


def run_session(session, oracle, want=None):
    """(None or the first mismatch's message, facts: per step the associations handed out and timing()'s last_n_long behind its wait)"""
    import torch  # noqa: F401  (torch bundles its own HIP runtime: load it BEFORE libsharkhip so one runtime serves both)
    from tests.test_gpu_segments import _dev_ptrs, _to_device
    want = want or expected_session(session, oracle)
    steps = session["steps"]
    h = fz.build_context(step_case(session, steps[0]), want["steps"][0]["nidx"])
    replay = "  (replay: python tests/fuzz_sessions.py 1 %d)" % session["seed"]
    facts = []
    try:
        for g, idx in enumerate(want["groups"]):
            make_calls(h, session, want, steps[idx[0]]["calls"])
            resident = {i: _to_device(steps[i]["batch"]) for i in idx if steps[i]["family"] in ("classify_device", "submit_device")}
            tickets = {}
            for i in idx:                                        # (a group of one of the two synchronous families is its one call below)
                s = steps[i]
                if s["family"] == "submit":
                    tickets[i] = h.submit(*fz._args(s["batch"]))
                elif s["family"] == "submit_device":
                    tickets[i] = h.submit_device(s["n"], max_read_len=s["bound"], **_dev_ptrs(resident[i]))
            for i in idx:
                s, md = steps[i], steps[i]["modes"]
                if s["family"] == "classify":
                    goff, gids = h.classify(*fz._args(s["batch"]))
                    hand_out = (goff, gids, fz.host_records(h, md))
                elif s["family"] == "submit":
                    goff, gids = h.wait(tickets[i])
                    hand_out = (goff, gids, fz.host_records(h, md))
                elif s["family"] == "classify_device":
                    hand_out = fz.device_records(h, md, h.classify_device(s["n"], max_read_len=s["bound"], **_dev_ptrs(resident[i])))
                else:
                    hand_out = fz.device_records(h, md, h.wait_device(tickets[i]))
                facts.append(dict(step=i, family=s["family"], n_assoc=int(hand_out[0][-1]), last_n_long=int(h.timing()["last_n_long"])))
                bad = check_hand_out(session, want, i, hand_out)
                if bad:
                    return bad + replay, facts
            bad = check_states(session, want, g, read_states(h, steps[idx[-1]]["n_bins"]))
            if bad:
                return bad + replay, facts
        return None, facts
    finally:
        h.close()


# ---------------------------------------------------------------------------
# the replay and soak driver
# ---------------------------------------------------------------------------
def main():
    from oracle import pyoracle
    if not os.path.exists(pyoracle.LIB_PATH):
        pyoracle.build()
    iters = int(sys.argv[1]) if len(sys.argv) > 1 else 20
    seed0 = int(sys.argv[2]) if len(sys.argv) > 2 else 20340021
    t_start = time.time()
    total = {}
    for it in range(iters):
        session = draw_session(seed0 + it)
        want = expected_session(session, pyoracle)
        bad, facts = run_session(session, pyoracle, want)
        for key, v in want["coverage"].items():
            total[key] = total.get(key, 0) + v
        print("%4d %s assoc=%s %s" % (it, describe_session(session), [f["n_assoc"] for f in facts], "ok" if not bad else "MISMATCH"), flush=True)
        if bad:
            print(bad)
            print("replay: python tests/fuzz_sessions.py 1 %d" % (seed0 + it))
            sys.exit(1)
    print("FUZZ OK: %d sessions in %.0f s; coverage %s" % (iters, time.time() - t_start, dict(sorted(total.items()))))


if __name__ == "__main__":
    main()
