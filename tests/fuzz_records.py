#!/usr/bin/env python3
"""(test infrastructure)  Randomised differential test of the record modes -- everything behind the classify kernel -- against their
exact Python models, every mode on at once: evidence, candidates, placement, segments, alignments with gap closure, end extension and
spliced ends, rescue, pairs and the fragments state, plain or spliced depth, the junction table, owned or aligned pileup and the
variants read from it, and the indel table with its counters (at alignments mode's floor, at another, or without alignments mode; its
parameters come from a random stream of their own, and it is off in one case of five).  Three separable parts, so that the CPU can do everything but the comparison:

  draw(seed, bias)        a case from numpy alone: reference, batch, every mode's parameters, the entry family.  No GPU, no oracle.
  expected(case, oracle)  the CPU oracle's associations and, chained in the order the crafted tests use, every model's records and
                          states, plus a `coverage` dictionary of what the case exercised.
  run(case, oracle)       the same case on the device through the drawn family; genes against the oracle first, then every record
                          kind byte for byte and every accumulator element for element.  No tolerances.

The mates are hostile on purpose: besides tests/spliced_synth.py's classes (transcript, record, two bases deleted, six repeated,
random) there are insertions of 1 to 70 junk bases at a junction, empty mates, mates shorter than k and of exactly k bases, unspliced
mates of 129 to 700 bases from a long record, N, lower case and other bytes, and SILENCED mates: a copy of record bases beside a
cleanly placed partner with just enough evenly spread substitutions to leave fewer than s_min clean windows (tests/rescue_cases.py's
idea), which is what reaches rescue_kernel's placing path.  The `indel` bias draws genes whose exons hold a low-complexity stretch and
mates with one planted event inside an exon (indel_gene, indel_mate): what indel_kernel's left-normalisation works on.

tests/test_fuzz_records_cpu.py runs draw and expected over the committed schedule and asserts what the schedule covers;
tests/test_gpu_fuzz_records.py runs the schedule in the `-m gpu` suite.  By hand on a GPU box:
    timeout -k 10 600 python tests/fuzz_records.py [iterations] [seed] [bias]
prints one line per case, stops at the first mismatch and prints the line that replays it (`python tests/fuzz_records.py 1 SEED BIAS`).
A soak is the same command with more iterations and a fresh seed; give every such step a time limit of its own, as above, and stop at
the first fault instead of starting the next step."""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

from shark_amd import capi
from shark_amd.capi import SHK_INLINE_IDS, SHK_MAX_CANDIDATES
from tests import synth
from tests.candidates_model import expected_candidates
from tests.depth_model import expected_depth, model_layout
from tests.evidence_model import expected_evidence
from tests.align_model import expected_alignments
from tests.extend_model import best_extension, expected_aligned_pileup
from tests.indels_model import expected_indels, new_stats, record_events, table_array
from tests.pairs_model import Fragments, expected_pairs
from tests.pileup_model import expected_pileup
from tests.placement_model import expected_placements, masked_mates
from tests.rescue_cases import silencing
from tests.rescue_model import expected_rescue
from tests.segments_model import SegmentsModel, expected_segments
from tests.splice_model import check_sites, expected_alignments_spliced, ranged_candidates
from tests.spliced_model import expected_junction_table, expected_spliced_depth, table_rows
from tests.variants_model import DEFAULTS as VARIANT_DEFAULTS
from tests.variants_model import expected_summary, expected_variants

BIASES = ("", "splice", "rescue", "tie", "wide", "indel")
# the random streams' keys, each an explicit number: default_rng([seed, key]) draws a case's reference, batch and every mode but indels,
# default_rng([seed, key, 1]) indels mode's parameters (a second stream: the first one's consumption is what it was before that mode)
BIAS_KEY = {"": 0, "splice": 1, "rescue": 2, "tie": 3, "wide": 4, "indel": 6}
WIDE_B_KEY, WIDE_C_KEY = 5, 7
assert sorted(BIAS_KEY) == sorted(BIASES) and len(set(BIAS_KEY.values()) | {WIDE_B_KEY, WIDE_C_KEY}) == len(BIASES) + 2
KS = (5, 11, 16, 17, 21, 31)
FLOORS = (1, 3, 6, 8, 12)
FAMILIES = ("classify", "submit", "classify_device", "submit_device")
CLASSES = ("transcript", "record", "deleted", "repeated", "random", "insertion", "empty", "short", "exact_k", "long", "silenced", "indel")
BF_BITS = 1 << 26
JUNCTION_CAPACITY = 1 << 16          # (a batch tied over six genes at k = 5 and floor 1 shows more than 4 096 distinct junctions)
VARIANT_PARAMS = (VARIANT_DEFAULTS, (1, 1, 0, 1))
PL_WAVES, PL_MAX_BLOCKS = 4, 2048            # placement_kernel, segments_kernel, pileup_kernel, align_kernel: one wave per read
WIDE_A_PAIRS = PL_MAX_BLOCKS * PL_WAVES + 65
DEPTH_LANES = 2048 * 256                     # depth_accumulate_kernel, spliced_accumulate_kernel: one thread per read
WIDE_B_BLOCK, WIDE_B_TIMES, WIDE_B_REST = 1021, 513, 836
WIDE_B_PAIRS = DEPTH_LANES + 321
assert WIDE_B_BLOCK * WIDE_B_TIMES + WIDE_B_REST == WIDE_B_PAIRS
WIDE_C_FLOOR, WIDE_C_MIN_INTRON = 8, 20      # wide case (c): indel_kernel, one thread per read as well; (b)'s shape, a batch of its own
INDEL_COUNTERS = ("deletions", "insertions", "complex_gaps", "long_insertions", "nonbase_insertions")      # the five classifying ones
LETTERS = np.frombuffer(b"NRYKMSWBDHV", dtype=np.uint8)       # (letters only: under -q the reference is undefined on bytes below '@')


def _args(b):
    return b["seq1"], b["off1"], b["seq2"], b["off2"], b["qual1"], b["qual2"]


def largest_submit_bound(k, paired):
    """the largest max_read_len shk_classify_device_submit takes: the bound's slots must fit the largest kernel specialisation (640)"""
    def slots(n):
        per = n - k + 1 if n >= k else 0
        return ((n + 7) & ~7) + per if (paired and per) else per
    return max(n for n in range(1, 641 + k) if slots(n) <= 640)


def slot_reserve(n):
    """the associations a slot's first reservation holds for a batch of n reads (tests/test_gpu_publish_records.py's inequality)"""
    return 2 * n + 4096 + (2 * n + 4096) // 4 + 64


# ---------------------------------------------------------------------------
# the reference
# ---------------------------------------------------------------------------
def spliced_gene(rng, n_introns, k, hostile=0.0):
    """tests/spliced_synth.py's gene with its coordinates kept: dict(rec, tr, introns [(donor, acceptor)], cuts: the transcript offsets
    of the junctions).  Introns of 30 to 90 bases (a closure of R = 64 read bases needs G >= 64); now and then an intron begins like
    the exon behind it (microhomology of 1 to 3 bases: the junction has two descriptions)"""
    lo, hi = (18, 40) if k <= 17 else (k + 3, k + 20)
    exons = [synth.random_seq(rng, int(rng.integers(lo, hi))) for _ in range(n_introns + 1)]
    exons[0] = synth.random_seq(rng, 70)
    exons[-1] = synth.random_seq(rng, 70)
    parts, introns, spans, at = [], [], [], 0
    for i, e in enumerate(exons):
        if i:
            gap = synth.random_seq(rng, int(rng.integers(30, 91)))
            same = int(rng.integers(1, 4)) if rng.random() < 0.3 else 0
            gap[:same] = e[:same]
            parts.append(gap)
            introns.append((at, at + len(gap), same))
            at += len(gap)
        parts.append(e)
        spans.append((at, at + len(e)))
        at += len(e)
    rec = np.concatenate(parts)
    if hostile:
        spoil_record(rng, rec, hostile)
    tr = np.concatenate([rec[a:b] for a, b in spans])
    cuts = np.cumsum([b - a for a, b in spans])[:-1].tolist()
    return dict(rec=rec, tr=tr, introns=introns, cuts=cuts)


def spoil_record(rng, rec, hostile):
    """lower case, N and '-' in a record, never at its two ends"""
    u = rng.random(len(rec))
    u[[0, -1]] = 1.0
    rec[u < hostile] |= 0x20
    rec[u < hostile / 2] = ord("N")
    rec[u < hostile / 8] = ord("-")


def indel_gene(rng, n_introns, margin, hostile=0.0):
    """the gene of the `indel` bias: spliced_gene's dict and introns, but exons long enough to hold an event with a block of the drawn
    floor on either side (margin = the clean bases such a block needs), and inside every exon a planted low-complexity STRETCH of 8 to
    80 bases -- a homopolymer, a di- or a trinucleotide repeat --, where an event shifts left by more than its own length.
    spans: the exons' record ranges; stretches: per exon (record offset, length, unit length)"""
    parts, introns, spans, stretches, at = [], [], [], [], 0
    for i in range(n_introns + 1):
        left, right = (synth.random_seq(rng, int(rng.integers(margin + 30, margin + 71))) for _ in range(2))
        u = int(rng.choice([1, 1, 2, 2, 3]))
        unit = synth.random_seq(rng, u)
        if u > 1 and len(set(unit.tolist())) == 1:
            unit[0] = synth.ACGT[(int(np.searchsorted(synth.ACGT, unit[0])) + 1) % 4]
        n = int(rng.choice([8, 12, 20, 30, 45, 64, 80, int(rng.integers(8, 81))]))
        e = np.concatenate([left, np.tile(unit, n // u + 1)[:n], right])
        if i:
            gap = synth.random_seq(rng, int(rng.integers(30, 91)))
            same = int(rng.integers(1, 4)) if rng.random() < 0.3 else 0
            gap[:same] = e[:same]
            parts.append(gap)
            introns.append((at, at + len(gap), same))
            at += len(gap)
        parts.append(e)
        spans.append((at, at + len(e)))
        stretches.append((at + len(left), n, u))
        at += len(e)
    rec = np.concatenate(parts)
    if hostile:
        spoil_record(rng, rec, hostile)
    tr = np.concatenate([rec[a:b] for a, b in spans])
    cuts = np.cumsum([b - a for a, b in spans])[:-1].tolist()
    return dict(rec=rec, tr=tr, introns=introns, cuts=cuts, spans=spans, stretches=stretches, margin=margin)


def long_gene(rng):
    """an unspliced record of 1 500 to 2 500 bases with a tandem copy: bases [400, 500) stand again at [560, 660), so a mate cut from
    either is silent as it is (its k-mers occur twice) and has two places of equal cost"""
    rec = synth.random_seq(rng, int(rng.integers(1500, 2501)))
    rec[560:660] = rec[400:500]
    return dict(rec=rec, tr=rec, introns=[], cuts=[], tandem=(400, 560, 100))


def substituted(m, at):
    """the bases at `at` replaced by the next base of ACGT (whatever case or byte stood there)"""
    m = m.copy()
    for i in at:
        c = int(np.searchsorted(synth.ACGT, m[i] & 0xDF))
        m[i] = synth.ACGT[(c + 1) % 4]
    return m


# ---------------------------------------------------------------------------
# the mates
# ---------------------------------------------------------------------------
def indel_mate(rng, gene):
    """a transcript or record mate of an indel_gene with ONE planted event inside an exon, at least the gene's margin of bases away from
    the mate's ends and, for the events outside the stretch, from the exon's: a deletion of 1 to 30 record bases, an insertion of 1 to 12
    or of 13 to 40 random bases, a tandem duplication (the inserted bases copy the record bases in front of them), or -- every third mate
    -- units of the exon's low-complexity stretch lost or gained somewhere inside it (or one random base gained there); the mate then
    spans the whole stretch.  Which gaps come out of it is the alignment model's business"""
    m = gene["margin"]
    e = int(rng.integers(0, len(gene["spans"])))
    a, b = gene["spans"][e]
    s0, sn, u = gene["stretches"][e]
    rec = gene["rec"]
    if rng.random() < 0.5:
        src, shift = rec, 0
    else:
        src, shift = gene["tr"], sum(y - x for x, y in gene["spans"][:e]) - a
    what = str(rng.choice(["deletion", "insertion", "long", "duplication", "stretch", "stretch"]))
    gone, piece = 0, np.zeros(0, np.uint8)
    if what == "stretch":
        n = min(u * int(rng.choice([1, 1, 2, 3, 5])), sn)
        if rng.random() < 0.5:
            x = s0 + int(rng.integers(0, sn - n + 1))
            gone = n
        else:
            x = s0 + int(rng.integers(0, sn + 1))
            piece = rec[x - n:x].copy() if x - n >= s0 else rec[x:x + n].copy()
            if rng.random() < 0.2:
                piece = synth.random_seq(rng, 1)
        lo, hi = s0, s0 + sn
    else:
        if what == "deletion":
            gone = int(rng.integers(1, 31))
        x = int(rng.integers(a + m, b - m - gone + 1))
        if what != "deletion":
            n = int(rng.integers(13, 41)) if what == "long" or (what == "duplication" and rng.random() < 0.2) else int(rng.integers(1, 13))
            piece = rec[x - min(n, x - a):x].copy() if what == "duplication" else synth.random_seq(rng, n)
        lo, hi = x, x + gone
    la, lb = x - lo + m + int(rng.integers(0, 21)), hi - (x + gone) + m + int(rng.integers(0, 21))
    p = x + shift
    return np.concatenate([src[max(0, p - la):p], piece, src[p + gone:p + gone + lb]])


def one_mate(rng, kind, gene, long, k):
    """one mate of class `kind` in the record's orientation"""
    rec, tr = gene["rec"], gene["tr"]
    L = int(rng.integers(60, 121))
    if kind == "indel":
        return indel_mate(rng, gene)
    if kind == "empty":
        return np.zeros(0, np.uint8)
    if kind in ("short", "exact_k"):
        L = k if kind == "exact_k" else int(rng.integers(1, k))
        a = int(rng.integers(0, len(tr) - L + 1))
        return tr[a:a + L].copy()
    if kind == "long":
        rec = long["rec"]
        L = int(rng.choice([129, 300, 511, 512, 513, 700, int(rng.integers(129, 701))]))
        a = int(rng.integers(0, len(rec) - L + 1))
        return rec[a:a + L].copy()
    if kind == "random":
        return synth.random_seq(rng, L)
    if kind == "insertion" and gene["cuts"]:
        R = int(rng.choice([1, 2, 3, 8, 20, 30, 40, 63, 64, 64, 64, 65, 65, 66, 70, int(rng.integers(1, 71))]))
        fits = [i for i, (d, a, _) in enumerate(gene["introns"]) if a - d >= R] or list(range(len(gene["cuts"])))
        i = fits[int(rng.integers(0, len(fits)))]
        t = gene["cuts"][i]
        la, lb = int(rng.integers(25, 56)), int(rng.integers(25, 56))
        return np.concatenate([tr[max(0, t - la):t], synth.random_seq(rng, R), tr[t:t + lb]])
    src = rec if kind == "record" else tr
    L = min(L, len(src) - 8)
    a = int(rng.integers(0, len(src) - L + 1))
    if kind == "record" and rng.random() < 0.4:
        a = 0 if rng.random() < 0.5 else len(src) - L
    if kind == "deleted":
        return np.concatenate([src[a:a + L // 2], src[a + L // 2 + 2:a + L + 2]])
    if kind == "repeated":
        return np.concatenate([src[a:a + L // 2], src[a + L // 2 - 6:a + L - 6]])
    return src[a:a + L].copy()


def silenced_pair(rng, gene, long, k, s_min, max_frag):
    """(anchor, target), both as they are sequenced: the anchor a clean copy of record bases, the target a copy of record bases on the
    other strand with silencing substitutions.  Flavours: inside the partner's window (rescued: states 4, 5), in the long record's
    tandem copy (two places of equal cost: state 3), outside the window (state 2, or 1 where the window is empty), substituted twice as
    heavily (state 2)"""
    flavour = str(rng.choice(["near", "near", "near", "copy", "far", "heavy"]))
    if flavour in ("copy", "far") and long is None:
        flavour = "near"
    if flavour in ("copy", "far") or (long is not None and rng.random() < 0.3):
        gene = long
    rec = gene["rec"]
    la = min(int(rng.integers(60, 101)), len(rec) - 8)
    lt = min(int(rng.choice([32, 33, 40, 60, 64, 65, 100, int(rng.integers(32, 121))])), len(rec) - 8)
    forward = bool(rng.random() < 0.5)                       # the anchor on strand 0, the target right of it -- or the mirror image
    if flavour == "copy":
        a0, b0, n = gene["tandem"]
        lt = min(lt, n)
        x = a0 + int(rng.integers(0, n - lt + 1))
        a = max(0, x - 120) if forward else min(len(rec) - la, x + 80)
    else:
        a = int(rng.integers(0, len(rec) - la + 1))
        if forward:
            lo, hi = max(a, a + la - lt), min(a + max_frag - lt, len(rec) - lt)
        else:
            lo, hi = max(a + la - max_frag, 0), min(a, a + la - lt, len(rec) - lt)
        if flavour == "far":
            lo, hi = (hi + 1, len(rec) - lt) if forward else (0, lo - 1)
        x = int(rng.integers(lo, hi + 1)) if hi >= lo else a
        x = min(max(x, 0), len(rec) - lt)                        # (a max_frag below the target's length puts the window's end left of the record)
    at = silencing(lt, k, s_min)
    if flavour == "heavy":
        at = sorted(set(at) | set(range(1, lt, 4)))
    if at and rng.random() < 0.3:
        at = at + [p for p in (int(rng.integers(0, lt)),) if p not in at]     # one more: costs around max_cost
    target = substituted(rec[x:x + lt], at)
    anchor = rec[a:a + la].copy()
    return (anchor, synth.revcomp(target)) if forward else (synth.revcomp(anchor), target)


def draw_mates(rng, panel, long, n, k, s_min, max_frag, weights, sub):
    """(mates 1, mates 2, the classes drawn)"""
    kinds = [c for c in CLASSES if weights.get(c, 0) > 0]
    p = np.array([weights[c] for c in kinds], dtype=np.float64)
    p /= p.sum()
    m1s, m2s, seen = [], [], set()
    for _ in range(n):
        gene = panel[int(rng.integers(0, len(panel)))]
        kind = [str(c) for c in rng.choice(kinds, size=2, p=p)]
        if "silenced" in kind:
            mates = list(silenced_pair(rng, gene, long, k, s_min, max_frag))
            seen.add("silenced")
        else:
            mates = [one_mate(rng, c, gene, long, k) for c in kind]
            seen.update(kind)
            if rng.random() < 0.5 and kind[0] == kind[1] == "transcript":
                # a proper pair: mate 2 downstream of mate 1 on the other strand
                tr = gene["tr"]
                l1, l2 = (min(len(m), len(tr) - 8) for m in mates)
                a = int(rng.integers(0, len(tr) - l1 + 1))
                b = int(rng.integers(a, max(a, len(tr) - l2) + 1))
                mates = [tr[a:a + l1].copy(), synth.revcomp(tr[b:b + l2])]
            for t in range(2):
                s = rng.random(len(mates[t])) < sub
                mates[t][s] = synth.ACGT[rng.integers(0, 4, size=int(s.sum()))]
            if rng.random() < 0.5:
                mates = [synth.revcomp(m) for m in mates]
        if rng.random() < 0.5:
            mates.reverse()
        m1s.append(mates[0])
        m2s.append(mates[1])
    return m1s, m2s, seen


def spoil(rng, m, n_rate, other_rate, lower_rate):
    if len(m) == 0:
        return m
    m = m.copy()
    m[(m < 0x41) | (m > 0x7A)] = ord("N")                     # (a record's '-' under a mate: a letter in the read)
    m[rng.random(len(m)) < n_rate] = ord("N")
    u = rng.random(len(m)) < other_rate
    m[u] = LETTERS[rng.integers(0, len(LETTERS), size=int(u.sum()))]
    m[rng.random(len(m)) < lower_rate] |= 0x20
    return m


def qualities(rng, m):
    q = np.where(rng.random(len(m)) < 0.9, rng.integers(20, 42, size=len(m)), rng.integers(2, 20, size=len(m)))
    return (q + 33).astype(np.uint8)


# ---------------------------------------------------------------------------
# the site list of spliced ends
# ---------------------------------------------------------------------------
def draw_sites(rng, panel_of_record, lengths, crowded):
    """true introns, their microhomology-shifted duplicates, shifted wrong neighbours, decoys anywhere in the record and -- crowded --
    more than 64 sites whose donors fall into one end's range and as many whose acceptors do"""
    sites = set()
    for g, gene in enumerate(panel_of_record):
        if gene is None:
            continue
        n = lengths[g]
        for d, a, same in gene["introns"]:
            sites.add((g, d, a))
            for s in range(1, same + 1):
                sites.add((g, d + s, a + s))
            if rng.random() < 0.3:
                s = int(rng.choice([-3, -2, -1, 1, 2, 3]))
                sites.add((g, d + s, a + s))
            if rng.random() < 0.3:
                sites.add((g, d, a + int(rng.integers(1, 30))))                 # a competing acceptor
            if rng.random() < 0.3:
                sites.add((g, d + int(rng.integers(-16, 48)), a + int(rng.integers(-47, 17))))     # a decoy inside both search ranges
        for _ in range(int(rng.integers(0, 6))):
            d = int(rng.integers(1, n - 2))
            sites.add((g, d, d + int(rng.integers(1, 200))))
        if crowded and gene["introns"]:
            d0, a0, _ = gene["introns"][int(rng.integers(0, len(gene["introns"])))]
            for t in range(-16, 60):
                sites.add((g, d0 + t, a0 + (t * 7) % 23))
                sites.add((g, d0 - (t * 5) % 19, a0 - t))
    ok = sorted((g, d, a) for g, d, a in sites if 1 <= d < a <= lengths[g] - 1)
    return check_sites(ok, lengths)


# ---------------------------------------------------------------------------
# draw
# ---------------------------------------------------------------------------
def draw_indels(rng, md, panel, forced):
    """indels mode's (floor, min_intron), or None: off in one case of five.  From a stream of its own, which every case consumes alike.
    The floor: alignments mode's (one align_kernel launch serves both); aligned pileup's where that is another (the accumulating launch
    serves nobody else: a second storing one); another one (with aligned pileup at a third floor: three launches in one tail, two of them
    storing); one of its own without alignments mode (the context's private array is the only record array).  min_intron: 1 (no
    deletion at all), 2, 3, the CLI's 20, 65 535 (every intron a deletion) and an intron's length of this panel or one more: a gap of
    exactly min_intron is nothing, one of min_intron - 1 a deletion.  forced (the wide and the overflow case): on, at a floor whose
    records the models compute anyway"""
    al_floor = md["al_floor"]
    pile_floor = md["pileup"][1] if md["pileup"][0] == "aligned" else 0
    introns = [a - d for g in panel for d, a, _ in g["introns"]]
    edge = introns[int(rng.integers(0, len(introns)))] + int(rng.integers(0, 2)) if introns else 20
    min_intron = int(rng.choice([1, 2, 3, 20, 20, 65535, edge, edge]))
    off, v, own = rng.random() < 0.2, rng.random(), int(rng.choice(FLOORS))
    others = [f for f in FLOORS if f not in (al_floor, pile_floor)]
    other = others[int(rng.integers(0, len(others)))]
    if forced:
        return (al_floor or pile_floor or own, 20 if min_intron == 1 else min_intron)
    if off:
        return None
    if not al_floor:
        return (own, min_intron)
    if v < 0.4:
        return (al_floor, min_intron)
    if v < 0.6 and pile_floor and pile_floor != al_floor:
        return (pile_floor, min_intron)
    return (other, min_intron)


def draw(seed, bias=""):
    """a case: a dict of plain Python numbers, lists and numpy arrays, deterministic in (seed, bias)"""
    rng = np.random.default_rng([int(seed), BIAS_KEY[bias]])
    wide = bias == "wide"
    k = int(rng.choice(KS))
    # ---- the reference
    n_genes = 2 if wide else int(rng.integers(1, 5))
    hostile = float(rng.choice([0.0, 0.0, 0.02])) if not wide else 0.0
    if bias == "indel":
        panel = [indel_gene(rng, int(rng.integers(0, 4)), k + max(FLOORS) + 3, hostile) for _ in range(n_genes)]
    else:
        panel = [spliced_gene(rng, int(rng.integers(1 if wide else 0, 5)), k, hostile) for _ in range(n_genes)]
    twins = 0
    if bias == "tie" or (not wide and rng.random() < 0.25):
        twins = 6 if (bias == "tie" and rng.random() < 0.5) else int(rng.integers(2, 7))
    overflow = bias == "tie" and twins == 6 and rng.random() < 0.2
    if overflow:
        panel = panel[:1]
    genes_of_record = [panel[0]] * max(twins, 1) + panel[1:]
    want_long = not wide and not overflow and rng.random() < (0.5 if bias == "rescue" else 0.3)
    long = long_gene(rng) if want_long else None
    if long is not None:
        genes_of_record.append(long)
    records = [g["rec"] for g in genes_of_record]
    if not wide and rng.random() < 0.2:
        records.append(synth.random_seq(rng, int(rng.integers(max(k, 20), 64))))      # a record shorter than 64 bases
        genes_of_record.append(None)
    lengths = [len(r) for r in records]
    # ---- the modes
    al_floor = int(rng.choice(FLOORS))
    if long is not None and rng.random() < 0.3:
        al_floor = 40
    md = dict(evidence=not wide, cand_m=0 if wide else int(rng.integers(1, SHK_MAX_CANDIDATES + 1)), placement=True,
              seg_m=4 if wide else int(rng.integers(1, 5)))
    md["depth"] = None if wide else (("plain", int(rng.choice([1, 3, 8]))) if rng.random() < 0.5 else ("spliced", int(rng.choice([1, 3, 6, 8, 12]))))
    md["junc_floor"] = 0 if wide else int(rng.choice([1, 3, 8]))
    u = rng.random()
    if wide or u < 0.3:
        md["pileup"] = ("owned", int(rng.choice([1, 3, 8])))
    elif u < 0.55:
        md["pileup"] = ("aligned", al_floor)
    elif u < 0.8:
        md["pileup"] = ("aligned", int(rng.choice([f for f in (1, 3, 6, 8, 12) if f != al_floor])))
    else:
        md["pileup"] = ("aligned", al_floor)
        al_floor = 0                                             # aligned pileup without alignments mode: no records are stored
    md["al_floor"] = al_floor
    md["ext"] = (0, 0) if (not wide and rng.random() < 0.45) else (int(rng.integers(1, 16)), int(rng.integers(0, 16)))
    if wide:
        md["ext"] = (4, 5)
    splice_on = wide or bias == "splice" or rng.random() < 0.6
    md["splice"] = None
    if splice_on:
        h = int(rng.choice([1, 2, 3, 3, 8, 20, 48, int(rng.integers(1, 49))]))
        md["splice"] = (h, int(rng.integers(0, 9)), int(rng.integers(0, 7)))
        if bias == "splice" and rng.random() < 0.3:
            md["splice"] = (h, int(rng.choice([2, 8, 64])), int(rng.choice([0, 1, 2])))
    sites = draw_sites(rng, genes_of_record, lengths, crowded=bool(rng.random() < (0.3 if bias == "splice" else 0.1))) if splice_on else []
    if not sites:
        md["splice"] = None
    small = bias == "rescue" and rng.random() < 0.5
    md["pairs"] = md["rescue"] = None
    if al_floor and not wide:
        md["pairs"] = (int(rng.choice([1, 20, 30, 1000])), int(rng.choice([1, 50, 300, 611, 1000, 4096, 100000])), int(rng.choice([2, 64, 1024, 4096])))
        md["rescue"] = (int(rng.choice([1, 20, 30])), int(rng.choice([1, 40, 90, 200] if small else [1, 90, 200, 611, 1000, 4096])),
                        int(rng.choice([0, 1, 2, 4, 8, 8, 16, 255])), int(rng.choice([0, 1, 4, 4, 255])))
    md["indels"] = draw_indels(np.random.default_rng([int(seed), BIAS_KEY[bias], 1]), md, panel, forced=wide or overflow)
    # ---- the batch
    paired = True if wide else bool(rng.random() < 0.8)
    n = WIDE_A_PAIRS if wide else (1520 if overflow else int(rng.choice([1, 63, 64, 65, 200, 200, 300, 300])))
    q = 0 if wide else int(rng.choice([0, 0, 0, 0, 2, 20, 20, 35]))
    weights = dict(transcript=0.42, record=0.08, deleted=0.05, repeated=0.05, random=0.04, insertion=0.10, empty=0.02, short=0.03, exact_k=0.03,
                   long=0.06 if long is not None else 0.0, silenced=0.12 if paired else 0.0)
    if bias == "rescue":
        weights["silenced"] = 0.45 if paired else 0.0
    if bias == "splice":
        weights["transcript"] = 0.6
    if bias == "indel":
        weights["indel"] = 0.8
    if wide or overflow:
        weights = dict(transcript=0.85, record=0.05, deleted=0.05, insertion=0.05)
    s_floor = al_floor or md["pileup"][1]
    max_frag = md["rescue"][1] if md["rescue"] else 1000
    sub = float(rng.choice([0.0, 0.01, 0.03]))
    first_trip = PL_MAX_BLOCKS * PL_WAVES
    m1s, m2s, classes = draw_mates(rng, panel[:1] if overflow else panel, long, min(n, first_trip) if wide else n, k, s_floor, max_frag, weights, sub)
    if wide:
        # the reads of the second trip: mates that no read of the first trip holds, so no kernel can pass by handing out an earlier read's result
        m1s, m2s = [m[:100] for m in m1s], [m[:100] for m in m2s]
        held = {bytes(m) for m in m1s + m2s}
        while len(m1s) < n:
            a, b, _ = draw_mates(rng, panel, long, 1, k, s_floor, max_frag, weights, max(sub, 0.01))
            a, b = a[0][:100], b[0][:100]
            if bytes(a) not in held and bytes(b) not in held:
                m1s.append(a)
                m2s.append(b)
                held.update((bytes(a), bytes(b)))
    n_rate = 0.0 if wide else float(rng.choice([0.0, 0.002, 0.05]))
    other = 0.0 if wide else float(rng.choice([0.0, 0.0, 0.005]))
    lower = 0.0 if wide else float(rng.choice([0.0, 0.0, 0.1]))
    m1s = [spoil(rng, m, n_rate, other, lower) for m in m1s]
    m2s = [spoil(rng, m, n_rate, other, lower) for m in m2s]
    for lst in (m1s, m2s):
        if not sum(len(m) for m in lst):
            lst[0] = synth.random_seq(rng, 30)                  # (no batch whose sequence array is empty)
    q1 = [qualities(rng, m) for m in m1s] if q else None
    q2 = [qualities(rng, m) for m in m2s] if q else None
    batch = synth.batch_from_lists(m1s, m2s if paired else None, q1, q2 if paired else None)
    longest = max(max(len(m) for m in m1s), max(len(m) for m in m2s) if paired else 0)
    # ---- the entry family
    family = "classify" if wide else str(rng.choice(FAMILIES))
    bound = 0
    if family == "classify_device":
        bound = int(rng.choice([longest, 0, max(1, longest // 3)]))
    elif family == "submit_device":
        bound = min(int(rng.choice([longest, longest, max(1, longest // 3)])), largest_submit_bound(k, paired))
    return dict(seed=int(seed), bias=bias, k=k, c=0.0, min_quality=q, records=records, lengths=lengths, twins=twins, has_long=long is not None,
                intron_lengths=[sorted({a - d for d, a, _ in g["introns"]}) if g else [] for g in genes_of_record],
                modes=md, sites=sites, paired=paired, n=n, batch=batch, classes=sorted(classes), longest=longest, family=family, bound=bound,
                times=2 if family in ("submit", "submit_device") else 1)


def variant(case, **changes):
    """the case with some of its modes replaced (wide case (a): aligned pileup on a second context, the same batch single-end)"""
    out = dict(case)
    out["modes"] = dict(case["modes"])
    for key, v in changes.items():
        if key == "single_end":
            b = dict(case["batch"])
            b["seq2"] = b["off2"] = b["qual2"] = None
            out["batch"], out["paired"] = b, False
        else:
            out["modes"][key] = v
    return out


def emptied_from(batch, keep):
    """the batch with every mate of the pairs from `keep` on empty: as many reads, fewer associations"""
    out = dict(batch)
    for m in ("1", "2"):
        if batch["seq" + m] is None:
            continue
        off = batch["off" + m].copy()
        off[keep:] = off[keep]
        out["off" + m] = off
        for part in ("seq", "qual"):
            if batch[part + m] is not None:
                out[part + m] = batch[part + m][:int(off[keep])].copy()
    return out


def describe(case):
    md = case["modes"]
    return "seed=%d bias=%s k=%d records=%d twins=%d n=%d%s q=%d %s bound=%d/%d seg=%d cand=%d depth=%s junc=%d pileup=%s al=%d ext=%s splice=%s sites=%d pairs=%s rescue=%s indels=%s" % (
        case["seed"], case["bias"] or "-", case["k"], len(case["records"]), case["twins"], case["n"], "x2" if case["paired"] else "", case["min_quality"],
        case["family"], case["bound"], case["longest"], md["seg_m"], md["cand_m"], md["depth"], md["junc_floor"], md["pileup"], md["al_floor"], md["ext"],
        md["splice"], len(case["sites"]), md["pairs"], md["rescue"], md["indels"])


# ---------------------------------------------------------------------------
# expected
# ---------------------------------------------------------------------------
def _bump(cov, key, by=1):
    if by:
        cov[key] = cov.get(key, 0) + int(by)


def indel_coverage(cov, case, records, goff, gids, gene_records, stats):
    """what indels mode's model met in the case: tests/indels_model.py's record_events once more, record by record, for the facts that
    its table does not keep (an event's shift, whether its read was tied, what -q did to an insertion)"""
    q, min_intron = case["min_quality"], case["modes"]["indels"][1]
    for name in INDEL_COUNTERS:
        _bump(cov, "indels." + name, stats[name])
    _bump(cov, "indels.single_end", not case["paired"] and stats["mates"] > 0)
    largest = 0
    plain = list(masked_mates(case["batch"], 0)) if q else None
    for i, pair in enumerate(masked_mates(case["batch"], q)):
        for j in range(int(goff[i]), int(goff[i + 1])):
            g = int(gids[j])
            for t, mate in enumerate(pair):
                rec = records[j, t]
                n = int(rec["n_blocks"])
                if mate is None or n < 2:
                    continue
                st, shifts = new_stats(), []
                events = record_events(rec, mate, gene_records.get(g, b""), min_intron, st, shifts)
                for (x, kind, length, seq), d in zip(events, shifts):
                    _bump(cov, "indels.rev" if int(rec["strand"]) & 1 else "indels.fwd")
                    _bump(cov, "indels.shift_ge_1", d >= 1)
                    _bump(cov, "indels.shift_over_len", kind == 1 and d > length)
                    _bump(cov, "indels.tied", int(goff[i + 1]) - int(goff[i]) >= 2)
                    _bump(cov, "indels.intron_as_deletion", kind == 0 and length >= 30 and length in case["intron_lengths"][g])
                    largest = max(largest, d)
                if q and st["nonbase_insertions"]:
                    clear = new_stats()
                    record_events(rec, plain[i][t], gene_records.get(g, b""), min_intron, clear)
                    _bump(cov, "indels.masked", st["nonbase_insertions"] - clear["nonbase_insertions"])
                b = rec["block"]
                for r in range(n - 1):
                    R = int(b[r + 1][1]) - int(b[r][1]) - int(b[r][2])
                    G = int(b[r + 1][0]) - int(b[r][0]) - int(b[r][2])
                    _bump(cov, "indels.gap_eq_min_intron", R == 0 and G == min_intron)
    cov["indels.largest_shift"] = largest


def expected(case, oracle, candidates=ranged_candidates, scorer=best_extension, memo=None, primed=True):
    """every record array and accumulator state of the case, from the oracle's associations and the models; states are those after
    case["times"] counted batches (the ticket families submit the batch twice).  `coverage` counts what the case exercised.  memo: a
    dict shared by variants of ONE case over the SAME batch (variant() with other modes): associations, placements, segments and the
    alignment records per floor are then computed once.  primed=False (tests/fuzz_sessions.py: the batch comes behind others through a
    live context, whose arrays hold those batches' records) leaves the overflow case's primer out: the states are the batch's own"""
    memo = {} if memo is None else memo

    def once(key, fn):
        if key not in memo:
            memo[key] = fn()
        return memo[key]

    k, q, md, batch = case["k"], case["min_quality"], case["modes"], case["batch"]
    times = case["times"]
    recs = [bytes(r) for r in case["records"]]
    o = oracle.Shark(k=k, c=case["c"], bf_bits=BF_BITS, min_quality=q)
    nidx = o.build(recs)
    sm = SegmentsModel(recs, k)
    goff, gids = once("genes", lambda: tuple(np.asarray(a) for a in o.classify(*_args(batch))))
    n_assoc = int(goff[-1])
    gs = model_layout(sm, nidx)
    out = dict(goff=goff, gids=gids, nidx=nidx, gene_start=gs)
    cov = {}
    out["coverage"] = cov
    _bump(cov, "k.%d" % k)
    _bump(cov, "family." + case["family"])
    _bump(cov, "seg_m.%d" % md["seg_m"])
    _bump(cov, "single_end", not case["paired"])
    _bump(cov, "masked", q > 0)
    for c in case["classes"]:
        _bump(cov, "class." + c)
    widths = np.diff(goff.astype(np.int64)) if len(goff) > 1 else np.zeros(0, np.int64)
    _bump(cov, "tie.2", (widths == 2).any())
    _bump(cov, "tie.over_inline", (widths > SHK_INLINE_IDS).any())
    cov["widest"] = int(widths.max()) if len(widths) else 0
    overflow = n_assoc > slot_reserve(case["n"])
    too_long = case["family"] in ("classify_device", "submit_device") and 0 < case["bound"] < case["longest"]
    _bump(cov, "repair.overflow", overflow)
    _bump(cov, "repair.length", too_long)
    _bump(cov, "repair.length.submit_device", too_long and case["family"] == "submit_device")
    out["expect_overflow"], out["expect_long"] = overflow, too_long
    if md["evidence"]:
        out["evidence"] = expected_evidence(o, batch)
    if md["cand_m"]:
        out["candidates"] = expected_candidates(o, batch, md["cand_m"])
    if md["placement"]:
        out["placement"] = once("placement", lambda: expected_placements(sm, batch, goff, gids, q))
    keys4, rows4 = once("segments", lambda: expected_segments(sm, batch, goff, gids, 4, q))
    out["segments"] = (keys4, rows4) if md["seg_m"] == 4 else expected_segments(sm, batch, goff, gids, md["seg_m"], q)
    # ---- alignments: steps 1 .. 3, 3b, 3a, 4; rescue behind them; pairs behind rescue
    P, B = md["ext"]
    params = md["splice"] or (0, 0, 0)
    sites = case["sites"] if md["splice"] else []
    ext, spl = int(P > 0), int(bool(md["splice"]))

    def counted(side, sites_g, x, qq, ln, L, len_g):
        got = candidates(side, sites_g, x, qq, ln, L, len_g)
        _bump(cov, "splice.range_over_64", len(got) > 64)
        return got

    def deciding(kinds, to_end, p, b):
        e = scorer(kinds, to_end, p, b)
        _bump(cov, "ext.bonus_decided", to_end and e != scorer(kinds, to_end, p, 0))
        return e

    def records_at(floor, tally):
        key = ("records", floor, P, B, params, len(sites))
        if key in memo:
            return memo[key]
        st, xs, als, gaps = {}, {}, {}, []
        r = expected_alignments_spliced(sm, batch, goff, gids, rows4, floor, sites, params, P, B, q, st if tally else None,
                                        counted if tally else candidates, deciding if tally else scorer, xs if tally else None,
                                        als if tally else None, gaps if tally else None)
        if tally:
            for key in ("trimmed", "closed", "open_insertion", "open_wide", "dropped"):
                _bump(cov, "align." + key, als.get(key, 0))
            _bump(cov, "align.closed_r64", sum(1 for R, G, closed in gaps if closed and R == 64))
            _bump(cov, "align.open_r65", sum(1 for R, G, closed in gaps if not closed and R >= 65))
            for key in ("left", "right"):
                _bump(cov, "ext." + key, xs.get(key, 0))
            for key, v in st.items():
                _bump(cov, "splice." + key, v)
                for what in ("ambiguous", "too_costly", "no_candidate"):
                    if key.endswith(what):
                        _bump(cov, "splice.any_" + what, v)
            nb = r["n_blocks"].reshape(-1)
            for b in range(1, 5):
                _bump(cov, "n_blocks.%d" % b, int((nb == b).sum()))
            for s in range(2):
                _bump(cov, "strand.%d" % s, int(((nb > 0) & (r["strand"].reshape(-1) == s)).sum()))
        memo[key] = r
        return r

    kind, floor = md["pileup"] if md["pileup"] else (None, 0)
    al = None
    if md["al_floor"]:
        al = records_at(md["al_floor"], True)
        _bump(cov, "inst.%d%d%d.stored" % (ext, int(kind == "aligned" and floor == md["al_floor"]), spl))
        before = al
        if md["rescue"]:
            al, rs = expected_rescue(before, batch, goff, gids, dict(sm.records), *md["rescue"], min_quality=q)
            out["rescue"] = rs
            for s, c in enumerate(np.bincount(rs["state"], minlength=6)[:6]):
                _bump(cov, "rescue.state%d" % s, c)
        out["alignments"] = al
        if md["pairs"]:
            pr = expected_pairs(al, batch, goff, md["pairs"][0], md["pairs"][1])
            out["pairs"] = pr
            hist, classes = Fragments(md["pairs"][2]).add(pr, goff).arrays()
            out["fragments"] = (hist * np.uint64(times), classes * np.uint64(times))
            for s, c in enumerate(np.bincount(pr["cls"], minlength=6)[:6]):
                _bump(cov, "pairs.cls%d" % s, c)
    # ---- the accumulators
    if md["depth"]:
        if md["depth"][0] == "plain":
            d, m = expected_depth(sm, batch, goff, gids, md["depth"][1], q)
        else:
            d, m = expected_spliced_depth(sm, batch, goff, gids, rows4, md["depth"][1])
        out["depth"] = (d * np.uint32(times), m * times)
    if md["junc_floor"]:
        out["junctions"] = [(g, d, a, i, n * times) for g, d, a, i, n in table_rows(expected_junction_table(batch, goff, gids, rows4, k, md["junc_floor"]))]
    if kind == "owned":
        counts, lost, mates = expected_pileup(sm, batch, goff, gids, rows4, floor, q)
        out["pileup_lost"] = lost
    elif kind == "aligned":
        if floor == md["al_floor"]:
            pile_records = before                                # (a rescued mate does not enter the pileup)
        else:
            pile_records = records_at(floor, md["al_floor"] == 0)
            _bump(cov, "inst.%d1%d.unstored" % (ext, spl))
            _bump(cov, "pileup.other_floor", md["al_floor"] != 0)
        counts, mates, bearing = expected_aligned_pileup(sm, batch, goff, gids, pile_records, q)
        out["pileup_records"], out["bearing"] = pile_records, bearing * times
    if kind:
        counts = counts * np.uint32(times)
        out["pileup"] = (counts, mates * times)
        out["variants"] = [(expected_variants(counts, sm.records, gs, prm), expected_summary(counts, sm.records, gs, prm)) for prm in VARIANT_PARAMS]
        _bump(cov, "variant_site", len(out["variants"][0][0]) > 0 or len(out["variants"][1][0]) > 0)
    # ---- indels: align_kernel's records at the mode's own floor, BEFORE rescue rewrites them
    if md["indels"]:
        floor, min_intron = md["indels"]
        recs_i = before if floor == md["al_floor"] else records_at(floor, False)
        table, stats = expected_indels(recs_i, batch, goff, gids, sm.records, min_intron, q)
        arr = table_array(table)
        arr["fwd"] *= np.uint32(times)
        arr["rev"] *= np.uint32(times)
        out["indels"] = (arr, {name: v * times for name, v in stats.items()})
        if overflow and primed:
            # The overflow repair: the tail's first pass must count nothing.  Its kernels return early, so the record arrays hold what
            # was there before -- in a fresh context nothing in particular.  So this case is PRIMED: the same reads go through the
            # context first with the last ones emptied until the associations fit (the same n: no array is allocated anew), indels
            # mode and the record modes on, every other accumulator off.  The arrays then hold valid records of this very batch's
            # first reads when the overflowing batch's first pass comes by -- in EVERY slot: a context hands its SHK_PIPE_DEPTH
            # slots out in turn, so the primer goes through as often.  A read's associations and records are its own, so the
            # primer's state is the model's over the same records with the emptied reads' associations gone
            keep = int(np.searchsorted(goff, slot_reserve(case["n"]) * 3 // 4, side="right")) - 1
            pgoff = goff.copy()
            pgoff[keep:] = goff[keep]
            primer = emptied_from(batch, keep)
            ptab, pst = expected_indels(recs_i, primer, pgoff, gids, sm.records, min_intron, q)
            D = capi.SHK_PIPE_DEPTH
            both = {key: [f * times + D * ptab.get(key, (0, 0))[0], r * times + D * ptab.get(key, (0, 0))[1]] for key, (f, r) in table.items()}
            assert set(ptab) <= set(table)
            out["indels"] = (table_array(both), {name: v * times + D * pst[name] for name, v in stats.items()})
            out["primer"] = dict(batch=primer, goff=pgoff.astype(np.uint32), gids=gids[:int(pgoff[-1])].astype(np.uint16))
            assert 0 < pst["deletions"] + pst["insertions"] and 0 < int(pgoff[-1]) <= slot_reserve(case["n"])
        out["indel_records"] = recs_i
        indel_coverage(cov, case, recs_i, goff, gids, sm.records, stats)
        _bump(cov, "indels.floor_same" if floor == md["al_floor"] else "indels.without_alignments" if not md["al_floor"] else "indels.floor_other")
        _bump(cov, "indels.third_launch", kind == "aligned" and len({floor, md["pileup"][1], md["al_floor"]}) == 3 and md["al_floor"] > 0)
        _bump(cov, "indels.before_rescue", bool(md["rescue"]) and floor == md["al_floor"] and al.tobytes() != before.tobytes())
        _bump(cov, "indels.with_overflow", overflow)
        _bump(cov, "indels.with_length_repair", too_long)
        _bump(cov, "indels.with_length_repair.submit_device", too_long and case["family"] == "submit_device")
    out["expect_indels"] = bool(md["indels"])
    out["stored"] = bool(md["al_floor"])
    out["model"], out["rows4"], out["before_rescue"] = sm, rows4, (before if md["al_floor"] else None)
    cov["instantiation"] = (ext, int(kind == "aligned"), spl)
    cov["entry"] = case["family"]
    o.close()
    return out


# ---------------------------------------------------------------------------
# run
# ---------------------------------------------------------------------------
def first_difference(kind, got, want):
    """None, or what differs: the kind and the first differing record as the device and the model each see it"""
    got, want = np.asarray(got), np.asarray(want)
    if got.dtype != want.dtype or got.shape != want.shape:
        return "%s: dtype / shape %s %s, model %s %s" % (kind, got.dtype, got.shape, want.dtype, want.shape)
    if got.tobytes() == want.tobytes():
        return None
    if got.ndim == 0:
        return "%s: got %s, model %s" % (kind, got, want)
    bad = [j for j in range(len(want)) if got[j].tobytes() != want[j].tobytes()]
    j = bad[0]
    return "%s: record %d: got %s, model %s (%d of %d records differ)" % (kind, j, got[j].tolist(), want[j].tolist(), len(bad), len(want))


def set_modes(h, case):
    md = case["modes"]
    h.evidence_enable(md["evidence"])
    h.candidates_enable(md["cand_m"])
    h.placement_enable(md["placement"])
    h.segments_enable(md["seg_m"])
    if md["depth"]:
        (h.depth_enable if md["depth"][0] == "plain" else h.depth_enable_spliced)(md["depth"][1])
    if md["junc_floor"]:
        h.junctions_enable(md["junc_floor"], JUNCTION_CAPACITY)
    if md["pileup"]:
        (h.pileup_enable if md["pileup"][0] == "owned" else h.pileup_enable_aligned)(md["pileup"][1])
    h.alignments_enable(md["al_floor"])
    h.alignments_extend(*md["ext"])
    if md["splice"]:
        h.splice_sites_set(np.array(case["sites"], dtype=np.int64).reshape(-1, 3))
        h.alignments_splice(*md["splice"])
    if md["pairs"]:
        h.pairs_enable(*md["pairs"])
    if md["rescue"]:
        h.rescue_enable(*md["rescue"])
    if md["indels"]:
        h.indels_enable(md["indels"][0], md["indels"][1], JUNCTION_CAPACITY)


def build_context(case, oracle_nidx):
    """the context the way tests/test_gpu_variants.py's build_kb makes it: the record bases kept (which implies the positions)"""
    from shark_amd import SharkHip
    h = SharkHip(k=case["k"], c=case["c"], bf_bits=BF_BITS, min_quality=case["min_quality"])
    info = h.build([bytes(r) for r in case["records"]], keep_positions=False, keep_bases=True)
    assert info["nidx"] == oracle_nidx, (info["nidx"], oracle_nidx)
    return h


def host_records(h, md):
    rec = {}
    if md["evidence"]:
        rec["evidence"] = h.evidence_last()
    if md["cand_m"]:
        rec["candidate reads"], rec["candidate entries"] = h.candidates_last()
    if md["placement"]:
        rec["placement"] = h.placement_last()
    rec["segment keys"], rec["segment entries"] = h.segments_last()
    if md["al_floor"]:
        rec["alignments"] = h.alignments_last()
        if md["rescue"]:
            rec["rescue"] = h.rescue_last()
        if md["pairs"]:
            rec["pairs"] = h.pairs_last()
    return rec


def device_records(h, md, r):
    """the resident batch's associations and records, read back through the capi.*_from_device helpers"""
    n, tot = int(r.n), int(r.n_assoc)
    goff, gids = np.zeros(n + 1, np.uint32), np.zeros(tot, np.uint16)
    capi.hip_memcpy_dtoh(goff, r.gene_off, goff.nbytes)
    if tot:
        capi.hip_memcpy_dtoh(gids, r.gene_ids, gids.nbytes)
    rec = {}
    if md["evidence"]:
        ev = np.zeros((n, 3), np.uint32)
        capi.hip_memcpy_dtoh(ev, h.evidence_last(), ev.nbytes)
        rec["evidence"] = ev
    if md["cand_m"]:
        cn, cm, rp, ep = h.candidates_last()
        assert (cn, cm) == (n, md["cand_m"])
        reads, entries = np.zeros((n, 2), np.uint32), np.zeros((n, cm, 3), np.uint32)
        capi.hip_memcpy_dtoh(reads, rp, reads.nbytes)
        capi.hip_memcpy_dtoh(entries, ep, entries.nbytes)
        rec["candidate reads"], rec["candidate entries"] = reads, entries
    na, m, kp, ep = h.segments_last()
    assert na == tot and m == md["seg_m"]
    rec["segment keys"], rec["segment entries"] = capi.segments_from_device(na, m, kp, ep)
    kinds = [("placement", md["placement"], h.placement_last, capi.placements_from_device),
             ("alignments", md["al_floor"], h.alignments_last, capi.alignments_from_device),
             ("rescue", md["al_floor"] and md["rescue"], h.rescue_last, capi.rescues_from_device),
             ("pairs", md["al_floor"] and md["pairs"], h.pairs_last, capi.pairs_from_device)]
    for name, on, last, read in kinds:
        if on:
            na, ptr = last()
            assert na == tot, name
            rec[name] = read(na, ptr)
    return goff, gids, rec


def compare_records(got, want, goff, gids):
    """the first difference between one hand-out's records and the model's, or None"""
    bad = first_difference("gene_off", goff, want["goff"].astype(np.uint32)) or first_difference("gene_ids", gids, want["gids"].astype(np.uint16))
    if bad:
        return bad + " (against the oracle)"
    pairs = [("evidence", "evidence"), ("placement", "placement"), ("alignments", "alignments"), ("rescue", "rescue"), ("pairs", "pairs")]
    for kind, key in pairs:
        if kind in got:
            bad = first_difference(kind, got[kind], want[key])
            if bad:
                return bad
    if "candidate reads" in got:
        bad = first_difference("candidate reads", got["candidate reads"], want["candidates"][0]) or \
            first_difference("candidate entries", got["candidate entries"], want["candidates"][1])
        if bad:
            return bad
    return first_difference("segment keys", got["segment keys"], want["segments"][0]) or first_difference("segment entries", got["segment entries"], want["segments"][1])


def compare_states(h, case, want):
    md = case["modes"]
    if md["depth"]:
        bad = first_difference("depth", h.depth_all(), want["depth"][0]) or first_difference("depth mates", np.uint64(h.depth_mates()), np.uint64(want["depth"][1]))
        if bad:
            return bad
    if md["junc_floor"]:
        got = [tuple(int(v) for v in r) for r in h.junctions_get()]
        if got != want["junctions"]:
            j = next((i for i, (a, b) in enumerate(zip(got, want["junctions"])) if a != b), min(len(got), len(want["junctions"])))
            return "junction table: row %d: got %s, model %s (%d rows, model %d)" % (j, got[j:j + 1], want["junctions"][j:j + 1], len(got), len(want["junctions"]))
    if md["pileup"]:
        bad = first_difference("pileup", h.pileup_all(), want["pileup"][0]) or first_difference("pileup mates", np.uint64(h.pileup_mates()), np.uint64(want["pileup"][1]))
        if bad:
            return bad
        for prm, (sites, summary) in zip(VARIANT_PARAMS, want["variants"]):
            bad = first_difference("variants %s" % (prm,), h.variants(prm[0], prm[1], (prm[2], prm[3])), sites) or \
                first_difference("variants summary %s" % (prm,), h.variants_summary(prm[0], prm[1], (prm[2], prm[3])), summary)
            if bad:
                return bad
    if md["al_floor"] and md["pairs"]:
        hist, classes = h.fragments(md["pairs"][2])
        bad = first_difference("fragment classes", classes, want["fragments"][1]) or first_difference("fragment histogram", hist, want["fragments"][0])
        if bad:
            return bad
    if md["indels"]:
        stats = h.indels_stats()
        bad = compare_indels(None if stats["dropped"] else h.indels_get(0), stats, want["indels"])
        if bad:
            return bad
    return first_difference("depth layout", h.depth_layout(), want["gene_start"])


def compare_indels(table, stats, want):
    """None, or the first of the seven counters that differs (dropped is 0 in the model: the table is large enough), or the table's first
    differing entry.  The counters first: shk_indels_get refuses while anything was dropped (table None)"""
    for name in capi.INDEL_STAT_NAMES:
        if stats[name] != want[1][name]:
            return "indel counter %s: got %d, model %d" % (name, stats[name], want[1][name])
    assert stats == want[1]
    return first_difference("indel table", table, want[0])


def run(case, oracle, want=None):
    """(None or the mismatch's message, facts about the run: last_kernel, last_n_long, n_assoc, family)"""
    import torch  # noqa: F401  (torch bundles its own HIP runtime: load it BEFORE libsharkhip so one runtime serves both)
    from tests.test_gpu_segments import _dev_ptrs, _to_device
    want = want or expected(case, oracle)
    md, batch, n = case["modes"], case["batch"], case["n"]
    h = build_context(case, want["nidx"])
    replay = "  (replay: python tests/fuzz_records.py 1 %d %s)" % (case["seed"], case["bias"])
    try:
        if want.get("primer"):
            quiet = dict(md, evidence=False, cand_m=0, depth=None, junc_floor=0, pileup=None, pairs=None, rescue=None)
            set_modes(h, dict(case, modes=quiet))
            for _ in range(capi.SHK_PIPE_DEPTH):
                goff, gids = h.classify(*_args(want["primer"]["batch"]))
                bad = first_difference("gene_off", goff, want["primer"]["goff"]) or first_difference("gene_ids", gids, want["primer"]["gids"])
                if bad:
                    return bad + " (the primer, against the oracle)", dict(family=case["family"])
        set_modes(h, case)
        family = case["family"]
        hand_outs = []
        if family == "classify":
            goff, gids = h.classify(*_args(batch))
            hand_outs.append((goff, gids, host_records(h, md)))
        elif family == "submit":
            tickets = [h.submit(*_args(batch)), h.submit(*_args(batch))]        # a second ticket in flight
            for t in tickets:
                goff, gids = h.wait(t)
                hand_outs.append((goff, gids, host_records(h, md)))
        else:
            dev = _to_device(batch)
            ptrs = _dev_ptrs(dev)
            if family == "classify_device":
                hand_outs.append(device_records(h, md, h.classify_device(n, max_read_len=case["bound"], **ptrs)))
            else:
                tickets = [h.submit_device(n, max_read_len=case["bound"], **ptrs), h.submit_device(n, max_read_len=case["bound"], **ptrs)]
                for t in tickets:
                    hand_outs.append(device_records(h, md, h.wait_device(t)))
        facts = dict(last_kernel=h.last_kernel(), last_n_long=int(h.timing()["last_n_long"]), n_assoc=int(hand_outs[-1][0][-1]), family=family)
        for goff, gids, got in hand_outs:
            bad = compare_records(got, want, goff, gids)
            if bad:
                return bad + replay, facts
        bad = compare_states(h, case, want)
        return (bad + replay if bad else None), facts
    finally:
        h.close()


# ---------------------------------------------------------------------------
# wide case (b): the second trip of depth_accumulate_kernel's and spliced_accumulate_kernel's stride loops
# ---------------------------------------------------------------------------
def tiled(block, times, rest):
    """the SoA batch `block` `times` times over, followed by `rest`"""
    out = {"qual1": None, "qual2": None}
    for m in ("1", "2"):
        lens = np.concatenate([np.tile(np.diff(block["off" + m].astype(np.int64)), times), np.diff(rest["off" + m].astype(np.int64))])
        out["seq" + m] = np.concatenate([np.tile(block["seq" + m], times), rest["seq" + m]])
        off = np.zeros(len(lens) + 1, dtype=np.uint64)
        off[1:] = np.cumsum(lens)
        out["off" + m] = off
    return out


def draw_wide_depth(seed):
    """(records, block, remainder) of wide case (b): the block's 1 021 pairs come from the first two genes, the remainder's 836 from the
    third as well.  513 x 1 021 = 523 773, so the second trip -- the 321 reads from 524 288 on -- lies wholly inside the remainder (whose
    first 515 pairs end the first trip) and covers bases that no pair of the block covers"""
    rng = np.random.default_rng([int(seed), WIDE_B_KEY])
    panel = [spliced_gene(rng, 1 + i, 17) for i in range(3)]
    w = dict(transcript=0.8, record=0.1, deleted=0.05, insertion=0.05)
    b1, b2, _ = draw_mates(rng, panel[:2], None, WIDE_B_BLOCK, 17, 8, 1000, w, 0.01)
    r1, r2, _ = draw_mates(rng, panel[2:] * 3 + panel[:2], None, WIDE_B_REST, 17, 8, 1000, w, 0.01)
    return dict(seed=int(seed), k=17, records=[g["rec"] for g in panel], block=synth.batch_from_lists(b1, b2), rest=synth.batch_from_lists(r1, r2),
                longest=max(len(m) for m in b1 + b2 + r1 + r2))


def expected_wide_depth(case, oracle):
    """T x model(block) + model(remainder): depth, spliced depth and the junction table are sums over mates, a mate's contribution
    depends on the mate and its associations alone, so tiling the block T times multiplies its contribution by T -- exactly"""
    T = WIDE_B_TIMES
    recs = [bytes(r) for r in case["records"]]
    o = oracle.Shark(k=17, c=0.0, bf_bits=BF_BITS, min_quality=0)
    nidx = o.build(recs)
    sm = SegmentsModel(recs, 17)
    out = dict(nidx=nidx)
    parts = []
    for b in (case["block"], case["rest"]):
        goff, gids = o.classify(*_args(b))
        rows = expected_segments(sm, b, goff, gids, 4)[1]
        parts.append(dict(goff=np.asarray(goff).astype(np.int64), gids=np.asarray(gids), plain=expected_depth(sm, b, goff, gids, 1),
                          spliced=expected_spliced_depth(sm, b, goff, gids, rows, 8), table=expected_junction_table(b, goff, gids, rows, 17, 8)))
    blk, rest = parts
    out["goff"] = np.concatenate([[0]] + [blk["goff"][1:] + t * blk["goff"][-1] for t in range(T)] + [rest["goff"][1:] + T * blk["goff"][-1]]).astype(np.uint32)
    out["gids"] = np.concatenate([np.tile(blk["gids"], T), rest["gids"]]).astype(np.uint16)
    for kind in ("plain", "spliced"):
        out[kind] = (blk[kind][0] * np.uint32(T) + rest[kind][0], blk[kind][1] * T + rest[kind][1])
    table = {key: [i, n * T] for key, (i, n) in blk["table"].items()}
    for key, (i, n) in rest["table"].items():
        e = table.setdefault(key, [i, 0])
        e[0], e[1] = min(e[0], i), e[1] + n
    out["junctions"] = table_rows(table)
    # non-vacuity: bases that only the reads of the second trip cover (the remainder's last WIDE_B_PAIRS - DEPTH_LANES pairs)
    first = DEPTH_LANES - T * WIDE_B_BLOCK
    b = case["rest"]
    tail = synth.batch_from_lists(*[[b["seq" + m][int(b["off" + m][i]):int(b["off" + m][i + 1])] for i in range(first, WIDE_B_REST)] for m in ("1", "2")])
    goff, gids = o.classify(*_args(tail))
    rows = expected_segments(sm, tail, goff, gids, 4)[1]
    out["rest_only"] = int(((expected_depth(sm, tail, goff, gids, 1)[0] > 0) & (blk["plain"][0] == 0)).sum())
    out["rest_only_spliced"] = int(((expected_spliced_depth(sm, tail, goff, gids, rows, 8)[0] > 0) & (blk["spliced"][0] == 0)).sum())
    o.close()
    return out


def run_wide_depth(case, oracle, want=None):
    """None or the mismatch's message: plain depth on one context, spliced depth and the junction table on another"""
    import torch  # noqa: F401
    from shark_amd import SharkHip
    want = want or expected_wide_depth(case, oracle)
    batch = tiled(case["block"], WIDE_B_TIMES, case["rest"])
    assert len(batch["off1"]) - 1 == WIDE_B_PAIRS > DEPTH_LANES
    for kind in ("plain", "spliced"):
        h = SharkHip(k=17, c=0.0, bf_bits=BF_BITS)
        try:
            assert h.build([bytes(r) for r in case["records"]], keep_positions=True)["nidx"] == want["nidx"]
            if kind == "plain":
                h.depth_enable(1)
            else:
                h.depth_enable_spliced(8)
                h.junctions_enable(8, JUNCTION_CAPACITY)
            goff, gids = h.classify(*_args(batch))
            bad = first_difference("gene_off", goff, want["goff"]) or first_difference("gene_ids", gids, want["gids"]) or \
                first_difference(kind + " depth", h.depth_all(), want[kind][0]) or \
                first_difference(kind + " depth mates", np.uint64(h.depth_mates()), np.uint64(want[kind][1]))
            if not bad and kind == "spliced":
                got = [tuple(int(v) for v in r) for r in h.junctions_get()]
                if got != want["junctions"]:
                    bad = "junction table: got %s ..., model %s ..." % (got[:3], want["junctions"][:3])
            if bad:
                return bad
        finally:
            h.close()
    return None


# ---------------------------------------------------------------------------
# wide case (c): the second trip of indel_kernel's stride loop
# ---------------------------------------------------------------------------
def draw_wide_indels(seed):
    """(b)'s construction with content of its own: three indel_genes at k = 17; the block's 1 021 pairs come from the first two, the
    remainder's 836 mostly from the third and mostly of the `indel` class, so that the second trip's 321 pairs show events -- and keys --
    that nothing in front of them shows"""
    rng = np.random.default_rng([int(seed), WIDE_C_KEY])
    panel = [indel_gene(rng, 1 + i, 17 + max(FLOORS) + 3) for i in range(3)]
    b1, b2, _ = draw_mates(rng, panel[:2], None, WIDE_B_BLOCK, 17, WIDE_C_FLOOR, 1000, dict(transcript=0.6, record=0.1, deleted=0.05, insertion=0.05, indel=0.2), 0.01)
    r1, r2, _ = draw_mates(rng, panel[2:] * 3 + panel[:2], None, WIDE_B_REST, 17, WIDE_C_FLOOR, 1000, dict(transcript=0.2, record=0.05, deleted=0.05, indel=0.7), 0.01)
    return dict(seed=int(seed), k=17, records=[g["rec"] for g in panel], block=synth.batch_from_lists(b1, b2), rest=synth.batch_from_lists(r1, r2),
                longest=max(len(m) for m in b1 + b2 + r1 + r2))


def expected_wide_indels(case, oracle):
    """T x model(block) + model(remainder): the table's counts and the seven counters are sums over mates as well.  Alignments mode is
    off: the records are those of align_kernel's storing launch at the mode's own floor.  `tail`: the table and counters of the second
    trip's 321 pairs alone; `tail_only`: its keys that neither the block nor the remainder's pairs in front of them show"""
    T = WIDE_B_TIMES
    recs = [bytes(r) for r in case["records"]]
    o = oracle.Shark(k=17, c=0.0, bf_bits=BF_BITS, min_quality=0)
    nidx = o.build(recs)
    sm = SegmentsModel(recs, 17)
    out = dict(nidx=nidx)
    first = DEPTH_LANES - T * WIDE_B_BLOCK

    def part(b):
        goff, gids = o.classify(*_args(b))
        rows = expected_segments(sm, b, goff, gids, 4)[1]
        al = expected_alignments(sm, b, goff, gids, rows, WIDE_C_FLOOR)
        return np.asarray(goff).astype(np.int64), np.asarray(gids), expected_indels(al, b, goff, gids, sm.records, WIDE_C_MIN_INTRON)

    def cut(b, lo, hi):
        return synth.batch_from_lists(*[[b["seq" + m][int(b["off" + m][i]):int(b["off" + m][i + 1])] for i in range(lo, hi)] for m in ("1", "2")])

    (bo, bi, (btab, bst)), (ro, ri, (rtab, rst)) = part(case["block"]), part(case["rest"])
    out["goff"] = np.concatenate([[0]] + [bo[1:] + t * bo[-1] for t in range(T)] + [ro[1:] + T * bo[-1]]).astype(np.uint32)
    out["gids"] = np.concatenate([np.tile(bi, T), ri]).astype(np.uint16)
    table = {key: [f * T, r * T] for key, (f, r) in btab.items()}
    for key, (f, r) in rtab.items():
        e = table.setdefault(key, [0, 0])
        e[0], e[1] = e[0] + f, e[1] + r
    out["indels"] = (table_array(table), {name: bst[name] * T + rst[name] for name in bst})
    head, tail = part(cut(case["rest"], 0, first))[2], part(cut(case["rest"], first, WIDE_B_REST))[2]
    assert {name: head[1][name] + tail[1][name] for name in rst} == rst                  # (sums over mates: the remainder is its two parts)
    out["tail"], out["tail_only"] = tail, sorted(set(tail[0]) - set(btab) - set(head[0]))
    o.close()
    return out


def run_wide_indels(case, oracle, want=None):
    """None or the mismatch's message: one context, one classify, indels mode alone"""
    import torch  # noqa: F401
    from shark_amd import SharkHip
    want = want or expected_wide_indels(case, oracle)
    batch = tiled(case["block"], WIDE_B_TIMES, case["rest"])
    assert len(batch["off1"]) - 1 == WIDE_B_PAIRS > DEPTH_LANES
    h = SharkHip(k=17, c=0.0, bf_bits=BF_BITS)
    try:
        assert h.build([bytes(r) for r in case["records"]], keep_positions=False, keep_bases=True)["nidx"] == want["nidx"]
        h.indels_enable(WIDE_C_FLOOR, WIDE_C_MIN_INTRON, JUNCTION_CAPACITY)
        goff, gids = h.classify(*_args(batch))
        bad = first_difference("gene_off", goff, want["goff"]) or first_difference("gene_ids", gids, want["gids"])
        if bad:
            return bad
        stats = h.indels_stats()
        return compare_indels(None if stats["dropped"] else h.indels_get(0), stats, want["indels"])
    finally:
        h.close()


# ---------------------------------------------------------------------------
# the replay and soak driver
# ---------------------------------------------------------------------------
def main():
    from oracle import pyoracle
    if not os.path.exists(pyoracle.LIB_PATH):
        pyoracle.build()
    iters = int(sys.argv[1]) if len(sys.argv) > 1 else 100
    seed0 = int(sys.argv[2]) if len(sys.argv) > 2 else 20261021
    bias = sys.argv[3] if len(sys.argv) > 3 else ""
    t_start = time.time()
    total = {}
    for it in range(iters):
        case = draw(seed0 + it, bias)
        want = expected(case, pyoracle)
        bad, facts = run(case, pyoracle, want)
        for key, v in want["coverage"].items():
            if isinstance(v, int) and key not in ("widest", "indels.largest_shift"):
                total[key] = total.get(key, 0) + v
        print("%4d %s assoc=%d long=%d %s" % (it, describe(case), facts["n_assoc"], facts["last_n_long"], "ok" if not bad else "MISMATCH"), flush=True)
        if bad:
            print(bad)
            print("replay: python tests/fuzz_records.py 1 %d %s" % (seed0 + it, bias))
            sys.exit(1)
    print("FUZZ OK: %d cases in %.0f s; coverage %s" % (iters, time.time() - t_start, dict(sorted(total.items()))))


if __name__ == "__main__":
    main()
