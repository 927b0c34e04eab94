"""The case table of rescue mode's tests (include/shark_hip.h, "rescue"), in plain Python and numpy: pairs built directly from one record
of 12 000 bases.  The ANCHOR is a perfect copy of record bases (or its reverse complement); the TARGET is a copy of record bases made
silent without touching c, so that the pair stays classified and the target gets no block.  A mate's support is the number of its
windows that vote for its best diagonal, so a target is silent when fewer than S_MIN of its windows are clean: evenly spread
substitutions see to that (a target with fewer than S_MIN windows is silent as it is), and its cost at its true place is their
number.  A long target would need more substitutions than any sensible max_cost allows; it is cut from a stretch of the record that
occurs twice (SHADOW), whose k-mers are ambiguous and do not vote at all: silent at cost 0, the second copy far outside the window.  tests/test_rescue_cpu.py holds the table against the model on the CPU, tests/test_gpu_rescue.py runs it on
the GPU.  Every case says what it was built for; `expect` holds what must come out at the parameter set named.

The whole table runs behind -q 20: every base has quality 40 but the ones a case masks.

The tests' references hold the record and a second one, unrelated (DECOY), or the record several times over.  On an index of ONE
record the classifier's one-gene kernels drop some pairs of more than about 500 bases from a ragged host batch -- the table's long
targets among them, with every mode off, against the oracle -- which is not rescue mode's code and not what this table is about."""
import numpy as np

from tests import synth

MIN_INTRON = 20
MAX_FRAG = 611            # a perfect anchor of 100 bases beside a target of 100: n_cand = 512, eight full passes of 64
MAX_COST = 8
MIN_GAP = 4
S_MIN = 60
MIN_QUALITY = 20
LA = 100                  # the anchor's length, and most targets'
LEN_G = 12000
CAP1 = MAX_COST + MIN_GAP + 1

# parameter sets (min_intron, max_frag, max_cost, min_gap) the table is run at
PARAMS = {"default": (MIN_INTRON, MAX_FRAG, MAX_COST, MIN_GAP), "gap0": (MIN_INTRON, MAX_FRAG, MAX_COST, 0), "wide": (MIN_INTRON, 4096, MAX_COST, MIN_GAP)}

# the record's special places
TANDEM_FAR = (2000, 2300)         # an exact copy of 100 bases 300 further on: two candidates of equal cost in different passes
TANDEM_GAP = (3000, 3300)         # a copy with MIN_GAP substitutions: costs apart by exactly min_gap
TANDEM_GAP1 = (3600, 3900)        # a copy with MIN_GAP - 1 substitutions
TANDEM_NEAR = (4400, 4450)        # an exact copy of 40 bases 50 further on: two candidates of equal cost in one pass
COPY_SUBS = (3, 5, 7, 9)          # where the inexact copies differ (no silencing substitution falls there)
RECORD_N = 5050
INTRON = (6100, 6400)             # the spliced anchor is record[6000:6100] + record[6400:6500]
SHADOW = (9200, 10500, 560)       # record[9200:9760] occurs again at 10 500: no k-mer of it votes


def make_record(seed=1):
    rng = np.random.default_rng(seed)
    rec = synth.random_seq(rng, LEN_G)
    for (a, b), n_sub in ((TANDEM_FAR, 0), (TANDEM_GAP, MIN_GAP), (TANDEM_GAP1, MIN_GAP - 1)):
        rec[b:b + LA] = _sub(rec[a:a + LA], *COPY_SUBS[:n_sub])
    rec[TANDEM_NEAR[1]:TANDEM_NEAR[1] + 40] = rec[TANDEM_NEAR[0]:TANDEM_NEAR[0] + 40]
    rec[RECORD_N] = ord("N")
    a, b, n = SHADOW
    rec[b:b + n] = rec[a:a + n]
    return rec


def make_decoy(seed=77):
    return synth.random_seq(np.random.default_rng(seed), 600)


def reference(every=1):
    """the records of a test's reference: the table's record and the decoy, or the record `every` times over"""
    rec = make_record()
    return [rec, make_decoy()] if every == 1 else [rec] * every


def _sub(m, *at):
    m = m.copy()
    for i in at:
        m[i] = synth.ACGT[(int(np.searchsorted(synth.ACGT, m[i])) + 1) % 4]
    return m


def clean_windows(n, k, at):
    """the number of windows of a mate of n bases that hold none of the positions `at`"""
    return sum(all(not (p <= a < p + k) for a in at) for p in range(max(n - k + 1, 0)))


def silencing(n, k, s_min=S_MIN):
    """the fewest evenly spread positions in a mate of n bases that leave fewer than s_min clean windows"""
    m = 0
    while True:
        at = [(i + 1) * n // (m + 1) for i in range(m)]
        if clean_windows(n, k, at) < s_min:
            return at
        m += 1


def rescue_cases(k, seed=1):
    """(record, cases): cases is a list of dicts: name, m1, m2, q1, q2 (qualities), why, expect = {parameter set: dict(state, and where
    rescued x, cost; optionally n_cand, cost2, matches, mismatches)}"""
    rec = make_record(seed)
    rng = np.random.default_rng(seed + 1)
    rc = synth.revcomp
    F = lambda a, n=LA: rec[a:a + n].copy()                       # noqa: E731  an anchor on strand 0
    R = lambda a, n=LA: rc(rec[a:a + n])                          # noqa: E731  an anchor on strand 1
    cases = []

    def target(x, n, strand, extra=(), put=None):
        """(the target mate, its cost at x): record[x:x + n] silenced, with substitutions at `extra` and the bytes of put = {q: byte} on
        top (positions in the record's orientation), on `strand`"""
        in_shadow = SHADOW[0] <= x and x + n <= SHADOW[0] + SHADOW[2]
        at = ([] if in_shadow else silencing(n, k)) + list(extra)
        assert len(set(at)) == len(at) and not set(at) & set(COPY_SUBS), (at, "substitutions collide")
        assert in_shadow or clean_windows(n, k, at) < S_MIN
        m = _sub(rec[x:x + n], *at)
        for q, byte in (put or {}).items():
            assert q not in at
            m[q] = byte
        return (rc(m) if strand else m), len(at) + len(put or {})

    def add(name, anchor, tgt, anchor_is, why, expect, quals=None):
        m = (anchor, tgt) if anchor_is == 1 else (tgt, anchor)
        q = quals or (None, None)
        q = (q[0], q[1]) if anchor_is == 1 else (q[1], q[0])
        cases.append(dict(name=name, m1=m[0], m2=m[1], q1=q[0], q2=q[1], why=why, expect=expect))

    def rescued(t_mate, x, cost, **more):
        return dict(state=3 + t_mate, x=x, cost=cost, **more)

    # ---- the four arrangements: the anchor on either strand, as either mate ----
    t, c = target(700, LA, 1)
    add("A on strand 0 as mate 1", F(500), t, 1, "the plain case", {"default": rescued(2, 700, c, n_cand=512), "wide": rescued(2, 700, c, n_cand=3997)})
    add("A on strand 0 as mate 2", F(500), t, 2, "mates swapped: state 4", {"default": rescued(1, 700, c)})
    t, c = target(500, LA, 0)
    add("A on strand 1 as mate 1", R(700), t, 1, "the target on strand 0, left of the anchor", {"default": rescued(2, 500, c, n_cand=512)})
    add("A on strand 1 as mate 2", R(700), t, 2, "mates swapped", {"default": rescued(1, 500, c)})
    # ---- the window's ends: lo = 500, hi = 1011 beside F(500); lo = 489, hi = 1000 beside R(1000) ----
    for x, name, ok in ((500, "at lo: lane 0 of the first pass", True), (1011, "at hi: lane 63 of the last pass", True), (499, "one base below lo", False),
                        (1012, "one base beyond hi", False)):
        t, c = target(x, LA, 1)
        add("A on strand 0, target " + name, F(500), t, 1, "the window's edge", {"default": rescued(2, x, c) if ok else dict(state=2, cost=CAP1)})
    for x, name, ok in ((489, "at lo: the last lane of the tie order", True), (1000, "at hi", True), (488, "one base below lo", False), (1001, "one base beyond hi", False)):
        t, c = target(x, LA, 0)
        add("A on strand 1, target " + name, R(1000), t, 1, "the window's edge", {"default": rescued(2, x, c) if ok else dict(state=2, cost=CAP1)})
    # ---- the window cut by the record's ends; n_cand = 1, 63, 64, 65, 129 ----
    for n in (1, 63, 64, 65, 129):
        t, c = target(0, LA, 0)
        add("window cut by the record's start, n_cand %d" % n, R(n - 1), t, 1, "lo = 0; the target in the first lane", {"default": rescued(2, 0, c, n_cand=n)})
        t, c = target(LEN_G - LA, LA, 1)
        add("window cut by the record's end, n_cand %d" % n, F(LEN_G - LA - (n - 1)), t, 1, "hi = len_g - L_T; the target in the last lane",
            {"default": rescued(2, LEN_G - LA, c, n_cand=n, **({"cost2": CAP1} if n == 1 else {}))})
    t, c = target(LEN_G - 400, 120, 1)
    add("empty window", F(LEN_G - LA), t, 1, "a target longer than the anchor, the anchor at the record's end: hi < lo", {"default": dict(state=1, n_cand=0, cost=CAP1, cost2=CAP1)})
    # ---- the cost bound ----
    n_sil = len(silencing(LA, k))
    t, c = target(700, LA, 1, extra=range(11, 11 + MAX_COST - n_sil))
    add("cost exactly max_cost", F(500), t, 1, "rescued", {"default": rescued(2, 700, MAX_COST)})
    t, c = target(700, LA, 1, extra=range(11, 12 + MAX_COST - n_sil))
    add("cost max_cost + 1", F(500), t, 1, "state 2", {"default": dict(state=2, cost=MAX_COST + 1)})
    # ---- a tandem copy: two candidates ----
    a, b = TANDEM_FAR
    t, c = target(a, LA, 1)
    add("tandem copy, A on strand 0", F(a - 100), t, 1, "equal costs in different passes: ambiguous; at min_gap 0 the smallest x",
        {"default": dict(state=3, cost=c, cost2=c), "gap0": rescued(2, a, c, cost2=c)})
    t, c = target(a, LA, 0)
    add("tandem copy, A on strand 1", R(b + 150), t, 1, "at min_gap 0 the largest x: the smallest frag", {"default": dict(state=3, cost=c, cost2=c), "gap0": rescued(2, b, c, cost2=c)})
    a, b = TANDEM_GAP
    t, c = target(a, LA, 1)
    add("copy apart by exactly min_gap", F(a - 100), t, 1, "rescued", {"default": rescued(2, a, c, cost2=c + MIN_GAP)})
    a, b = TANDEM_GAP1
    t, c = target(a, LA, 1)
    add("copy apart by min_gap - 1", F(a - 100), t, 1, "state 3", {"default": dict(state=3, cost=c, cost2=c + MIN_GAP - 1), "gap0": rescued(2, a, c)})
    a, b = TANDEM_NEAR
    t, c = target(a, 40, 1)
    add("near copy: best and second in one pass", F(a - 130), t, 1, "lo = a - 70: candidates 70 and 120, both in the second pass",
        {"default": dict(state=3, cost=0, cost2=0), "gap0": rescued(2, a, 0, cost2=0)})
    # ---- bases that are neither: they count in cost, not in mismatches ----
    n_t = 7 if 7 not in silencing(LA, k) else 8
    t, c = target(700, LA, 1, put={n_t: ord("N")})
    add("N in the target", F(500), t, 1, "cost counts it, mismatches do not", {"default": rescued(2, 700, c, matches=LA - c, mismatches=c - 1)})
    t, c0 = target(700, LA, 1)
    qual = np.full(LA, 33 + 40, dtype=np.uint8)
    qual[[20, 21, 22]] = 33 + 2                                   # (the mate's own bytes 20 .. 22: read coordinates 77 .. 79 on strand 1)
    add("bases masked by -q", F(500), t, 1, "three masked bases", {"default": rescued(2, 700, c0 + 3, matches=LA - c0 - 3, mismatches=c0)},
        quals=(np.full(LA, 33 + 40, dtype=np.uint8), qual))
    t, c = target(RECORD_N - 40, LA, 1, put={40: ord("A")})
    add("record N under the target", F(RECORD_N - 250), t, 1, "record code 4 under a base", {"default": rescued(2, RECORD_N - 40, c, matches=LA - c, mismatches=c - 1)})
    # ---- the anchor's introns and clips move the window ----
    spliced = np.concatenate([rec[6000:INTRON[0]], rec[INTRON[1]:6500]])
    i_a = INTRON[1] - INTRON[0]
    hi = 6000 + i_a + MAX_FRAG - LA
    t, c = target(hi, LA, 1)
    add("spliced anchor, target at hi", spliced, t, 1, "hi = s_A + I_A + max_frag - L_T", {"default": rescued(2, hi, c)})
    t, c = target(hi + 1, LA, 1)
    add("spliced anchor, target beyond hi", spliced, t, 1, "hi moves by exactly I_A", {"default": dict(state=2)})
    t, c = target(7000 + MAX_FRAG - LA, LA, 1)
    add("clipped 5' end of A on strand 0, target at hi", _sub(F(7000), 3), t, 1, "s_A = 7004, cl_A = 4: hi stays 7000 + max_frag - L_T", {"default": rescued(2, 7000 + MAX_FRAG - LA, c)})
    t, c = target(7001 + MAX_FRAG - LA, LA, 1)
    add("clipped 5' end of A on strand 0, target beyond hi", _sub(F(7000), 3), t, 1, "without cl the window would reach it", {"default": dict(state=2)})
    t, c = target(8000 + LA - MAX_FRAG, LA, 0)
    add("clipped 5' end of A on strand 1, target at lo", rc(_sub(F(8000), 96)), t, 1, "e_A = 8096, cr_A = 4: lo stays 8100 - max_frag", {"default": rescued(2, 8000 + LA - MAX_FRAG, c)})
    t, c = target(7999 + LA - MAX_FRAG, LA, 0)
    add("clipped 5' end of A on strand 1, target below lo", rc(_sub(F(8000), 96)), t, 1, "without cr the window would reach it", {"default": dict(state=2)})
    # ---- the target's length ----
    # (the anchor's last ten bases lie in SHADOW: a target of 512 bases beside max_frag 611 must overlap its anchor)
    for n in (31, 32, 33, 57, 101, 102, 103, 511, 512, 513):
        x = 9340 if n <= 103 else 9200                              # (a short target ends behind the anchor's end: lo = e_A - L_T)
        t, c = target(x, n, 1)                                      # (inside SHADOW: silent at cost 0)
        ok = 32 <= n <= 512
        add("L_T = %d" % n, F(9110), t, 1, "whole dwords, a partial last dword, the two bounds",
            {"default": rescued(2, x, c, matches=n - c, mismatches=c, n_cand=(512 if n <= LA else MAX_FRAG - n + 1)) if ok else dict(state=0)})
    t, c = target(5200, LA, 1)
    add("a far target", F(1500), t, 1, "beyond max_frag 611, inside 4 096", {"default": dict(state=2), "wide": rescued(2, 5200, c)})
    # ---- not attempted ----
    add("both mates placed", F(500), R(700), 1, "state 0, records untouched", {"default": dict(state=0)})
    t1, _ = target(500, LA, 0)
    t2, _ = target(700, LA, 1)
    add("no mate placed", t1, t2, 1, "state 0, records untouched", {"default": dict(state=0)})
    add("an off-target partner", F(500), synth.random_seq(rng, LA), 1, "attempted: nothing fits", {"default": dict(state=2, cost=CAP1, cost2=CAP1)})
    return rec, cases


def case_batch(k, seed=1, single_end=False):
    """(record, cases, the SoA batch with qualities)"""
    rec, cases = rescue_cases(k, seed)
    full = lambda m, q: q if q is not None else np.full(len(m), 33 + 40, dtype=np.uint8)   # noqa: E731
    m1, m2 = [c["m1"] for c in cases], [c["m2"] for c in cases]
    q1, q2 = [full(c["m1"], c["q1"]) for c in cases], [full(c["m2"], c["q2"]) for c in cases]
    if single_end:
        return rec, cases, synth.batch_from_lists(m1, None, q1, None)
    return rec, cases, synth.batch_from_lists(m1, m2, q1, q2)


def check_expectations(cases, params, records, rescues, gene_off, every=1):
    """the table's non-vacuity: association j * every of read i carries what case i was built for at the parameter set `params`"""
    gene_off = np.asarray(gene_off)
    seen = set()
    for i, case in enumerate(cases):
        want = case["expect"].get(params)
        if want is None:
            continue
        assert int(gene_off[i + 1]) - int(gene_off[i]) == every, (case["name"], "associations")
        for j in range(int(gene_off[i]), int(gene_off[i + 1])):
            rs = rescues[j]
            seen.add(int(rs["state"]))
            for field, v in want.items():
                if field in ("x", "matches", "mismatches"):
                    t = int(rs["state"]) - 4
                    got = int(records[j][t]["block"][0][0]) if field == "x" else int(records[j][t][field])
                else:
                    got = int(rs[field])
                assert got == v, (case["name"], params, field, got, v, rs)
            if int(rs["state"]) >= 4:
                t = int(rs["state"]) - 4
                assert int(records[j][t]["n_blocks"]) == 1 and tuple(records[j][t]["block"][0])[1] == 0, case["name"]
    return seen
