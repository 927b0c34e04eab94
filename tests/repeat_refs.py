"""Seeded references with the structure of real gene FASTAs -- paralog families, an interspersed element, low-complexity runs,
tandem copies, a k-mer-saturated neighbourhood of one minimiser, one motif shared by tens of thousands of records -- and reads
that SWEEP the boundaries of that structure instead of drawing positions.  numpy only; genes and mates are uint8 arrays as in
tests/synth.py, so the same bytes go to the oracle and to the library.

Every reference builder returns (genes, marks): marks is a list of dicts {"kind", "gene", "start", "end", ...} naming where the
structure sits (half-open, in the gene's own coordinates), which is what the read builders take.  `compose` joins several such
results into one reference and renumbers the marks."""
import numpy as np

from tests import synth

A, C, G, T, N = (ord(x) for x in "ACGTN")
RUN_LENGTHS = (-1, 0, 1, 100, 253, 254, 255, 256, 300, 1000)      # -1, 0, 1: k - 1, k, k + 1


def _seq(s):
    return np.frombuffer(s if isinstance(s, bytes) else s.encode(), np.uint8).copy()


def _substitute(rng, s, rate=None, at=None):
    """substitutions that always change the base (so `identity` is what it says)"""
    s = s.copy()
    idx = np.flatnonzero(rng.random(len(s)) < rate) if at is None else np.asarray(at)
    for j in idx:
        s[j] = rng.choice([b for b in (A, C, G, T) if b != s[j]])
    return s


def _indels(rng, s, n):
    """n insertions or deletions of 1-3 bases"""
    for _ in range(n):
        j = int(rng.integers(1, len(s) - 4))
        w = int(rng.integers(1, 4))
        s = np.concatenate([s[:j], synth.random_seq(rng, w), s[j:]]) if rng.random() < 0.5 else np.concatenate([s[:j], s[j + w:]])
    return s


def compose(*parts):
    genes, marks = [], []
    for g, m in parts:
        marks += [dict(x, gene=x["gene"] + len(genes)) for x in m]
        genes += list(g)
    return genes, marks


def plain(rng, n, lo=300, hi=1500):
    return synth.make_genes(rng, n, lo, hi), []


# ---------------------------------------------------------------------------
# references
# ---------------------------------------------------------------------------
def families(rng, n_fam, n_par, length, identity):
    """n_fam families of n_par paralogs, each derived from its family's ancestor by substitutions (1 - identity per base) and up to
    three 1-3-base indels.  The reference's last two records are an exact duplicate and the reverse complement of member 0."""
    genes, marks = [], []
    for f in range(n_fam):
        anc = synth.random_seq(rng, length)
        for p in range(n_par):
            s = _indels(rng, _substitute(rng, anc, 1.0 - identity), int(rng.integers(0, 4)))
            marks.append({"kind": "paralog", "gene": len(genes), "start": 0, "end": len(s), "family": f})
            genes.append(s)
    marks.append({"kind": "duplicate", "gene": len(genes), "start": 0, "end": len(genes[0]), "of": 0})
    genes.append(genes[0].copy())
    marks.append({"kind": "revcomp", "gene": len(genes), "start": 0, "end": len(genes[0]), "of": 0})
    genes.append(synth.revcomp(genes[0]))
    return genes, marks


def interspersed(rng, genes, element_len, n_carriers, divergence, both_strands=True):
    """one element of element_len bases inserted into the first n_carriers genes (new random genes when `genes` has fewer) at a
    random position, in either orientation; copy i is diverged by substitutions at a rate that runs from 0 (the first three fifths of
    the carriers: exact copies, the conserved k-mers' lists have that many genes) up to `divergence`"""
    genes = [g.copy() for g in genes]
    while len(genes) < n_carriers:
        genes.append(synth.random_seq(rng, int(rng.integers(150, 400))))
    el = synth.random_seq(rng, element_len)
    marks = []
    for i in range(n_carriers):
        rate = 0.0 if 5 * i < 3 * n_carriers else divergence * (5 * i - 3 * n_carriers) / (2.0 * n_carriers)
        e = _substitute(rng, el, rate)
        rev = bool(both_strands and rng.random() < 0.5)
        if rev:
            e = synth.revcomp(e)
        at = int(rng.integers(0, len(genes[i]) + 1))
        genes[i] = np.concatenate([genes[i][:at], e, genes[i][at:]])
        marks.append({"kind": "element", "gene": i, "start": at, "end": at + element_len, "rev": rev, "rate": rate})
    return genes, marks


def _unit_run(unit, n):
    u = _seq(unit) if isinstance(unit, (str, bytes)) else unit
    return np.tile(u, n // len(u) + 1)[:n]


def low_complexity(rng, genes, k):
    """homopolymer runs of k - 1, k, k + 1, 100, 253, 254, 255, 256, 300 and 1 000 bases (A), the complement of the 300 run in
    another gene (one canonical k-mer for both), (AC)n, (AT)n, a period-3 and a period-(k - 1) repeat, a run broken by one N, a run
    with a lower-case stretch, a run at the very start and at the very end of a record, and a record that is nothing but a run.
    Each structure sits in a carrier of its own: genes[i] while they last, new random records after that."""
    src = [g.copy() for g in genes]
    out, marks = [], []

    def put(run, kind, where="mid", **kw):
        body = src.pop(0) if src else synth.random_seq(rng, int(rng.integers(200, 500)))
        # the flanks must not prolong the run
        if where == "only":
            body = body[:0]
            at = 0
        elif where == "start":
            at = 0
        elif where == "end":
            at = len(body)
        else:
            at = int(rng.integers(k + 3, len(body) - k - 2))
        left, right = body[:at].copy(), body[at:].copy()
        if not len(run):                                   # (k = 1: the run of k - 1 bases is empty)
            left = left[:0]
        elif len(left) and left[-1] in (run[0], run[0] | 0x20, run[-1]):
            left[-1] = G if run[0] not in (G, G | 0x20) and run[-1] != G else T
        if len(run) and len(right) and right[0] in (run[-1], run[-1] | 0x20, run[0]):
            right[0] = G if run[-1] not in (G, G | 0x20) and run[0] != G else T
        marks.append(dict({"kind": kind, "gene": len(out), "start": at, "end": at + len(run)}, **kw))
        out.append(np.concatenate([left, run, right]))

    for d in RUN_LENGTHS:
        n = k + d if d <= 1 else d
        put(_unit_run("A", n), "homopolymer", n=n)
    put(_unit_run("T", 300), "homopolymer-complement", n=300)
    put(_unit_run("AC", 120), "period2-AC", n=120)
    put(_unit_run("AT", 120), "period2-AT", n=120)
    put(_unit_run("ACG", 150), "period3", n=150)
    put(_unit_run(synth.random_seq(rng, max(k - 1, 2)), 200), "period-k-1", n=200)
    r = _unit_run("C", 120)
    r[60] = N
    put(r, "run-with-N", n=120)
    r = _unit_run("G", 120)
    r[40:75] |= 0x20
    put(r, "run-lower-case", n=120)
    put(_unit_run("C", 90), "run-at-start", where="start", n=90)
    put(_unit_run("G", 90), "run-at-end", where="end", n=90)
    put(_unit_run("T", 200), "run-only", where="only", n=200)
    out += src                                             # carriers that were not needed stay in the reference
    return out, marks


def tandem(rng, unit_len, copies, drift):
    """one gene: 120 unique bases, `copies` copies of a unit of unit_len bases, 150 unique bases.  drift: copy j (j >= 1) differs from
    copy j - 1 by one more substitution at a random place (so copy j differs from copy 0 at up to j places)"""
    unit = synth.random_seq(rng, unit_len)
    head, tail = synth.random_seq(rng, 120), synth.random_seq(rng, 150)
    head[-1] = synth.ACGT[(list(synth.ACGT).index(unit[-1]) + 1) % 4]      # the array starts and ends where the marks say: the flanks do not
    first = unit[0]                                                          # continue the period by a base
    parts, marks, at = [head], [], len(head)
    for j in range(copies):
        if drift and j:
            unit = _substitute(rng, unit, at=[int(rng.integers(0, unit_len))])
        parts.append(unit.copy())
        marks.append({"kind": "tandem-copy", "gene": 0, "start": at, "end": at + unit_len, "copy": j, "copies": copies})
        at += unit_len
    tail[0] = next(b for b in synth.ACGT if b not in (first, unit[0]))
    parts.append(tail)
    return [np.concatenate(parts)], marks


KTAB_C1 = 0x9E3779B1          # the hash of the minimiser-bucketed table (shark_amd/csrc/kmer_device.hpp: ktab_home)


def _pack(s):
    v = 0
    for b in s:
        v = (v << 2) | {A: 0, C: 1, G: 2, T: 3}[int(b) & 0xDF]
    return v


def _unpack(v, n):
    return np.array([(A, C, G, T)[(v >> (2 * (n - 1 - i))) & 3] for i in range(n)], np.uint8)


def wmer_hash(s):
    """hash of the canonical form of w-mer s (w <= 15) as ktab_home computes it; the smallest one among a k-mer's w-mers names the line"""
    a, b = _pack(s), _pack(synth.revcomp(np.asarray(s, np.uint8)))
    return (min(a, b) * KTAB_C1) & 0xFFFFFFFF


def smallest_hash_wmer(w):
    """the w-mer (w <= 15) whose hash is the smallest there is: h = 1, 2, ... until the preimage under the (odd, hence invertible)
    multiplier is a w-mer in canonical form.  Whatever k-mer contains it has it as its minimiser."""
    inv = pow(KTAB_C1, -1, 1 << 32)
    for h in range(1, 1 << 20):
        a = (h * inv) & 0xFFFFFFFF
        if a < (1 << (2 * w)):
            s = _unpack(a, w)
            if a <= _pack(synth.revcomp(s)) and wmer_hash(s) == h:
                return s, h
    raise AssertionError("no w-mer found")


def saturated_neighbourhood(rng, k, w, wmer=None):
    """genes that together contain every k-mer around the w-mer with the smallest hash: for each of its k - w + 1 places in a k-mer
    and each of the 4^(k - w) fillings of the other places, the k-mer between two random flanks of 12 bases; one gene per place.
    All (k - w + 1) * 4^(k - w) k-mers (48 for k = 17, w = 15) share that minimiser, hence one 16-slot line of the table.
    wmer: another w-mer to build the neighbourhood of (its k-mers share it as their minimiser only where no other w-mer of theirs
    hashes lower)."""
    m = smallest_hash_wmer(w)[0] if wmer is None else np.asarray(wmer, np.uint8)
    genes, marks = [], []
    for place in range(k - w + 1):
        parts, at = [], 0
        for fill in range(4 ** (k - w)):
            f = _unpack(fill, k - w)
            km = np.concatenate([f[:place], m, f[place:]])
            fl = synth.random_seq(rng, 12)
            parts += [fl, km]
            marks.append({"kind": "neighbour", "gene": place, "start": at + 12, "end": at + 12 + k})
            at += 12 + k
        parts.append(synth.random_seq(rng, 12))
        genes.append(np.concatenate(parts))
    return genes, marks


def poly_a_carriers(rng, n_genes):
    """n_genes random records of 150-400 bases, each with an A or T run of 20 ... 60 bases somewhere inside"""
    genes, marks = [], []
    for i in range(n_genes):
        g = synth.random_seq(rng, int(rng.integers(150, 400)))
        n = int(rng.integers(20, 61))
        at = int(rng.integers(1, len(g) - n - 1))
        g[at:at + n] = A if i % 3 else T
        marks.append({"kind": "poly-a", "gene": i, "start": at, "end": at + n, "n": n})
        genes.append(g)
    return genes, marks


def shared_motif(rng, n_genes, motif_len=40, flank=30):
    """n_genes records: random flank, one common motif, random flank -- every k-mer of the motif carries a list of n_genes genes"""
    motif = synth.random_seq(rng, motif_len)
    fl = synth.ACGT[rng.integers(0, 4, size=(n_genes, 2, flank))]
    genes = [np.concatenate([fl[i, 0], motif, fl[i, 1]]) for i in range(n_genes)]
    marks = [{"kind": "motif", "gene": 0, "start": flank, "end": flank + motif_len, "n_genes": n_genes}]
    return genes, marks


# ---------------------------------------------------------------------------
# reads: lists of (mate1, mate2) uint8 arrays
# ---------------------------------------------------------------------------
def _pair(g, s, L, gap, flip):
    """the pair of a fragment of L + gap bases at s (clipped to the gene): mate 1 its first L bases, mate 2 the first L bases of its
    reverse complement; flip: the fragment's other strand"""
    s = max(0, min(s, len(g)))
    f = g[s:s + L + gap]
    if flip:
        f = synth.revcomp(f)
    return f[:L].copy(), synth.revcomp(f)[:L].copy()


def sweep(genes, gene, b, L, gap=40, step=1):
    """boundary b of a repeat inside genes[gene]: the pairs whose mate 1 starts at every offset b - L + 1 ... b (every step-th),
    alternating strands"""
    g = genes[gene]
    return [_pair(g, s, L, gap, (s // step) & 1) for s in range(max(0, b - L + 1), min(b, len(g) - 1) + 1, step)]


def inside(genes, gene, start, end, L, step=1):
    """pairs lying wholly inside [start, end) of genes[gene] (mate 2 the reverse complement of the same bases)"""
    g = genes[gene]
    L = min(L, end - start)
    return [_pair(g[:end], s, L, 0, (s // step) & 1) for s in range(start, end - L + 1, step)]


def pure(L):
    """low-complexity pairs: A x L, T x L, (AC) x L/2, (AT) x L/2, (ACG) x L/3"""
    out = []
    for u in ("A", "T", "AC", "AT", "ACG"):
        r = _unit_run(u, L)
        out.append((r.copy(), synth.revcomp(r)))
    return out


def polya_tail(rng, L, tails=(10, 20, 30, 40, 50, 60)):
    """off-target random pairs with a poly-A tail of 10 ... 60 bases on mate 1 (poly-T head on mate 2)"""
    out = []
    for t in tails:
        m1 = synth.random_seq(rng, L)
        t = min(t, L)
        m1[L - t:] = A
        m2 = synth.random_seq(rng, L)
        m2[:t] = T
        out.append((m1, m2))
    return out


def dress(rng, pairs, sub=0.0, n_rate=0.0, lower=0.0):
    """substitutions, N and lower-case stretches on top of pairs"""
    out = []
    for pr in pairs:
        ms = []
        for m in pr:
            m = m.copy()
            hit = rng.random(len(m)) < sub
            m[hit] = synth.ACGT[rng.integers(0, 4, size=int(hit.sum()))]
            m[rng.random(len(m)) < n_rate] = N
            if lower and len(m) > 8 and rng.random() < lower:
                j = int(rng.integers(0, len(m) - 4))
                m[j:j + int(rng.integers(3, 30))] |= 0x20
            ms.append(m)
        out.append(tuple(ms))
    return out


def batch(pairs, paired=True, ragged_rng=None, qual_rng=None):
    """SoA batch (tests/synth.py layout).  ragged_rng: every mate cut to a length drawn from [len/2, len] -- synth.make_reads' var_len
    convention; qual_rng: qualities, nine in ten of them 30 ... 41"""
    m1, m2 = [], []
    for a, b in pairs:
        if ragged_rng is not None:
            a = a[:int(ragged_rng.integers(max(1, len(a) // 2), len(a) + 1))] if len(a) else a
            b = b[:int(ragged_rng.integers(max(1, len(b) // 2), len(b) + 1))] if len(b) else b
        m1.append(a)
        m2.append(b)

    def quals(ms):
        return [(np.where(qual_rng.random(len(m)) < 0.9, qual_rng.integers(30, 42, size=len(m)), qual_rng.integers(2, 30, size=len(m))) + 33).astype(np.uint8)
                for m in ms]
    q1 = quals(m1) if qual_rng is not None else None
    q2 = quals(m2) if (qual_rng is not None and paired) else None
    return synth.batch_from_lists(m1, m2 if paired else None, q1, q2)


def pad_uniform(pairs, L, rng):
    """every mate exactly L bases: shorter ones (fragments clipped at a record's end) continued with random bases"""
    out = []
    for pr in pairs:
        out.append(tuple(np.concatenate([m, synth.random_seq(rng, L - len(m))]) if len(m) < L else m[:L] for m in pr))
    return out


def boundary_sweeps(genes, marks, L, step=1, kinds=None):
    """sweeps over both ends of every marked structure (of the given kinds)"""
    out = []
    for m in marks:
        if kinds is None or m["kind"] in kinds:
            out += sweep(genes, m["gene"], m["start"], L, step=step) + sweep(genes, m["gene"], m["end"], L, step=step)
    return out


def mixed_reference(rng, k=17):
    """a random mix of the builders: what the fuzzer's "rep" bias draws its genes from"""
    parts = [plain(rng, int(rng.integers(2, 12)), 200, 1200)]
    if rng.random() < 0.7:
        parts.append(families(rng, int(rng.integers(1, 4)), int(rng.integers(2, 9)), int(rng.integers(300, 1500)), float(rng.choice([0.9, 0.95, 0.99, 0.995]))))
    if rng.random() < 0.8:
        parts.append(interspersed(rng, [], int(rng.integers(80, 301)), int(rng.integers(10, 301)), float(rng.choice([0.0, 0.05, 0.15]))))
    if rng.random() < 0.5:
        parts.append(low_complexity(rng, [], k))
    if rng.random() < 0.6:
        parts.append(tandem(rng, int(rng.integers(40, 401)), int(rng.integers(2, 31)), bool(rng.random() < 0.5)))
    return compose(*parts)


# ---------------------------------------------------------------------------
# whole-program cases (the layout of tests/ref_cases.py): one small case per builder, recorded from the reference program into
# tests/golden/ref_repeat_cases.npz by tests/golden/gen_ref_repeat_cases.py, and the four long-list cases, which are only run
# live (their ssv runs to megabytes)
# ---------------------------------------------------------------------------
BUILDER_CASES = ("families", "interspersed", "low_complexity", "tandem", "saturated_neighbourhood", "shared_motif")
LONG_CASES = ("motif65534", "motif65535", "motif65536", "motif70000")


def program_case(name):
    """the inputs of case `name` as tests/ref_cases.py's `case` lays them out (no outputs yet)"""
    from tests import ref_cases as rc
    rng = np.random.default_rng(20261101 + (BUILDER_CASES + LONG_CASES).index(name))
    k, c, single, bf_bits = 17, 0.5, False, 1 << 22
    if name == "families":
        genes, marks = families(rng, 2, 4, 400, 0.95)
        pairs = [_pair(genes[m["gene"]], int(s), 100, 40, bool(s & 1)) for m in marks for s in rng.integers(0, 250, 4)]
        c = 0.6
    elif name == "interspersed":
        genes, marks = interspersed(rng, [], 120, 50, 0.15)
        pairs = []
        for m in (marks[0], marks[20], marks[-1]):
            pairs += sweep(genes, m["gene"], m["start"], 76, step=9) + sweep(genes, m["gene"], m["end"], 76, step=9)
            pairs += inside(genes, m["gene"], m["start"], m["end"], 76, step=11)
        c = 0.3
    elif name == "low_complexity":
        genes, marks = low_complexity(rng, [], k)
        pairs = boundary_sweeps(genes, marks, 100, step=17) + pure(100) + pure(40) + polya_tail(rng, 100)
    elif name == "tandem":
        genes, marks = compose(tandem(rng, 60, 8, True), tandem(rng, 45, 12, False))
        pairs = boundary_sweeps(genes, marks, 100, step=13)
        c = 0.6
    elif name == "saturated_neighbourhood":
        genes, marks = saturated_neighbourhood(rng, k, 15)
        pairs = [(genes[m["gene"]][m["start"]:m["end"]], synth.revcomp(genes[m["gene"]][m["start"]:m["end"]])) for m in marks]
        pairs += boundary_sweeps(genes, marks[::8], 60, step=7)
        c = 0.0
    elif name == "shared_motif":
        genes, marks = shared_motif(rng, 300)
        motif = genes[0][30:70]
        pairs = [(motif, motif[:0]), (genes[7][:80], synth.revcomp(genes[7][:80])), (motif[3:30], synth.revcomp(motif)), (synth.random_seq(rng, 80),) * 2,
                 (genes[299][10:90], motif[:0])]
        c = 0.0
    else:
        n = int(name[5:])
        genes, marks = shared_motif(rng, n)
        if n == 70000:
            genes[69000] = np.concatenate([_unit_run("A", 70000), _seq("C"), synth.random_seq(rng, 49)])
        motif = genes[0][30:70]
        none = motif[:0]
        pairs = [(motif, none), (genes[5][:80], none), (_unit_run("A", 60), none), (synth.random_seq(rng, 80), none), (none, none),
                 (np.concatenate([genes[min(n - 1, 69000)][-50:], _unit_run("A", 30)]), none), (motif, synth.revcomp(motif)), (genes[n - 1][10:90], none)]
        c, bf_bits = 0.0, 1 << 30
    recs = [("g%d" % i, "", bytes(g)) for i, g in enumerate(genes)]
    reads = [(b"r%d/1" % i, bytes(a), b"I" * len(a), b"r%d/2" % i, bytes(b), b"I" * len(b)) for i, (a, b) in enumerate(pairs)]
    return rc.case(name, recs, reads, k, c, 0, single, bf_bits)
