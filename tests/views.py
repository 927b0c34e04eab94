"""Reads of designed coverage, hostile neighbours and unaligned views of a batch (numpy only; torch is imported by to_device alone).

The classify kernels read a mate as aligned dwords around it and realign in registers, so they touch bytes of the neighbouring
reads and of whatever surrounds the caller's buffers; only masks keep those bytes out of the result.  The generators here make
such a leak visible:

  ladder               pairs whose oracle coverage is designed, on the steps thr - 2 ... thr + 1 around thr = ceil(c * len)
  ladder_with_invalid  the same with a few N (or bases under -q) outside the gene stretch: len, and thr with it, drops
  hostile              reads one base under the threshold whose stretch ends flush with a mate's end (starts flush with its
                       beginning) while the neighbouring bytes of the buffer continue the gene: one leaked base makes them pass
  embed / to_device    the batch's arrays inside larger ones, at chosen byte displacements, between hostile bytes
  with_first_offset    the same reads with off[0] != 0

A read is a tuple (m1, m2, q1, q2) of uint8 arrays (m2, q1, q2 may be None); batch_of() joins reads into the SoA dict of
tests/synth.py."""
import math

import numpy as np

from tests import synth

HI_Q, LO_Q = ord("I"), ord("#")          # phred 40 and phred 2
PAD = 64                                  # bytes around every embedded byte array (lead and trail fit in them)
POISON = np.uint64(2 ** 63)               # what lies around an embedded offsets array


def threshold(c, length):
    """ceil(c * len) in the reference's own double arithmetic (ReadAnalyzer.hpp:104 accepts max >= c * len)"""
    return int(math.ceil(float(c) * float(length)))


# ---------------------------------------------------------------------------
# one pair from runs of gene bases
# ---------------------------------------------------------------------------
def _other(rng, avoid):
    cand = [int(b) for b in synth.ACGT if int(b) not in avoid]
    return cand[int(rng.integers(0, len(cand)))]


def _pair(rng, genes, k, l1, l2, runs, gene=None, before=0, after=0):
    """runs: [(mate, at, x)] with at in 'left' | 'right' | 'mid' | ('first', x2) (two runs x and x2 inside the mate, one mismatching
    base at least between them).  Every run is a window of one gene, on a strand drawn per run; the bases that flank it inside
    the mate differ from the gene's own neighbours of the window, so a run of x bases covers exactly x.  Returns (m1, m2, info, taken):
    info[j] = (mate, position, x, bytes of the gene before the window, bytes behind it) per placed run -- `before` / `after`
    bases of them, in the mate's orientation; taken[t] marks the bytes of mate t that belong to a run."""
    gi = int(rng.integers(0, len(genes))) if gene is None else gene
    mates = [synth.random_seq(rng, l1), synth.random_seq(rng, l2)]
    avoid = [dict(), dict()]
    taken = [np.zeros(l1, bool), np.zeros(l2, bool)]
    info = []

    def place(t, p, x):
        g = genes[gi] if rng.random() < 0.5 else synth.revcomp(genes[gi])
        s = int(rng.integers(before + 1, len(g) - x - after))
        mates[t][p:p + x] = g[s:s + x]
        taken[t][p:p + x] = True
        if p > 0:
            avoid[t].setdefault(p - 1, set()).add(int(g[s - 1]))
        if p + x < len(mates[t]):
            avoid[t].setdefault(p + x, set()).add(int(g[s + x]))
        info.append((t, p, x, g[s - before:s].copy(), g[s + x:s + x + after].copy()))

    for t, at, x in runs:
        L = len(mates[t])
        if isinstance(at, tuple):                     # two runs: x, a gap of one to three bases where they fit, x2
            x2 = at[1]
            gap = int(rng.integers(1, min(3, L - x - x2) + 1))
            p = int(rng.integers(0, L - x - x2 - gap + 1))
            place(t, p, x)
            place(t, p + x + gap, x2)
        else:
            p = 0 if at == "left" else L - x if at == "right" else (int(rng.integers(1, L - x)) if L - x >= 2 else 0)
            place(t, p, x)
    for t in (0, 1):
        for p, av in avoid[t].items():
            if not taken[t][p]:
                mates[t][p] = _other(rng, av)
    return mates[0], mates[1], info, taken


FORMS = ("m1-left", "m1-right", "m1-mid", "m2-left", "m2-right", "m2-mid", "split", "two-runs-m1", "two-runs-m2")


def _runs_of(rng, form, k, l1, l2, x):
    """the runs that give coverage x in this placement form, or None where the form cannot hold x bases"""
    L = (l1, l2)
    if form.startswith("m1-") or form.startswith("m2-"):
        t = int(form[1]) - 1
        return [(t, form[3:], x)] if k <= x <= L[t] else None
    if form == "split":
        lo, hi = max(k, x - l2), min(l1, x - k)
        if l2 == 0 or lo > hi:
            return None
        a = int(rng.integers(lo, hi + 1))
        return [(0, ("left", "right", "mid")[int(rng.integers(0, 3))], a), (1, ("left", "right", "mid")[int(rng.integers(0, 3))], x - a)]
    t = int(form[-1]) - 1                          # two runs inside mate t, the rest (nothing, or k bases at least) in the other mate
    o = 1 - t
    if L[t] == 0:
        return None
    if 2 * k <= x <= L[t] - 1:
        a = x
    else:
        lo, hi = max(2 * k, x - L[o]), min(L[t] - 1, x - k)
        if L[o] == 0 or lo > hi:
            return None
        a = int(rng.integers(lo, hi + 1))
    a1 = int(rng.integers(k, a - k + 1))
    runs = [(t, ("first", a - a1), a1)]
    if x - a:
        runs.append((o, "mid", x - a))
    return runs


def _quals(read_lens, bad):
    """phred 40 everywhere, phred 2 at the positions `bad` (per mate)"""
    out = []
    for L, b in zip(read_lens, bad):
        q = np.full(L, HI_Q, np.uint8)
        q[list(b)] = LO_Q
        out.append(q)
    return out


def ladder(rng, genes, k, L1, L2, c, per_step, qual=False, n_invalid=(0, 0), forms=FORMS):
    """pairs (single-end when L2 == 0) of designed coverage on the steps thr - 2, thr - 1, thr, thr + 1 around thr = ceil(c * len),
    per_step of them per step and placement form (FORMS; a form that cannot hold a step's bases is left out for that step).
    n_invalid = (lo, hi): that many invalid bases per read, outside the gene stretch -- N, or with qual a base of phred 2 (half
    of the time); len and thr drop with them.  Returns (reads, design): design[i] = (coverage, len, step - thr, form)."""
    reads, design = [], []
    for form in forms:
        for step in (-2, -1, 0, 1):
            for _ in range(per_step):
                ninv = int(rng.integers(n_invalid[0], n_invalid[1] + 1))
                length = L1 + L2 - ninv
                x = threshold(c, length) + step
                runs = _runs_of(rng, form, k, L1, L2, x)
                if runs is None:
                    continue
                m1, m2, _, taken = _pair(rng, genes, k, L1, L2, runs)
                free = [(t, int(p)) for t in (0, 1) for p in np.flatnonzero(~taken[t])]
                if len(free) < ninv:
                    continue
                bad = [set(), set()]
                for j in rng.permutation(len(free))[:ninv]:
                    t, p = free[int(j)]
                    if qual and rng.random() < 0.5:
                        bad[t].add(p)
                    else:
                        (m1, m2)[t][p] = ord("N")
                q1, q2 = _quals((L1, L2), bad) if qual else (None, None)
                reads.append((m1, m2 if L2 else None, q1, q2 if L2 else None))
                design.append((x, length, step, form))
    return reads, design


def ladder_with_invalid(rng, genes, k, L1, L2, c, per_step, qual=False, forms=FORMS):
    """ladder with 1 to 3 invalid bases per read outside the stretch"""
    return ladder(rng, genes, k, L1, L2, c, per_step, qual=qual, n_invalid=(1, 3), forms=forms)


# ---------------------------------------------------------------------------
# hostile neighbours
# ---------------------------------------------------------------------------
def _share(rng, k, x, Lt, Lo):
    """how many of x bases lie in the target mate (of Lt bytes; the rest, nothing or k at least, in the other of Lo bytes)"""
    if x <= Lt and (Lo == 0 or rng.random() < 0.5):
        return x
    lo, hi = max(k, x - Lo), min(Lt, x - k)
    if Lo == 0 or lo > hi:
        return None
    return int(rng.integers(lo, hi + 1))


def hostile(rng, genes, k, L1, L2, c, per_case=2, trimmed=False, qual=False, ext=None):
    """reads of designed coverage thr - 1 whose stretch ends flush with a mate's end (starts flush with its beginning), each next to
    a neighbour -- an off-target read -- whose adjoining bytes continue the gene for ext >= k bases: a kernel that lets one byte
    of the neighbour into the mate sees coverage thr.  Both mates, both ends.  trimmed: the mate is cut to a shorter length (the
    batch is ragged), and there are mates of k - 1 bases whose neighbour would complete their only k-mer.
    Returns (units, marks, edges): units = lists of reads that must stay adjacent and in order; marks[u] = [(index in the unit,
    mate, 'end' | 'begin')]; edges = (first, lead, last, trail): a read for the head of the batch whose two mates start flush,
    with the bytes to put before each sequence array, and one for the tail whose mates end flush, with the bytes behind."""
    ext = ext or k + 8
    units, marks = [], []

    def q_of(m):
        return np.full(len(m), HI_Q, np.uint8) if qual and m is not None else None

    def read(m1, m2):
        return (m1, m2 if L2 else None, q_of(m1), q_of(m2) if L2 else None)

    def neighbour(t, end, cont, l1, l2):
        n1, n2 = synth.random_seq(rng, l1), synth.random_seq(rng, l2)
        m = (n1, n2)[t]
        if end == "end":
            m[:len(cont)] = cont                      # behind the hostile mate: the neighbour's first bases
        else:
            m[len(m) - len(cont):] = cont             # before it: the neighbour's last bases
        return read(n1, n2)

    def one(t, end, lt, lo, short=False):
        l1, l2 = (lt, lo) if t == 0 else (lo, lt)
        x = threshold(c, l1 + l2) - 1
        if short:                                     # the target mate is k - 1 gene bases and covers nothing; all of x in the other mate
            if not (k <= x <= lo):
                return
            runs = [(t, "left", lt), (1 - t, "mid", x)]
        else:
            a = _share(rng, k, x, lt, lo)
            if a is None:
                return
            runs = [(t, "right" if end == "end" else "left", a)] + ([(1 - t, "mid", x - a)] if x - a else [])
        # (all runs of a read come from one gene; a read of the short kind keeps its k - 1 bases out of the count)
        m1, m2, info, _ = _pair(rng, genes, k, l1, l2, runs, before=ext, after=ext)
        cont = info[0][4] if end == "end" else info[0][3]
        nb = neighbour(t, end, cont, L1, L2)
        units.append([read(m1, m2), nb] if end == "end" else [nb, read(m1, m2)])
        marks.append([(0 if end == "end" else 1, t, end)])

    # (a leak may or may not count the leaked byte into len: the lengths are those at which thr is the same for len and len + 1,
    #  so that coverage thr - 1 + 1 passes either way)
    if threshold(c, L1 + L2 + 1) != threshold(c, L1 + L2):
        raise ValueError("at c = %r a read of %d bases one under the threshold does not pass with one base more" % (c, L1 + L2))
    for t in ((0, 1) if L2 else (0,)):
        Lt, Lo = (L1, L2) if t == 0 else (L2, L1)
        for end in ("end", "begin"):
            for _ in range(per_case):
                cuts = [d for d in range(1, min(40, Lt - k) + 1) if threshold(c, Lt - d + Lo + 1) == threshold(c, Lt - d + Lo)] if trimmed else [0]
                one(t, end, Lt - cuts[int(rng.integers(0, len(cuts)))], Lo)
        if trimmed:
            for _ in range(per_case):
                one(t, "end", k - 1, Lo, short=True)

    # the batch's own edges: the first read starts flush in both mates, the last ends flush in both
    def edge(end):
        x = threshold(c, L1 + L2) - 1
        at = "right" if end == "end" else "left"
        a = _share(rng, k, x, L1, L2) if L2 else x
        if L2 and a == x:
            a = int(rng.integers(max(k, x - L2), min(L1, x - k) + 1))
        runs = [(0, at, a)] + ([(1, at, x - a)] if L2 else [])
        m1, m2, info, _ = _pair(rng, genes, k, L1, L2, runs, before=ext, after=ext)
        side = 4 if end == "end" else 3
        return read(m1, m2), [info[0][side], info[1][side] if L2 else np.zeros(0, np.uint8)]

    first, lead = edge("begin")
    last, trail = edge("end")
    return units, marks, (first, lead, last, trail)


# ---------------------------------------------------------------------------
# batches
# ---------------------------------------------------------------------------
def reads_of(batch):
    """the reads of a SoA batch as tuples"""
    n = len(batch["off1"]) - 1
    paired = batch.get("seq2") is not None

    def cut(arr, off, i):
        return None if arr is None else np.asarray(arr[int(off[i]):int(off[i + 1])], dtype=np.uint8).copy()

    return [(cut(batch["seq1"], batch["off1"], i), cut(batch["seq2"], batch["off2"], i) if paired else None,
             cut(batch.get("qual1"), batch["off1"], i), cut(batch.get("qual2"), batch["off2"], i) if paired else None) for i in range(n)]


def batch_of(reads):
    """the SoA dict of tests/synth.py from reads (all of them paired or none, all with qualities or none)"""
    paired = reads[0][1] is not None
    qual = reads[0][2] is not None
    return synth.batch_from_lists([r[0] for r in reads], [r[1] for r in reads] if paired else None,
                                  [r[2] for r in reads] if qual else None, [r[3] for r in reads] if (qual and paired) else None)


def compose(rng, plain, units=(), marks=(), edges=None):
    """shuffle single reads and units (whose reads stay adjacent), put the edge reads first and last.
    Returns (batch, marked, lead, trail): marked = [(read index, mate, 'end' | 'begin')] of the hostile reads, lead / trail = the
    hostile bytes for embed (sequence arrays; the edge reads' marks are part of `marked`)"""
    items = [[r] for r in plain] + [list(u) for u in units]
    mk = [[] for _ in plain] + [list(m) for m in marks]
    order = rng.permutation(len(items))
    reads, marked = [], []
    lead = trail = None
    if edges is not None:
        first, lead, last, trail = edges
        reads.append(first)
        marked += [(0, t, "begin") for t in ((0, 1) if first[1] is not None else (0,))]
    for j in order:
        for i, t, end in mk[int(j)]:
            marked.append((len(reads) + i, t, end))
        reads += items[int(j)]
    if edges is not None:
        marked += [(len(reads), t, "end") for t in ((0, 1) if last[1] is not None else (0,))]
        reads.append(last)
    batch = batch_of(reads)
    return batch, marked, lead, trail


def neighbour_byte(batch, mark, lead=None, trail=None):
    """the byte of the buffer behind (before) the marked mate: the next (previous) read's, or the trail's (lead's)"""
    i, t, end = mark
    seq, off = (batch["seq1"], batch["off1"]) if t == 0 else (batch["seq2"], batch["off2"])
    p = int(off[i + 1]) if end == "end" else int(off[i]) - 1
    if p < 0:
        return int(lead[t][-1])
    if p >= len(seq):
        return int(trail[t][0])
    return int(seq[p])


# ---------------------------------------------------------------------------
# views
# ---------------------------------------------------------------------------
BYTE_ARRAYS = ("seq1", "seq2", "qual1", "qual2")
OFF_ARRAYS = ("off1", "off2")


def _aligned(n, dtype):
    """a zeroed array of n items that starts on a 64-byte boundary"""
    raw = np.zeros(n * np.dtype(dtype).itemsize + 64, np.uint8)
    skip = (-raw.ctypes.data) % 64
    return raw[skip:skip + n * np.dtype(dtype).itemsize].view(dtype)


def _fill(rng_bytes, n):
    return np.resize(rng_bytes, n) if n else np.zeros(0, np.uint8)


_FILLER = np.frombuffer(b"GATTACAGGCTTACGTCCAGTAACGGTCATGC", dtype=np.uint8)


def shifts_of(s1=0, s2=0, q1=0, q2=0, o1=0, o2=0):
    """displacements for embed: every byte array PAD + its shift (0 ... 3) into its larger array, the offsets arrays 0 or 8 bytes"""
    return {"seq1": PAD + s1, "seq2": PAD + s2, "qual1": PAD + q1, "qual2": PAD + q2, "off1": o1, "off2": o2}


def embed(batch, shifts, lead=None, trail=None):
    """every array of the batch inside a larger host array that starts on a 64-byte boundary.  shifts[name]: the byte displacement of the
    view -- for seq / qual any number >= the lead's length (shifts_of: PAD + 0 ... 3), for off1 / off2 0 or 8 (one leading
    element).  lead / trail = [bytes for seq1, bytes for seq2]: what lies right before and behind the sequence views (the
    qualities get phred 40 there: a leaked base would count); the rest of the surroundings is filler bases, PAD bytes at least
    on either side, so that every aligned 16 bytes around a byte of a view lies inside the array.  The offsets arrays are
    surrounded by POISON.  Returns {"arrays": {name: array or None}, "disp": {name: bytes}, "n": reads}."""
    arrays, disp = {}, {}
    for name in BYTE_ARRAYS:
        a = batch.get(name)
        if a is None:
            arrays[name], disp[name] = None, 0
            continue
        d = int(shifts[name])
        t = int(name[-1]) - 1
        is_q = name.startswith("qual")
        le = np.zeros(0, np.uint8) if lead is None else np.asarray(lead[t], np.uint8)
        tr = np.zeros(0, np.uint8) if trail is None else np.asarray(trail[t], np.uint8)
        assert d >= len(le) and d >= 16
        total = -(-(d + len(a) + max(len(tr), PAD) + 16) // 16) * 16
        big = _aligned(total, np.uint8)
        big[:] = HI_Q if is_q else _fill(_FILLER, total)
        if not is_q:
            big[d - len(le):d] = le
            big[d + len(a):d + len(a) + len(tr)] = tr
        big[d:d + len(a)] = a
        arrays[name], disp[name] = big, d
    for name in OFF_ARRAYS:
        a = batch.get(name)
        if a is None:
            arrays[name], disp[name] = None, 0
            continue
        d = int(shifts[name])
        assert d in (0, 8)
        big = _aligned(d // 8 + len(a) + 3, np.uint64)
        big[:] = POISON
        big[d // 8:d // 8 + len(a)] = np.asarray(a, np.uint64)
        arrays[name], disp[name] = big, d
    return {"arrays": arrays, "disp": disp, "n": len(batch["off1"]) - 1}


def view_of(embedded, name, length):
    """the `length` items of the view inside the larger array (what a kernel is handed)"""
    a, d = embedded["arrays"][name], embedded["disp"][name]
    return a[d // a.itemsize:d // a.itemsize + length]


def to_device(embedded, device="cuda:0"):
    """(tensors, pointers): the larger arrays as torch tensors on the device -- keep them alive until the results are read back --
    and per name the address of the view (0 for an array the batch does not have)"""
    import torch
    dev = torch.device(device)
    tensors, ptr = {}, {}
    for name, a in embedded["arrays"].items():
        if a is None:
            ptr[name] = 0
            continue
        t = torch.from_numpy(np.ascontiguousarray(a).view(np.int64) if a.dtype == np.uint64 else np.ascontiguousarray(a)).to(dev)
        assert t.data_ptr() % 16 == 0
        tensors[name] = t
        ptr[name] = t.data_ptr() + embedded["disp"][name]
    torch.cuda.synchronize()
    return tensors, ptr


def with_first_offset(batch, o1, o2, lead=None):
    """the same reads with off1[0] = o1, off2[0] = o2: o bytes in front of each byte array -- the end of lead[t] where given, gene-like
    filler before that -- which belong to no read"""
    out = dict(batch)
    for t, o in ((0, int(o1)), (1, int(o2))):
        s, q, f = "seq%d" % (t + 1), "qual%d" % (t + 1), "off%d" % (t + 1)
        if batch.get(s) is None or o == 0:
            continue
        front = _fill(_FILLER, o).copy()
        if lead is not None and len(lead[t]):
            le = np.asarray(lead[t], np.uint8)[-o:]
            front[o - len(le):] = le
        out[s] = np.concatenate([front, batch[s]])
        if batch.get(q) is not None:
            out[q] = np.concatenate([np.full(o, HI_Q, np.uint8), batch[q]])
        out[f] = np.asarray(batch[f], np.uint64) + np.uint64(o)
    return out


# ---------------------------------------------------------------------------
# the cases tests/test_views_cpu.py checks on the oracle and tests/test_gpu_views.py runs on the kernels
# ---------------------------------------------------------------------------
# (c, len): the exact product is an integer N; in fp64 it lies above N (a pair covering N is rejected), below it ((0.57, 300): N
# passes) or on it ((0.5, 252))
THRESHOLD_PAIRS = ((0.56, 300), (0.55, 200), (0.68, 150), (0.34, 300), (0.81, 300), (0.57, 300), (0.5, 252), (0.56, 600))
SHAPES = {300: (150, 150), 200: (100, 100), 150: (150, 0), 252: (151, 101), 600: (300, 300)}
PER_STEP = 2
K, C = 17, 0.56                           # what every route runs unless a case says otherwise

# The references and filters of the GPU file's routes: name -> (genes, filter bits, -q, shapes of the mixed batches).  Both test files
# take their batches from the tables below, so that the oracle is asked about exactly the reads the kernels see.
ROUTE_REFS = {
    "three-pairs+tiles": (1, 1 << 30, 0, ((150, 150), (151, 101))),
    "three-pairs": (1, 1 << 30, 0, ((150, 150), (151, 101))),
    "several-genes": (5, 1 << 30, 0, ((150, 150), (151, 101))),
    "exact-table-q": (1, 1 << 30, 20, ((150, 150), (151, 101))),
    "class-by-class": (1, 1 << 30, 0, ((150, 150), (151, 101))),
    "lds-summary": (1, 1 << 30, 0, ((150, 150), (151, 101))),
    "summary+table": (6, 1 << 26, 0, ((150, 150), (151, 101))),
    "table": (6, 1 << 26, 0, ((150, 150), (151, 101))),
    "table-q": (6, 1 << 26, 20, ((150, 150), (151, 101))),
    "table-mod": (6, 3 << 24, 0, ((150, 150), (151, 101))),
    "table-mod-q": (6, 3 << 24, 20, ((150, 150), (151, 101))),
    "bit-vector": (6, 1 << 26, 0, ((150, 150), (151, 101))),
    "2x300": (1, 1 << 30, 0, ((300, 300),)),
    "2x300-table": (6, 1 << 26, 0, ((300, 300),)),
}
INVALID_RAGGED = ((False, False), (True, False), (False, True), (True, True))
STALE_ROUTES = ("three-pairs", "class-by-class", "table", "table-q")          # test_stale_bytes_behind_a_host_batch (mixed batches of seed 5)
EVIDENCE_ROUTES = {1: ("three-pairs", "exact-table-q"), 6: ("table-q", "table-mod"), 5: ("several-genes",)}
EVIDENCE_PAIRS = tuple((17, c, n) for c, n in THRESHOLD_PAIRS) + ((31, 0.56, 300), (31, 0.5, 252))


def pairs_of(name):
    """the (c, len) pairs a route runs: (0.56, 300) everywhere, the others in turn (every pair on three routes at least); the 2 x 300
    routes their own"""
    if ROUTE_REFS[name][3] == ((300, 300),):
        return [(0.56, 600)]
    j = list(ROUTE_REFS).index(name)
    rest = [p for p in THRESHOLD_PAIRS if p not in ((0.56, 300), (0.56, 600))]
    return [(0.56, 300)] + [rest[(2 * j + i) % len(rest)] for i in range(2)]


def threshold_cases(name):
    """test_exact_thresholds_on_every_route: [(k, c, len, invalid, ragged)] of a route"""
    return [(K, c, n, inv, rag) for c, n in pairs_of(name) for inv, rag in INVALID_RAGGED]


def evidence_cases(k, c, length):
    """test_exact_thresholds_in_evidence_mode: [(route, invalid, ragged)] of a (k, c, len); the references of several genes run two pairs"""
    names = EVIDENCE_ROUTES[1] + (EVIDENCE_ROUTES[6] + EVIDENCE_ROUTES[5] if (k, c, length) in ((17, 0.56, 300), (17, 0.5, 252)) else ())
    return [(name, inv, rag) for name in names for inv, rag in ((False, False), (True, True))]


def all_ladder_cases():
    """every ladder batch the GPU file runs, once: [(genes, filter bits, -q, k, c, len, invalid, ragged)]"""
    out = set()
    for name, (g, bf, q, _) in ROUTE_REFS.items():
        out |= {(g, bf, q) + case for case in threshold_cases(name)}
    for k, c, n in EVIDENCE_PAIRS:
        for name, inv, rag in evidence_cases(k, c, n):
            out.add(ROUTE_REFS[name][:3] + (k, c, n, inv, rag))
    return sorted(out)


def all_mixed_cases():
    """every mixed batch the GPU file runs, once: [(genes, filter bits, -q, L1, L2, trimmed, seed)] (k = K, c = C)"""
    out = set()
    for name, (g, bf, q, shapes) in ROUTE_REFS.items():
        out |= {(g, bf, q, L1, L2, tr, 1) for L1, L2 in shapes for tr in (False, True)}
    for name in STALE_ROUTES:
        out |= {ROUTE_REFS[name][:3] + (150, 150, tr, 5) for tr in (False, True)}
    return sorted(out)


def reference(n_genes, seed=20260):
    """a few genes of 1 to 3 kb"""
    return synth.make_genes(np.random.default_rng(seed + n_genes), n_genes, 1000, 3000)


def ladder_case(genes, k, c, length, qual=False, invalid=False, ragged=False, per_step=PER_STEP):
    """the ladder batch of one (c, len) pair: (batch, design).  ragged: a second ladder of shorter mates (another len, another
    thr) rides along, so that the batch has several lengths per mate."""
    L1, L2 = SHAPES[length]
    rng = np.random.default_rng([int(round(c * 100)), length, k, int(qual), int(invalid), int(ragged), len(genes)])
    gen = ladder_with_invalid if invalid else ladder
    reads, design = gen(rng, genes, k, L1, L2, c, per_step, qual=qual)
    if ragged:
        r2, d2 = gen(rng, genes, k, L1 - 7, L2 - 12 if L2 else 0, c, per_step, qual=qual)
        # ... and one of mates cut so that one base more in len moves thr: a byte behind the mate's end counted as valid shows
        d = [d for d in range(1, 24) if (L1 - d) % 8 and threshold(c, L1 - d + L2 + 1) != threshold(c, L1 - d + L2)]
        r3, d3 = gen(rng, genes, k, L1 - d[0], L2, c, per_step, qual=qual) if d else ([], [])
        order = rng.permutation(len(reads) + len(r2) + len(r3))
        reads, design = [(reads + r2 + r3)[int(j)] for j in order], [(design + d2 + d3)[int(j)] for j in order]
    return batch_of(reads), design


def mixed_case(genes, k, c, L1, L2, n_plain=300, qual=False, trimmed=False, seed=1):
    """the batch of test_resident_views_on_every_route: ordinary reads (70 % on target), a ladder, hostile reads next to their
    neighbours, shuffled, the batch's first and last read hostile to what embed puts around the arrays.
    Returns (batch, marked, lead, trail)."""
    rng = np.random.default_rng([seed, k, L1, L2, int(round(c * 100)), int(qual), int(trimmed), len(genes)])
    plain = reads_of(synth.make_reads(rng, genes, n_plain, read_len=max(L1, L2), paired=L2 > 0, on_target=0.7, qual=qual, var_len=trimmed))
    if not trimmed and L1 != L2 and L2:
        plain = [(r[0][:L1], r[1][:L2], None if r[2] is None else r[2][:L1], None if r[3] is None else r[3][:L2]) for r in plain]
    lad, _ = ladder(rng, genes, k, L1, L2, c, 1, qual=qual)
    units, marks, edges = hostile(rng, genes, k, L1, L2, c, per_case=3, trimmed=trimmed, qual=qual)
    return compose(rng, plain + lad, units, marks, edges)
