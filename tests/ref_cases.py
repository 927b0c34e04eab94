"""Whole-program cases for the reference shark: input builders, the npz layout of
tests/golden/ref_shark_cases.npz, and helpers that run a shark-like CLI on a case
and turn its ssv into per-read gene lists.

Used by tests/golden/gen_ref_shark_cases.py (which records the reference CLI's
answers) and by the tests that replay them (oracle, GPU) or compare the oracle
with the reference live on fresh draws.

Inputs are kept to what the reference defines: printable ASCII only (no byte
>= 0x80, no NUL), quality lines as long as their sequence, and in reads that a
-q mask can touch only letters (the mask subtracts 64 from a base, and the
reference then indexes `to_int` with the result)."""
import os
import subprocess

import numpy as np

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CASES_NPZ = os.path.join(GOLD, "ref_shark_cases.npz")

BLOBS = ("fasta", "fq1", "fq2", "ssv", "out1", "out2")
GIB_BITS = 1 << 33                      # -b 1

_RC = bytes.maketrans(b"ACGTacgtRYKMBVDHrykmbvdh", b"TGCAtgcaYRMKVBHDyrmkvbhd")
_IUPAC = b"RYKMSWBDHVN"


def revcomp(s):
    return s.translate(_RC)[::-1]


def rseq(rng, n):
    return np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, n)].tobytes()


# ---------------------------------------------------------------------------
# references
# ---------------------------------------------------------------------------
def make_genes(rng, n, lo, hi, k, features=()):
    """[(name, description, seq)]: random genes (each with a palindrome of k//2 + k//2 bases, a palindromic k-mer for even k)
    plus the requested features"""
    genes = []
    for i in range(n):
        s = rseq(rng, int(rng.integers(lo, hi + 1)))
        h = max(k // 2, 1)
        p = rseq(rng, h)
        at = int(rng.integers(0, len(s) + 1))
        s = s[:at] + p + revcomp(p) + s[at:]
        genes.append(["g%d" % i, "", s])
    a = genes[0][2]
    if "ties" in features:                              # shared halves, an exact copy
        half = len(a) // 2
        genes.append(["half1", "first half of g0", a[:half] + rseq(rng, half)])
        genes.append(["half2", "", rseq(rng, half) + a[half:]])
        genes.append(["copy0", "", a])
    if "revcomp" in features:
        genes.append(["rc0", "reverse complement of g0", revcomp(a)])
    if "contained" in features:
        st = len(a) // 4
        genes.append(["in0", "", a[st:st + max(len(a) // 3, k + 5)]])
        r = rseq(rng, 40 + k)
        genes.append(["rep", "repeat inside", rseq(rng, 50) + r + rseq(rng, 7) + r + r + rseq(rng, 30)])
    if "quirk" in features:                             # records without a k-mer still take a gene number
        genes.insert(1, ["short", "", rseq(rng, max(k - 1, 0))])
        genes.insert(3, ["alln", "", b"N" * (2 * k + 3)])
        genes.insert(4, ["empty", "", b""])
        genes.append(["nsplit", "", b"N".join(rseq(rng, max(k - 1, 1)) for _ in range(6))])
    if "dirty" in features:
        for g in genes[: max(2, len(genes) // 2)]:
            if not g[2]:
                continue
            s = bytearray(g[2])
            for _ in range(max(1, len(s) // 60)):
                j = int(rng.integers(0, len(s)))
                m = int(rng.integers(0, 3))
                if m == 0:
                    s[j:j + 30] = bytes(s[j:j + 30]).lower()
                elif m == 1:
                    s[j] = _IUPAC[int(rng.integers(0, len(_IUPAC)))]
                else:
                    s[j] = ord(".")
            g[2] = bytes(s)
    return [tuple(g) for g in genes]


def fasta_bytes(genes, width=0, rng=None):
    """FASTA text; width > 0 wraps sequences (multi-line records); width < 0 draws a width per record"""
    out = []
    for name, desc, s in genes:
        out.append(b">" + name.encode() + ((b" " + desc.encode()) if desc else b"") + b"\n")
        w = width if width >= 0 else int(rng.choice([7, 13, 60, 61, 80]))
        if w and s:
            out.extend(s[i:i + w] + b"\n" for i in range(0, len(s), w))
        else:
            out.append(s + b"\n")
    return b"".join(out)


def parse_fasta(data):
    """[(name, seq)] as kseq.h reads them: name up to the first whitespace, sequence lines joined"""
    recs = []
    for chunk in data.split(b"\n>"):
        if not chunk:
            continue
        if chunk.startswith(b">"):
            chunk = chunk[1:]
        lines = chunk.split(b"\n")
        head = lines[0].split()
        recs.append((head[0] if head else b"", b"".join(l.rstrip(b"\r") for l in lines[1:])))
    return recs


# ---------------------------------------------------------------------------
# reads
# ---------------------------------------------------------------------------
def _mutate(rng, s, sub, lower, nrate):
    s = bytearray(s)
    for j in np.flatnonzero(rng.random(len(s)) < sub):
        s[j] = b"ACGT"[int(rng.integers(0, 4))]
    for j in np.flatnonzero(rng.random(len(s)) < nrate):
        s[j] = ord("N")
    if lower and len(s) > 4:
        j = int(rng.integers(0, len(s) - 3))
        w = int(rng.integers(3, 40))
        s[j:j + w] = bytes(s[j:j + w]).lower()
    return bytes(s)


def _segment(rng, g, L):
    if L == 0:
        return b""
    if len(g) <= L:
        return g + rseq(rng, L - len(g))
    st = int(rng.integers(0, len(g) - L + 1))
    return g[st:st + L]


def _edge_read(rng, k, L):
    """reads that end up with fewer than k valid bases, or whose k-mers are cut by N"""
    m = int(rng.integers(0, 6))
    if m == 0:
        return b""
    if m == 1:
        return rseq(rng, int(rng.integers(1, k + 1)))[: max(k - 1, 0)]
    if m == 2:                                          # >= k bytes, < k valid
        s = bytearray(rseq(rng, k + 3))
        for j in rng.choice(len(s), 4, replace=False):
            s[j] = ord("N")
        return bytes(s)
    if m == 3:                                          # N runs: pieces shorter than k
        piece = max(k - 1, 1)
        return b"NN".join(rseq(rng, int(rng.integers(1, piece + 1))) for _ in range(int(rng.integers(2, 8))))
    if m == 4:
        return b"N" + rseq(rng, max(L - 2, k)) + b"N"
    return b"n" * int(rng.integers(1, 3)) + rseq(rng, max(L, k))


def make_reads(rng, genes, n, k, lengths, paired, q_active, mq, cfrac=None, p_edge=0.1, p_off=0.1, p_chim=0.1, sub=0.01,
               uniform=None):
    """[(name1, seq1, qual1, name2, seq2, qual2)] -- mate-2 fields are None when single-end.
    cfrac: reads are a clean gene segment of about cfrac * length followed by off-target bases (c thresholds).
    uniform: (L1, L2) -- every mate 1 has L1 bases and every mate 2 L2 (a uniform batch); edge reads are cut or padded
    with N to that length."""
    seqs = [g[2] for g in genes if len(g[2]) >= max(k, 1)] or [rseq(rng, 200)]
    reads = []
    for i in range(n):
        L = int(rng.choice(lengths))
        L2 = L if rng.random() < 0.7 else int(rng.choice(lengths))
        if uniform:
            L, L2 = uniform
        g = seqs[int(rng.integers(0, len(seqs)))]
        u = rng.random()
        if cfrac is not None:
            m = int(round(cfrac * L)) + int(rng.integers(-1, 2))
            m = min(max(m, 0), L)
            s1 = _segment(rng, g.upper(), m) + rseq(rng, L - m)
            s2 = _segment(rng, g.upper(), min(L2, m)) if paired else None
        elif u < p_edge:
            s1 = _edge_read(rng, k, L)
            s2 = _edge_read(rng, k, L2) if paired else None
        elif u < p_edge + p_off:
            s1, s2 = rseq(rng, L), (rseq(rng, L2) if paired else None)
        elif u < p_edge + p_off + p_chim:
            h = seqs[int(rng.integers(0, len(seqs)))]
            cut = int(rng.integers(0, L + 1))
            s1 = _segment(rng, g, cut) + _segment(rng, h, L - cut)
            s2 = revcomp(_segment(rng, h, L2)) if paired else None
        else:
            frag = _segment(rng, g, L + L2 + int(rng.integers(0, 50)))
            s1 = frag[:L]
            s2 = revcomp(frag)[:L2] if paired else None
            if rng.random() < 0.5:
                s1, s2 = revcomp(s1), (revcomp(s2) if paired else None)
            s1 = _mutate(rng, s1, sub, rng.random() < 0.2, 0.004)
            if paired:
                s2 = _mutate(rng, s2, sub, rng.random() < 0.2, 0.004)
            if rng.random() < 0.05 and len(s1):
                s1 = b"N" + s1[1:] if rng.random() < 0.5 else s1[:-1] + b"N"
        if uniform:
            s1 = s1[:L] + b"N" * (L - len(s1))
            s2 = (s2[:L2] + b"N" * (L2 - len(s2))) if paired else None
        elif paired and rng.random() < 0.03:
            s2 = b""
        if q_active:                                    # a masked byte below '@' would index to_int below 0
            s1, s2 = s1.replace(b".", b"N"), (s2.replace(b".", b"N") if paired else None)
        q1 = _quals(rng, len(s1), q_active, mq)
        q2 = _quals(rng, len(s2), q_active, mq) if paired else None
        tag = b" 1:N:0:ACGT" if i % 7 == 3 else b""
        reads.append((b"r%d/1" % i + tag, s1, q1, (b"r%d/2" % i + tag) if paired else None, s2, q2))
    return reads


def _quals(rng, n, q_active, mq):
    """constant 'I' without -q; with it, some reads entirely on the threshold (kept: DEL, 0x7F, when the threshold is 127),
    the others mostly on the threshold or one above (kept), some one below (masked) and some anywhere in '!'..'~'"""
    if not q_active:
        return b"I" * n
    if rng.random() < 0.15:
        return bytes([mq if 34 <= mq <= 127 else 126]) * n
    q = rng.integers(33, 127, n)
    if 34 <= mq <= 126:
        u = rng.random(n)
        q = np.where(u < 0.9, mq + (u < 0.45), np.where(u < 0.95, mq - 1, q))
    return np.minimum(q, 126).astype(np.uint8).tobytes()


def fastq_bytes(reads, mate):
    out = []
    for r in reads:
        name, s, q = (r[0], r[1], r[2]) if mate == 1 else (r[3], r[4], r[5])
        out.append(b"@" + name + b"\n" + s + b"\n+\n" + q + b"\n")
    return b"".join(out)


def parse_fastq(data):
    """[(id, seq, qual)] from 4-line FASTQ (the only layout the cases use)"""
    lines = data.split(b"\n")
    recs = []
    for i in range(0, len(lines) - 3, 4):
        h = lines[i][1:].split()
        recs.append((h[0] if h else b"", lines[i + 1], lines[i + 3]))
    return recs


def threshold(q):
    """the reference's (char)(q + 33), as an int in [-128, 127]; None when (char)q == 0 (no mask)"""
    c = ((q & 0xFF) ^ 0x80) - 0x80
    if c == 0:
        return None
    return (((c + 33) & 0xFF) ^ 0x80) - 0x80


# ---------------------------------------------------------------------------
# cases, the npz layout, running a CLI
# ---------------------------------------------------------------------------
def case(name, genes, reads, k, c, q=0, single=False, bf_bits=1 << 20, paired=None, fasta_width=0, rng=None):
    paired = reads[0][3] is not None if reads else bool(paired)
    return {"name": name, "k": k, "c": repr(float(c)), "q": q, "single": bool(single), "bf_bits": int(bf_bits),
            "paired": paired, "fasta": fasta_bytes(genes, fasta_width, rng),
            "fq1": fastq_bytes(reads, 1), "fq2": fastq_bytes(reads, 2) if paired else b""}


def cli_args(cs, workdir, bits_flag):
    """command-line arguments for case cs, files written into workdir.  bits_flag: how to ask for an exact filter size
    (None: `-b 1` cases only; otherwise e.g. "--bf-bits")"""
    paths = {x: os.path.join(workdir, x) for x in ("ref.fa", "s1.fq", "s2.fq", "o1.fq", "o2.fq")}
    with open(paths["ref.fa"], "wb") as f:
        f.write(cs["fasta"])
    with open(paths["s1.fq"], "wb") as f:
        f.write(cs["fq1"])
    args = ["-t", "1", "-r", paths["ref.fa"], "-1", paths["s1.fq"], "-o", paths["o1.fq"], "-k", str(cs["k"]), "-c", cs["c"]]
    if cs["paired"]:
        with open(paths["s2.fq"], "wb") as f:
            f.write(cs["fq2"])
        args += ["-2", paths["s2.fq"], "-p", paths["o2.fq"]]
    if cs["q"]:
        args += ["-q", str(cs["q"])]
    if cs["single"]:
        args += ["-s"]
    if cs["bf_bits"] == GIB_BITS:
        args += ["-b", "1"]
    elif bits_flag:
        args += [bits_flag, str(cs["bf_bits"])]
    return args, paths


def run_case(exe, cs, workdir, bits_flag=None, env_bits=None, timeout=120):
    """run a shark-like CLI on case cs -> (ssv, out1, out2) bytes.  env_bits: name of an environment variable that carries the
    exact filter size (the reference wrapper's REF_BF_BITS)"""
    args, paths = cli_args(cs, workdir, bits_flag)
    for p in (paths["o1.fq"], paths["o2.fq"]):
        if os.path.exists(p):
            os.remove(p)
    env = dict(os.environ)
    if env_bits:
        env.pop(env_bits, None)
        if cs["bf_bits"] != GIB_BITS:
            env[env_bits] = str(cs["bf_bits"])
    r = subprocess.run([exe] + args, capture_output=True, env=env, timeout=timeout)
    if r.returncode != 0:
        raise RuntimeError("%s failed on case %s (%d): %s" % (exe, cs["name"], r.returncode, r.stderr.decode()[-800:]))

    def rd(p):
        return open(p, "rb").read() if os.path.exists(p) else b""
    return r.stdout, rd(paths["o1.fq"]), rd(paths["o2.fq"]) if cs["paired"] else b""


def save(cases, path=CASES_NPZ):
    arrs = {}
    for b in BLOBS:
        parts = [cs[b] for cs in cases]
        arrs[b] = np.frombuffer(b"".join(parts), np.uint8)
        arrs[b + "_off"] = np.cumsum([0] + [len(p) for p in parts]).astype(np.int64)
    arrs["name"] = np.array([cs["name"] for cs in cases])
    arrs["k"] = np.array([cs["k"] for cs in cases], np.uint8)
    arrs["c"] = np.array([cs["c"] for cs in cases])
    arrs["q"] = np.array([cs["q"] for cs in cases], np.int32)
    arrs["single"] = np.array([cs["single"] for cs in cases], np.uint8)
    arrs["paired"] = np.array([cs["paired"] for cs in cases], np.uint8)
    arrs["bf_bits"] = np.array([cs["bf_bits"] for cs in cases], np.uint64)
    np.savez_compressed(path, **arrs)


def load(path=CASES_NPZ):
    z = np.load(path)
    cases = []
    for i in range(len(z["k"])):
        cs = {"name": str(z["name"][i]), "k": int(z["k"][i]), "c": str(z["c"][i]), "q": int(z["q"][i]),
              "single": bool(z["single"][i]), "paired": bool(z["paired"][i]), "bf_bits": int(z["bf_bits"][i])}
        for b in BLOBS:
            o = z[b + "_off"]
            cs[b] = z[b][o[i]:o[i + 1]].tobytes()
        cases.append(cs)
    return cases


def associations(cs, ssv=None):
    """per read (in file order) the list of gene numbers of the ssv's lines for it; a gene's number is the position of the
    first FASTA record with its name (legend_ID, ReadAnalyzer.hpp:106)"""
    ssv = cs["ssv"] if ssv is None else ssv
    legend = {}
    for i, (nm, _) in enumerate(parse_fasta(cs["fasta"])):
        legend.setdefault(nm, i)
    lines = [l.split(b" ") for l in ssv.split(b"\n") if l]
    reads = parse_fastq(cs["fq1"])
    out, j = [], 0
    for rid, _, _ in reads:
        genes = []
        while j < len(lines) and lines[j][0] == rid:
            genes.append(legend[lines[j][1]])
            j += 1
        out.append(genes)
    assert j == len(lines), "ssv line %d does not follow the read order" % j
    return out


def batch(cs):
    """the case's reads as a host SoA batch (the layout of the C ABI and of the oracle's batch API)"""
    from tests import synth
    r1 = parse_fastq(cs["fq1"])
    r2 = parse_fastq(cs["fq2"]) if cs["paired"] else None
    return synth.batch_from_lists([s for _, s, _ in r1], [s for _, s, _ in r2] if r2 else None,
                                  [q for _, _, q in r1], [q for _, _, q in r2] if r2 else None)


def render(cs, per_read):
    """ssv and both FASTQ outputs for per-read gene lists, as ReadOutput.hpp writes them (one batch of < 50 000 reads)"""
    names = [nm for nm, _ in parse_fasta(cs["fasta"])]
    r1 = parse_fastq(cs["fq1"])
    r2 = parse_fastq(cs["fq2"]) if cs["paired"] else None
    ssv, o1, o2 = [], [], []
    previd = b""
    for i, genes in enumerate(per_read):
        for g in genes:
            ssv.append(r1[i][0] + b" " + names[g] + b"\n")
            if previd != r1[i][0]:
                o1.append(b"@%s\n%s\n+\n%s\n" % r1[i])
                if r2:
                    o2.append(b"@%s\n%s\n+\n%s\n" % r2[i])
            previd = r1[i][0]
    return b"".join(ssv), b"".join(o1), b"".join(o2)
