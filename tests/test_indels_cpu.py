"""Indels mode without a GPU: the model's left-normalisation (tests/indels_model.py) against brute force over haplotype strings; the
planted-truth probe through the model chain (segments -> alignments -> indels); the rules on records worked out by hand, one each;
and the boundary -- the new symbols in the header, the binding and the library."""
import itertools
import os
import re
import subprocess

import numpy as np

from shark_amd import capi
from tests import synth
from tests.indels_cases import planted_probe
from tests.indels_model import (MAX_INS, check_entry, expected_indels, indel_lines, new_stats, pack, record_events, shift_left, table_array,
                                unpack)
from tests.align_model import expected_alignments, record_codes
from tests.segments_model import SegmentsModel, expected_segments

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "shark_amd", "libsharkhip.so")
CODE = {ord("A"): 0, ord("C"): 1, ord("G"): 2, ord("T"): 3}


def _rc(b):
    return bytes(synth.revcomp(np.frombuffer(bytes(b), np.uint8)))


def _record(seed, n):
    return bytes(synth.random_seq(np.random.default_rng(seed), n))


def _rec(strand, *blocks):
    """one capi.ALIGNMENT_DTYPE record with these blocks (x, q, len); the counts play no part here"""
    out = np.zeros((), dtype=capi.ALIGNMENT_DTYPE)
    out["n_blocks"], out["strand"] = len(blocks), strand
    for r, b in enumerate(blocks):
        out["block"][r] = b
    return out


def _events(rec, mate, record, min_intron=20):
    stats, shifts = new_stats(), []
    ev = record_events(rec, mate, record, min_intron, stats, shifts)
    return ev, {k: v for k, v in stats.items() if v}, shifts


def _seq(letters):
    return pack([CODE[c] for c in letters.encode()])


# ---------------------------------------------------------------------------
# normalisation against brute force
# ---------------------------------------------------------------------------
def _haplotype(record, kind, x, length, letters=b""):
    return record[:x] + (letters + record[x:] if kind else record[x + length:])


def test_normalisation_against_brute_force():
    """records of at most 40 bases over {A, C, N}, every deletion and every insertion over {A, C} of at most 3 bases at every position:
    the normalised event spells the raw one's haplotype, and an event further left spells it only across an N"""
    rng = np.random.default_rng(11)
    records = [b"A" * 7, b"AC" * 9 + b"A", b"CCNCCCC", b"ACACNACACAC", b"C"]
    for _ in range(40):
        n = int(rng.integers(2, 41))
        unit = bytes(rng.choice(np.frombuffer(b"AC", np.uint8), size=int(rng.integers(1, 4))))
        r = bytearray(rng.choice(np.frombuffer(b"AACCN", np.uint8), size=n).tobytes())
        a = int(rng.integers(0, n))
        r[a:] = (unit * n)[:n - a] if rng.random() < 0.7 else r[a:]              # (a repeat of period 1 .. 3 behind a random head)
        if rng.random() < 0.3:
            r[int(rng.integers(0, n))] = ord("N")
        records.append(bytes(r))
    checked = moved = 0
    for record in records:
        rc = record_codes(record)
        n = len(record)
        for length in (1, 2, 3):
            events = [(0, x, b"") for x in range(0, n - length + 1)]
            events += [(1, x, bytes(s)) for x in range(n) for s in itertools.product(b"AC", repeat=length)]
            for kind, x, letters in events:
                want = _haplotype(record, kind, x, length, letters)
                nx, ns, d = shift_left(kind, x, length, [CODE[c] for c in letters], rc)
                nl = bytes(b"ACGT"[b] for b in ns)
                assert nx == x - d and _haplotype(record, kind, nx, length, nl) == want, (record, kind, x, length, letters)
                for y in range(nx):                                              # further left: only across an N
                    cand = want[y:y + length] if kind else b""
                    if _haplotype(record, kind, y, length, cand) == want:
                        assert b"N" in record[y:nx], (record, kind, x, length, letters, y)
                checked += 1
                moved += d > 0
    print("events", checked, "moved", moved)
    assert checked > 10000 and moved > 2000


# ---------------------------------------------------------------------------
# planted truth through the model chain
# ---------------------------------------------------------------------------
def test_planted_truth_through_the_model_chain():
    """one 700-base record; the sample carries an A more in A x 8 at [200, 208), one CAG less in CAG x 4 at [400, 412) and GATTACA in
    front of base 550; error-free 100-base mates every 3 bases on alternating strands, k = 17, s_min = 8"""
    record, batch = planted_probe()
    sm = SegmentsModel([record], 17)
    n = len(batch["off1"]) - 1
    goff, gids = np.arange(n + 1, dtype=np.uint32), np.zeros(n, dtype=np.uint16)
    rows = expected_segments(sm, batch, goff, gids, 4)[1]
    recs = expected_alignments(sm, batch, goff, gids, rows, 8)
    shifts = []
    table, stats = expected_indels(recs, batch, goff, gids, sm.records, 20, shifts=shifts)
    print(stats, table)
    # every gap the chain shows is pure
    assert stats["complex_gaps"] == 0 and stats["long_insertions"] == 0 and stats["nonbase_insertions"] == 0
    assert sorted(table) == [(0, 200, 1, 1, _seq("A")), (0, 400, 0, 3, 0), (0, 550, 1, 7, _seq("GATTACA"))]
    # the raw events sit at the right end of their repeats (208, 409 behind the three units the sample has left, 551): the shifts
    assert sorted(set(shifts)) == [1, 8, 9]
    # fwd + rev = the mates whose records show the gap
    shown = {1: 0, 3: 0, 7: 0}
    for r in recs[:, 0]:
        for b in range(int(r["n_blocks"]) - 1):
            (xA, qA, lA), (xB, qB, lB) = r["block"][b], r["block"][b + 1]
            R, G = int(qB) - int(qA + lA), int(xB) - int(xA + lA)
            assert (R, G) in ((1, 0), (0, 3), (7, 0))
            shown[R + G] += 1
    assert [sum(table[key]) for key in sorted(table)] == [shown[1], shown[3], shown[7]] and min(shown.values()) >= 10
    assert all(f >= 3 and r >= 3 for f, r in table.values())                     # both strands see each
    assert stats["insertions"] == shown[1] + shown[7] and stats["deletions"] == shown[3] and stats["mates"] == int((recs["n_blocks"] >= 1).sum())
    assert indel_lines(table_array(table, 2), {0: "g"}) == ["g 200 I 1 A %d %d" % tuple(table[(0, 200, 1, 1, 0)]),
                                                            "g 400 D 3 * %d %d" % tuple(table[(0, 400, 0, 3, 0)]),
                                                            "g 550 I 7 GATTACA %d %d" % tuple(table[(0, 550, 1, 7, _seq("GATTACA"))])]


# ---------------------------------------------------------------------------
# the rules on records worked out by hand
# ---------------------------------------------------------------------------
REC = _record(3, 300)


def _unique_ins(n, x=60):
    """n inserted bases in front of REC[x] that cannot move: the last one differs from REC[x - 1]"""
    ins = bytearray(_record(40 + n, n))
    ins[-1] = next(c for c in b"ACGT" if c != REC[x - 1])
    return bytes(ins)


def test_insertion_of_12_is_tabled_13_is_long():
    for n, want in ((12, "insertions"), (13, "long_insertions")):
        ins = _unique_ins(n)
        mate = REC[10:60] + ins + REC[60:100]
        ev, stats, _ = _events(_rec(0, (10, 0, 50), (60, 50 + n, 40)), mate, REC)
        assert stats == {"mates": 1, want: 1}
        assert ev == ([(60, 1, 12, _seq(ins.decode()))] if n == 12 else [])
    assert MAX_INS == capi.SHK_INDEL_MAX_INS == 12


def test_insertion_with_an_N_and_with_a_masked_base(oracle):
    ins = bytearray(_unique_ins(5))
    clean = REC[10:60] + bytes(ins) + REC[60:100]
    rec = _rec(0, (10, 0, 50), (60, 55, 40))
    assert _events(rec, clean, REC)[1] == {"mates": 1, "insertions": 1}
    ins[2] = ord("N")
    ev, stats, _ = _events(rec, REC[10:60] + bytes(ins) + REC[60:100], REC)
    assert ev == [] and stats == {"mates": 1, "nonbase_insertions": 1}
    # the same clean mate with base 52 (inside the insertion) below -q 20: masked_mates hands the model a byte that is no base
    qual = np.full(len(clean), 33 + 30, dtype=np.uint8)
    qual[52] = 33 + 5
    batch = synth.batch_from_lists([clean], None, [qual])
    recs = np.zeros((1, 2), dtype=capi.ALIGNMENT_DTYPE)
    recs[0, 0] = rec
    table, stats = expected_indels(recs, batch, [0, 1], [0], {0: REC}, 20, min_quality=20)
    assert table == {} and stats["nonbase_insertions"] == 1 and stats["insertions"] == 0
    table, stats = expected_indels(recs, batch, [0, 1], [0], {0: REC}, 20, min_quality=0)
    assert list(table.values()) == [[1, 0]] and stats["insertions"] == 1


def test_deletion_below_min_intron_is_tabled_at_min_intron_not():
    for G, tabled in ((19, True), (20, False)):
        record = bytearray(REC)
        record[59], record[60 + G - 1] = ord("A"), ord("C")                      # (the deletion cannot move)
        ev, stats, _ = _events(_rec(0, (10, 0, 50), (60 + G, 50, 40)), bytes(record[10:60] + record[60 + G:100 + G]), bytes(record), 20)
        assert ev == ([(60, 0, 19, 0)] if tabled else []) and stats == ({"mates": 1, "deletions": 1} if tabled else {"mates": 1})
    # at min_intron 65535 a deletion of 65534 record bases is one; the length fits 16 bits
    big = _record(5, 66000)
    ev, stats, _ = _events(_rec(0, (0, 0, 50), (50 + 65534, 50, 40)), big[:50] + big[50 + 65534:90 + 65534], big, 65535)
    assert stats["deletions"] == 1 and ev[0][1:3] == (0, 65534)


def test_complex_gap_and_touching_blocks():
    mate = REC[10:60] + b"ACG" + REC[62:100]
    assert _events(_rec(0, (10, 0, 50), (62, 53, 38)), mate, REC) == ([], {"mates": 1, "complex_gaps": 1}, [])
    assert _events(_rec(0, (10, 0, 50), (60, 50, 40)), REC[10:100], REC) == ([], {"mates": 1}, [])
    # three blocks: a deletion, then blocks that touch in read and record
    record = bytearray(REC)
    record[29], record[31] = ord("A"), ord("C")
    record = bytes(record)
    ev, stats, _ = _events(_rec(0, (10, 0, 20), (32, 20, 20), (52, 40, 30)), record[10:30] + record[32:82], record)
    assert ev == [(30, 0, 2, 0)]
    assert stats == {"mates": 1, "deletions": 1}


def test_a_shift_stops_at_base_0_and_at_a_record_N():
    record = b"A" * 30 + _record(8, 100).replace(b"A", b"C")
    mate = b"A" * 31 + record[30:90]
    ev, _, shifts = _events(_rec(0, (0, 0, 30), (30, 31, 60)), mate, record)
    assert ev == [(0, 1, 1, 0)] and shifts == [30]
    ev, _, shifts = _events(_rec(0, (0, 0, 28), (30, 28, 60)), b"A" * 28 + record[30:90], record)
    assert ev == [(0, 0, 2, 0)] and shifts == [28]
    record = record[:12] + b"N" + record[13:]
    ev, _, shifts = _events(_rec(0, (0, 0, 30), (30, 31, 60)), b"A" * 12 + b"N" + b"A" * 18 + record[30:90], record)
    assert ev == [(13, 1, 1, 0)] and shifts == [17]
    ev, _, shifts = _events(_rec(0, (0, 0, 28), (30, 28, 60)), record[:28] + record[30:90], record)
    assert ev == [(13, 0, 2, 0)] and shifts == [15]


def test_repeat_runs_across_the_64_per_pass_edge():
    """runs of 63, 64, 65 and 130 bases in front of the event: the kernel compares 64 positions per pass"""
    for run in (63, 64, 65, 130):
        head, tail = b"GTGTC", _record(9, 60).replace(b"A", b"C")
        record = head + b"A" * run + tail
        xa = len(head) + run
        ev, _, shifts = _events(_rec(0, (0, 0, xa), (xa, xa + 1, 60)), head + b"A" * (run + 1) + tail, record)
        assert ev == [(5, 1, 1, 0)] and shifts == [run]
        ev, _, shifts = _events(_rec(0, (0, 0, xa - 3), (xa, xa - 3, 60)), head + b"A" * (run - 3) + tail, record)
        assert ev == [(5, 0, 3, 0)] and shifts == [run - 3]


def test_a_two_base_unit_into_40_units():
    """the shift exceeds R: the comparison passes from the inserted bases into the record"""
    head, tail = b"GGTCA", _record(10, 60)
    tail = (b"G" if tail[:1] == b"C" else b"") + tail                             # (the run ends behind the 40th unit)
    record = head + b"CT" * 40 + tail
    xa = len(head) + 80
    mate = head + b"CT" * 41 + tail
    ev, _, shifts = _events(_rec(0, (0, 0, xa), (xa, xa + 2, len(tail))), mate, record)
    assert ev == [(5, 1, 2, _seq("CT"))] and shifts == [80]
    # the same haplotype from the placement one base to the left: T C inserted in front of the last T
    ev, _, shifts = _events(_rec(0, (0, 0, xa - 1), (xa - 1, xa + 1, len(tail) + 1)), mate, record)
    assert ev == [(5, 1, 2, _seq("CT"))] and shifts == [79]


def test_strand_1_mates_report_on_the_records_strand():
    ins = b"GATTC" if REC[59:60] != b"C" else b"GATTG"
    mate = REC[10:60] + ins + REC[60:100]
    rec0, rec1 = _rec(0, (10, 0, 50), (60, 55, 40)), _rec(1, (10, 0, 50), (60, 55, 40))
    assert _events(rec0, mate, REC)[0] == _events(rec1, _rc(mate), REC)[0] == [(60, 1, 5, _seq(ins.decode()))]
    recs = np.zeros((2, 2), dtype=capi.ALIGNMENT_DTYPE)
    recs[0, 0], recs[1, 0] = rec0, rec1
    table, _ = expected_indels(recs, synth.batch_from_lists([mate, _rc(mate)]), [0, 1, 2], [0, 0], {0: REC}, 20)
    assert table == {(0, 60, 1, 5, _seq(ins.decode())): [1, 1]}
    assert indel_lines(table_array(table), {0: "gene"}) == ["gene 60 I 5 %s 1 1" % ins.decode()]
    assert len(table_array(table, 3)) == 0


def test_a_rescued_one_block_record_gives_no_event():
    assert _events(_rec(1, (40, 0, 100)), _rc(REC[40:140]), REC) == ([], {"mates": 1}, [])
    assert _events(_rec(0), REC[40:140], REC) == ([], {}, [])


def test_entry_validation_rules():
    lengths = [100, 50]
    ok = [(0, 0, 0, 1, 0, 1, 0, 0), (1, 49, 0, 1, 0, 0, 1, 0), (0, 99, 1, 12, (1 << 24) - 1, 1, 1, 0), (0, 35, 0, 65, 0, 5, 5, 0)]
    bad = [(2, 0, 0, 1, 0, 1, 0, 0), (0, 100, 1, 1, 0, 1, 0, 0), (0, 99, 0, 2, 0, 1, 0, 0), (0, 0, 2, 1, 0, 1, 0, 0), (0, 0, 0, 0, 0, 1, 0, 0),
           (0, 0, 0, 1, 1, 1, 0, 0), (0, 0, 1, 13, 0, 1, 0, 0), (0, 0, 1, 2, 16, 1, 0, 0), (0, 0, 1, 1, 0, 1, 0, 7), (0, 0, 0, 65536, 0, 1, 0, 0)]
    assert all(check_entry(e, lengths) for e in ok) and not any(check_entry(e, lengths) for e in bad)
    assert unpack(_seq("GATTACA"), 7) == [2, 0, 3, 3, 0, 1, 0]


# ---------------------------------------------------------------------------
# the boundary
# ---------------------------------------------------------------------------
NEW = ["shk_indels_enable", "shk_indels_get", "shk_indels_stats", "shk_indels_add", "shk_indels_reset"]


def test_new_symbols_in_header_binding_and_library():
    header = open(os.path.join(ROOT, "include", "shark_hip.h")).read()
    for name in NEW:
        assert re.search(r"^int %s\(shk_ctx \*" % name, header, re.M), name
        assert name in capi.EXPORTS
    assert "#define SHK_INDEL_MAX_INS 12" in header
    assert re.search(r"typedef struct shk_indel \{ uint32_t gene, x, kind, len, seq, fwd, rev, reserved; \} shk_indel;", header)
    assert capi.INDEL_DTYPE.itemsize == 32 and capi.INDEL_DTYPE.names == ("gene", "x", "kind", "len", "seq", "fwd", "rev", "reserved")
    assert capi.INDEL_STAT_NAMES == ("mates", "deletions", "insertions", "complex_gaps", "long_insertions", "nonbase_insertions", "dropped")
    for method in ("indels_enable", "indels_get", "indels_stats", "indels_add", "indels_reset"):
        assert callable(getattr(capi.SharkHip, method))
    import ctypes as C
    assert os.path.exists(LIB), "build the library first (make -C shark_amd/csrc)"
    L = C.CDLL(LIB)
    for name in NEW:
        assert hasattr(L, name), name


def test_the_host_only_parts_run_on_their_own():
    """shk_indels_add's entry validation and the command's line writer (shark_amd/csrc/indel_host.hpp) as a program without the library;
    tools/indel_host_check.sh builds the same file under AddressSanitizer and UndefinedBehaviorSanitizer"""
    tool = os.path.join(ROOT, "shark_amd", "bin", "shark-indel-host-check")
    assert os.path.exists(tool), "build first (make -C shark_amd/csrc)"
    r = subprocess.run([tool], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "indel host check ok", r.stderr


def test_the_commands_usage_errors(tmp_path):
    cli = os.path.join(ROOT, "shark_amd", "bin", "shark")
    for flags in (["--indels-min-support", "8"], ["--indels-min-intron", "20"], ["--indels-min-mates", "2"], ["--indels-capacity", "64"]):
        r = subprocess.run([cli, "-r", "x.fa", "-1", "y.fq"] + flags, capture_output=True, text=True, cwd=str(tmp_path))
        assert r.returncode == 1 and "--indels-min-support, --indels-min-intron, --indels-min-mates and --indels-capacity need --indels FILE." in r.stderr
    for flags, text in ((["--indels-min-support", "0"], "shark: --indels-min-support must be at least 1."),
                        (["--indels-min-intron", "65536"], "shark: --indels-min-intron must be 1 to 65535."),
                        (["--indels-capacity", "0"], "shark: --indels-capacity must be in the range [1, 4294967296].")):
        r = subprocess.run([cli, "-r", "x.fa", "-1", "y.fq", "--indels", "z"] + flags, capture_output=True, text=True, cwd=str(tmp_path))
        assert r.returncode == 1 and text in r.stderr
    for flags, text in ((["--extend-ends"], "shark: --extend-ends needs --sam FILE or --pileup-aligned (or --indels FILE)."),
                        (["--splice-junctions", "j"], "shark: --splice-junctions needs --sam FILE or --pileup-aligned (or --indels FILE).")):
        r = subprocess.run([cli, "-r", "x.fa", "-1", "y.fq"] + flags, capture_output=True, text=True, cwd=str(tmp_path))
        assert r.returncode == 1 and text in r.stderr
    r = subprocess.run([cli, "-h"], capture_output=True, text=True)
    assert "--indels FILE" in r.stderr and "--indels-capacity N" in r.stderr
