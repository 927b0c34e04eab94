"""The junction table on the GPU (shk_junctions_enable / shk_junctions_get / shk_junctions_reset, `shark --junctions
--junctions-device`): the keys, their mate counts and their smallest introns, row for row, against the model (tests/spliced_model.py:
a dict built with shark_amd.capi.junctions at m = 4).  Integers, no tolerances.

Run on the GPU box with `pytest -m gpu`."""
import os

import numpy as np
import pytest

import torch  # noqa: F401  (torch bundles its own HIP runtime: load it BEFORE libsharkhip so one runtime serves both)

from tests import synth
from tests.segments_model import SegmentsModel, expected_segments, junction_lines, mate_lengths
from tests.spliced_model import expected_junction_table, table_rows
from tests.test_gpu_segments import _args, _dev_ptrs, _to_device
from tests.test_gpu_spliced_depth import Expected, build, run_shark, spliced_gene, spliced_reads

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("k", [5, 17, 31])
@pytest.mark.parametrize("n_genes", [1, 2])
def test_spliced_mates_on_both_strands(oracle, k, n_genes):
    rng = np.random.default_rng(2000 + 10 * k + n_genes)
    genes = [spliced_gene(rng, 4 - i, k) for i in range(n_genes)]
    s_min = 3 if k == 5 else 8
    o, h, sm = build(oracle, [g for g, _ in genes], k=k)
    want = Expected(sm, s_min, s_min)
    h.junctions_enable(s_min, 256)
    for paired, ragged in ((True, True), (False, False)):
        batch = spliced_reads(rng, genes, 150, paired=paired, ragged=ragged)
        want.add(o, batch, *h.classify(*_args(batch)))
        got = want.check_table(h)
    assert len(got) >= 4 and sum(r[4] for r in got) > 50          # (not vacuous)
    h.junctions_reset()
    assert len(h.junctions_get()) == 0


@pytest.mark.parametrize("n", [1, 63, 64, 65, 1000])
def test_batch_sizes(oracle, n):
    rng = np.random.default_rng(2025)
    panel = [spliced_gene(rng, int(rng.integers(1, 5)), 17) for _ in range(12)]
    rng = np.random.default_rng(9 * n)
    o, h, sm = build(oracle, [g for g, _ in panel], k=17)
    want = Expected(sm)
    h.junctions_enable(8, 2048)
    for ragged in (False, True):
        batch = spliced_reads(rng, panel, n, ragged=ragged)
        want.add(o, batch, *h.classify(*_args(batch)))
        want.check_table(h)


def _one_junction_gene(rng):
    e1, intron, e2 = synth.random_seq(rng, 80), synth.random_seq(rng, 50), synth.random_seq(rng, 80)
    return np.concatenate([e1, intron, e2]), e1, e2


def test_a_thousand_mates_on_one_junction(oracle):
    rng = np.random.default_rng(71)
    rec, e1, e2 = _one_junction_gene(rng)
    o, h, sm = build(oracle, [rec], k=17)
    want = Expected(sm)
    h.junctions_enable(8, 64)
    batch = synth.batch_from_lists([np.concatenate([e1[30 + i % 8:], e2[:50 - i % 8]]) for i in range(1000)])
    want.add(o, batch, *h.classify(*_args(batch)))
    got = want.check_table(h)
    assert len(got) == 1 and got[0][4] == 1000 and got[0][3] == 50


@pytest.fixture(scope="module")
def many_keys():
    """60 genes of four introns each: a few hundred distinct junctions"""
    rng = np.random.default_rng(73)
    genes = [spliced_gene(rng, 4, 17) for _ in range(60)]
    return genes, spliced_reads(rng, genes, 1000, sub=0.0)


def test_long_probe_chains(oracle, many_keys):
    """a few hundred distinct keys in the smallest table that holds them (a power of two: 64 doubled until they fit), so the table is
    more than half full and most keys sit behind others"""
    genes, batch = many_keys
    o, h, sm = build(oracle, [g for g, _ in genes], k=17)
    want = Expected(sm)
    h.junctions_enable(8, 1 << 16)
    want.add(o, batch, *h.classify(*_args(batch)))
    n_keys = len(want.table)
    capacity = 64
    while capacity < n_keys:
        capacity *= 2
    assert 200 <= n_keys and n_keys > capacity // 2
    want.check_table(h)
    h.junctions_reset()
    h.junctions_enable(8, capacity)               # (another capacity: allowed on a table that was reset and is empty)
    h.classify(*_args(batch))
    h.classify(*_args(batch))
    for v in want.table.values():
        v[1] *= 2
    want.check_table(h)


def test_a_full_table_is_an_error_and_reset_recovers(oracle, many_keys):
    from shark_amd import SharkHipError
    genes, batch = many_keys
    o, h, sm = build(oracle, [g for g, _ in genes], k=17)
    want = Expected(sm)
    h.junctions_enable(8, 64)
    goff, gids = h.classify(*_args(batch))
    want.add(o, batch, goff, gids)
    assert len(want.table) > 64
    for _ in range(2):
        with pytest.raises(SharkHipError, match="full"):
            h.junctions_get()
    h.junctions_reset()
    assert len(h.junctions_get()) == 0
    small = synth.batch_from_lists([batch["seq1"][int(batch["off1"][i]):int(batch["off1"][i + 1])] for i in range(20)])
    want.reset()
    want.add(o, small, *h.classify(*_args(small)))
    got = want.check_table(h)
    assert 1 <= len(got) <= 64


def _disagreeing_pair():
    """two mates over one junction, the second with one base inserted right behind it (an indel within k of the junction): the same
    (donor, acceptor), introns one apart.  Found with the model from a seeded generator: the first seed whose pair qualifies"""
    for seed in range(100, 120):
        rng = np.random.default_rng(seed)
        rec, e1, e2 = _one_junction_gene(rng)
        for base in b"ACGT":
            a = np.concatenate([e1[30:], e2[:50]])
            b = np.concatenate([e1[30:], np.array([base], np.uint8), e2[:50]])
            batch = synth.batch_from_lists([a, b])
            sm = SegmentsModel([bytes(rec)], 17)
            rows = expected_segments(sm, batch, [0, 1, 2], [0, 0], 4)[1]
            per_mate = [expected_junction_table(synth.batch_from_lists([m]), [0, 1], [0], rows[i:i + 1], 17, 8) for i, m in enumerate((a, b))]
            if all(len(t) == 1 for t in per_mate) and list(per_mate[0]) == list(per_mate[1]) and \
                    list(per_mate[0].values())[0][0] != list(per_mate[1].values())[0][0]:
                return seed, rec, batch
    return None


def test_mates_that_disagree_on_the_intron_give_the_smallest(oracle):
    found = _disagreeing_pair()
    assert found is not None and found[0] == 100
    _, rec, batch = found
    o, h, sm = build(oracle, [rec], k=17)
    want = Expected(sm)
    h.junctions_enable(8, 64)
    for order in ((0, 1), (1, 0)):
        b = synth.batch_from_lists([batch["seq1"][int(batch["off1"][i]):int(batch["off1"][i + 1])] for i in order])
        want.reset()
        want.add(o, b, *h.classify(*_args(b)))
        got = want.check_table(h)
        assert len(got) == 1 and got[0][4] == 2 and got[0][3] == 49          # (the record's intron is 50; the insertion moves the second diagonal by one)
        h.junctions_reset()


def test_state_rules(oracle):
    from shark_amd import SharkHip, SharkHipError
    rng = np.random.default_rng(37)
    genes = [spliced_gene(rng, 2, 17) for _ in range(4)]
    records = [g for g, _ in genes]
    h = SharkHip(k=17, c=0.0, bf_bits=1 << 26)
    with pytest.raises(SharkHipError):
        h.junctions_enable(8, 64)                 # before finalize
    h.junctions_enable(0, 0)                      # (off is always allowed)
    h.build([bytes(g) for g in records])
    with pytest.raises(SharkHipError):
        h.junctions_enable(8, 64)                 # finalized without keep_positions
    o, h, sm = build(oracle, records, k=17)
    for read_out in (h.junctions_get, h.junctions_reset):
        with pytest.raises(SharkHipError):
            read_out()                            # never enabled on this context
    want = Expected(sm)
    b = spliced_reads(rng, genes, 50)
    h.junctions_enable(8, 100)                    # (rounded up to 128)
    h.junctions_enable(8, 128)
    h.junctions_enable(8, 64)                     # (nothing submitted yet: allocated anew)
    goff, gids = h.classify(*_args(b))
    want.add(o, b, goff, gids)
    with pytest.raises(SharkHipError, match="capacity"):
        h.junctions_enable(8, 128)                # a capacity change on a table in use
    h.junctions_enable(8, 33)                     # (the same capacity after rounding)
    tk = h.submit(*_args(b))
    for call in (lambda: h.junctions_enable(8, 64), lambda: h.junctions_enable(0, 0), h.junctions_get, h.junctions_reset):
        with pytest.raises(SharkHipError):
            call()                                # tickets outstanding
    h.wait(tk)
    want.add(o, b, goff, gids)
    want.check_table(h)
    # off keeps the table and stops the counting; shk_count_work's batch and a wrongly vouched batch are not counted
    h.junctions_enable(0, 0)
    h.classify(*_args(b))
    want.check_table(h)
    h.junctions_enable(8, 64)
    t = _to_device(b)
    p = _dev_ptrs(t)
    h.count_work(50, p["seq1"], p["off1"], p["seq2"], p["off2"])
    ub = spliced_reads(rng, genes, 64, ragged=False)
    t = _to_device(ub)
    tk = h.submit_device(64, max_read_len=120, uniform_len1=99, uniform_len2=99, **_dev_ptrs(t))
    with pytest.raises(SharkHipError):
        h.wait_device(tk)
    want.check_table(h)
    wide = SharkHip(k=17, c=0.0, bf_bits=1 << 26)
    wide.build([b"ACGTACGTTGCATGCAAGCT"] * 65537, keep_positions=True)
    with pytest.raises(SharkHipError, match="65 536"):
        wide.junctions_enable(8, 64)


def test_shark_junctions_device_on_the_example(oracle, example_dir, tmp_path):
    fa = synth.read_fasta(os.path.join(example_dir, "ENSG00000277117.fa"))
    r1 = synth.read_fastq(os.path.join(example_dir, "sample_1.fq"))
    r2 = synth.read_fastq(os.path.join(example_dir, "sample_2.fq"))
    batch = synth.batch_from_lists([s for _, s, _ in r1], [s for _, s, _ in r2])
    o = oracle.Shark(k=17, c=0.6, bf_bits=1 << 33)
    o.build([s for _, s in fa])
    goff, gids = o.classify(*_args(batch))
    rows = expected_segments(SegmentsModel([s for _, s in fa], 17), batch, goff, gids, 4)[1]
    want = junction_lines(goff, gids, rows, mate_lengths(batch), 17, [n.decode() for n, _ in fa], 8)
    assert len(want) == 9 and table_rows(expected_junction_table(batch, goff, gids, rows, 17, 8))
    base = ["-r", os.path.join(example_dir, "ENSG00000277117.fa"), "-1", os.path.join(example_dir, "sample_1.fq"),
            "-2", os.path.join(example_dir, "sample_2.fq"), "-o", str(tmp_path / "o1"), "-p", str(tmp_path / "o2")]
    r = run_shark(base + ["--junctions", str(tmp_path / "host.jn")], str(tmp_path))
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    host = (tmp_path / "host.jn").read_bytes()
    assert host.decode().split("\n")[:-1] == want
    for tag, extra in (("a", []), ("b", ["--gpus", "2", "--devices", "0,0", "--batch", "700"]), ("c", ["--junctions-capacity", "64", "--segments", str(tmp_path / "sg")])):
        r = run_shark(base + ["--junctions", str(tmp_path / (tag + ".jn")), "--junctions-device"] + extra, str(tmp_path))
        assert r.returncode == 0, r.stderr.decode()[-2000:]
        assert (tmp_path / (tag + ".jn")).read_bytes() == host
    # a table too small for the sample's junctions: a message and a non-zero exit, never a shorter file
    rng = np.random.default_rng(73)
    genes = [spliced_gene(rng, 4, 17) for _ in range(60)]
    b = spliced_reads(rng, genes, 1000, sub=0.0)
    (tmp_path / "g.fa").write_text("".join(">g%d\n%s\n" % (i, bytes(g).decode()) for i, (g, _) in enumerate(genes)))
    for name, seq, off in (("1.fq", b["seq1"], b["off1"]), ("2.fq", b["seq2"], b["off2"])):
        with open(tmp_path / name, "w") as f:
            for i in range(1000):
                s = bytes(seq[int(off[i]):int(off[i + 1])]).decode()
                f.write("@r%d\n%s\n+\n%s\n" % (i, s, "I" * len(s)))
    syn = ["-r", str(tmp_path / "g.fa"), "-1", str(tmp_path / "1.fq"), "-2", str(tmp_path / "2.fq"), "-c", "0.3", "-o", str(tmp_path / "o1"), "-p", str(tmp_path / "o2")]
    r = run_shark(syn + ["--junctions", str(tmp_path / "full.jn"), "--junctions-device", "--junctions-capacity", "64"], str(tmp_path))
    assert r.returncode == 1 and b"--junctions-capacity" in r.stderr and (tmp_path / "full.jn").read_bytes() == b""
    r = run_shark(syn + ["--junctions", str(tmp_path / "ok.jn"), "--junctions-device"], str(tmp_path))
    r2_ = run_shark(syn + ["--junctions", str(tmp_path / "ok_host.jn")], str(tmp_path))
    assert r.returncode == 0 and r2_.returncode == 0 and (tmp_path / "ok.jn").read_bytes() == (tmp_path / "ok_host.jn").read_bytes()
    assert (tmp_path / "ok.jn").read_bytes().count(b"\n") > 64
