"""Every refusal of the entry points behind the context's accumulated states (depth, junctions, pileup, fragments, variants, the splice
list) and of the mode switches that share their guards, as the caller reads it: str(SharkHipError) = "<call>: <shk_strerror> (<shk_last_error>)"
compared with a literal string, in one fixed sequence of calls; where no refusal is due the call succeeds.  The strings are the
library's as it stood before the states got one owner, one guard and one counter type: the test passes on both.

The sequence ends with a destroy while every state is allocated, and a second context of the same process repeats enable, classify and
read-out: element for element the first one's.

Run on the GPU box with `pytest -m gpu`."""
import numpy as np
import pytest

import torch  # noqa: F401  (torch bundles its own HIP runtime: load it BEFORE libsharkhip so one runtime serves both)

from tests.spliced_synth import spliced_gene, spliced_reads
from tests.test_gpu_segments import _args

pytestmark = pytest.mark.gpu

STATE = "call not allowed in the current mode"
ARG = "invalid argument"
TICKETS = "tickets are outstanding (wait for them first)"
KW = dict(k=17, c=0.0, bf_bits=1 << 26)


class Walk:
    """one context and what its last refusal left in shk_last_error (a refusal that sets no text shows that one again)"""

    def __init__(self, h):
        self.h = h
        self.last = ""

    def refused(self, call, who, code, text):
        from shark_amd import SharkHipError
        with pytest.raises(SharkHipError) as e:
            call()
        self.last = "%s: %s" % (who, text)
        assert str(e.value) == "%s: %s (%s)" % (who, code, self.last)

    def refused_without_text(self, call, who, code):
        from shark_amd import SharkHipError
        with pytest.raises(SharkHipError) as e:
            call()
        assert str(e.value) == "%s: %s (%s)" % (who, code, self.last)

    def each(self, calls, code, text):
        for who, call in calls:
            self.refused(call, who, code, text)


def enables(h, site):
    """every switch that asks something of the index, switched ON"""
    return [("shk_placement_enable", lambda: h.placement_enable(True)), ("shk_segments_enable", lambda: h.segments_enable(4)),
            ("shk_depth_enable", lambda: h.depth_enable(1)), ("shk_depth_enable_spliced", lambda: h.depth_enable_spliced(8)),
            ("shk_junctions_enable", lambda: h.junctions_enable(8, 256)), ("shk_pileup_enable", lambda: h.pileup_enable(8)),
            ("shk_pileup_enable_aligned", lambda: h.pileup_enable_aligned(8)), ("shk_alignments_enable", lambda: h.alignments_enable(8)),
            ("shk_pairs_enable", lambda: h.pairs_enable(20, 1000, 32)), ("shk_rescue_enable", lambda: h.rescue_enable(20, 1000, 8, 4)),
            ("shk_splice_sites_set", lambda: h.splice_sites_set(site))]


NEED_BASES = ("shk_pileup_enable_aligned", "shk_alignments_enable", "shk_pairs_enable", "shk_rescue_enable")


def read_outs(h, total):
    """every read-out and reset of the states, by the state whose never-enabled text it carries (variants: the pileup state's)"""
    zeros = np.zeros((total, 4), np.uint32)
    return {"depth mode": [("shk_depth_get", lambda: h.depth(0)), ("shk_depth_get_all", h.depth_all), ("shk_depth_summary", h.depth_summary),
                           ("shk_depth_mates", h.depth_mates), ("shk_depth_reset", h.depth_reset)],
            "the junction table": [("shk_junctions_get", h.junctions_get), ("shk_junctions_reset", h.junctions_reset)],
            "pileup mode": [("shk_pileup_get", lambda: h.pileup(0)), ("shk_pileup_get_all", h.pileup_all), ("shk_pileup_mates", h.pileup_mates),
                            ("shk_pileup_reset", h.pileup_reset), ("shk_pileup_add", lambda: h.pileup_add(zeros, 0)),
                            ("shk_variants_get", lambda: h.variants(1, 1)), ("shk_variants_summary", lambda: h.variants_summary(1, 1))],
            "pairs mode": [("shk_fragments_get", lambda: h.fragments(32)), ("shk_fragments_reset", h.fragments_reset)]}


def switch_all_on(h, sites):
    h.depth_enable_spliced(8)
    h.junctions_enable(8, 256)
    h.pileup_enable_aligned(8)
    h.alignments_enable(8)
    h.pairs_enable(20, 1000, 32)
    h.rescue_enable(20, 1000, 8, 4)
    h.splice_sites_set(sites)
    h.alignments_splice(3, 2, 2)


def read_everything(h, result):
    """the batch's genes and every read-out of every state, as arrays"""
    out = {"gene_off": result[0], "gene_ids": result[1], "depth_all": h.depth_all(), "depth_1": h.depth(1), "depth_summary": h.depth_summary(),
           "depth_mates": np.array([h.depth_mates()]), "junctions": h.junctions_get(), "pileup_all": h.pileup_all(), "pileup_2": h.pileup(2),
           "pileup_mates": np.array([h.pileup_mates()]), "variants": h.variants(1, 1, (1, 100)), "variants_summary": h.variants_summary(1, 1, (1, 100))}
    out["fragments_hist"], out["fragments_classes"] = h.fragments(32)
    return out


def test_every_refusal_as_the_caller_reads_it():
    from shark_amd import SharkHip
    rng = np.random.default_rng(97)
    genes = [spliced_gene(rng, 3, 17) for _ in range(3)]
    records = [bytes(rec) for rec, _ in genes]
    assert all(200 <= len(r) <= 400 for r in records)
    total = sum(len(r) for r in records)
    batch = spliced_reads(rng, genes, 50)
    site = np.array([(0, 80, 140)], dtype=np.int64)

    # ---- before finalize: every switch ON is refused, OFF needs nothing; no state exists ----
    w = Walk(SharkHip(**KW))
    h = w.h
    w.each(enables(h, site), STATE, "the index is not finalized")
    for off in (lambda: h.placement_enable(False), lambda: h.segments_enable(0), lambda: h.depth_enable(0), lambda: h.depth_enable_spliced(0),
                lambda: h.junctions_enable(0), lambda: h.pileup_enable(0), lambda: h.pileup_enable_aligned(0), lambda: h.alignments_enable(0),
                lambda: h.pairs_enable(20, 1000, 0), lambda: h.rescue_enable(20, 0, 8, 4), lambda: h.alignments_splice(0, 2, 2),
                lambda: h.alignments_extend(4, 5)):
        off()
    w.refused(h.depth_mates, "shk_depth_mates", STATE, "depth mode was never enabled on this context")
    w.refused(h.depth_reset, "shk_depth_reset", STATE, "depth mode was never enabled on this context")
    w.refused(h.junctions_get, "shk_junctions_get", STATE, "the junction table was never enabled on this context")
    w.refused(h.junctions_reset, "shk_junctions_reset", STATE, "the junction table was never enabled on this context")
    w.refused(h.pileup_mates, "shk_pileup_mates", STATE, "pileup mode was never enabled on this context")
    w.refused(h.pileup_reset, "shk_pileup_reset", STATE, "pileup mode was never enabled on this context")
    w.refused(lambda: h.fragments(32), "shk_fragments_get", STATE, "pairs mode was never enabled on this context")
    w.refused(h.fragments_reset, "shk_fragments_reset", STATE, "pairs mode was never enabled on this context")
    w.refused(lambda: h.alignments_splice(3, 2, 2), "shk_alignments_splice", STATE, "no site list (shk_splice_sites_set first)")
    h.close()

    # ---- finalized without keep_positions; with a ticket outstanding the switches report the ticket and the site list the index ----
    w = Walk(SharkHip(**KW))
    h = w.h
    h.build(records)
    w.each(enables(h, site), STATE, "the index was finalized without shk_ref_keep_positions")
    tk = h.submit(*_args(batch))
    w.each(enables(h, site)[:-1], STATE, TICKETS)
    w.refused(lambda: h.splice_sites_set(site), "shk_splice_sites_set", STATE, "the index was finalized without shk_ref_keep_positions")
    h.wait(tk)
    h.close()

    # ---- finalized with keep_positions, without keep_bases ----
    w = Walk(SharkHip(**KW))
    h = w.h
    h.build(records, keep_positions=True)
    for who, call in enables(h, site):
        if who in NEED_BASES:
            w.refused(call, who, STATE, "the index was finalized without shk_ref_keep_bases")
        else:
            call()
    w.refused(lambda: h.variants(1, 1), "shk_variants_get", STATE, "the index was finalized without shk_ref_keep_bases")
    w.refused(lambda: h.variants_summary(1, 1), "shk_variants_summary", STATE, "the index was finalized without shk_ref_keep_bases")
    h.close()

    # ---- the context with everything: never enabled, alone and with a ticket outstanding (never enabled is reported first) ----
    w = Walk(SharkHip(**KW))
    h = w.h
    h.build(records, keep_bases=True)
    assert int(h.depth_layout()[-1]) == total
    for what, calls in read_outs(h, total).items():
        w.each(calls, STATE, what + " was never enabled on this context")
    tk = h.submit(*_args(batch))
    for what, calls in read_outs(h, total).items():
        w.each(calls, STATE, what + " was never enabled on this context")
    # arguments are looked at before the tickets by these, behind them by the enables with a state or parameters of their own
    w.refused(lambda: h.candidates_enable(9), "shk_candidates_enable", ARG, "m must be at most SHK_MAX_CANDIDATES")
    w.refused(lambda: h.segments_enable(5), "shk_segments_enable", ARG, "m must be at most SHK_MAX_SEGMENTS")
    w.refused(lambda: h.alignments_extend(16, 0), "shk_alignments_extend", ARG, "mismatch_penalty and end_bonus are at most 15")
    w.refused(lambda: h.alignments_splice(49, 2, 2), "shk_alignments_splice", ARG, "min_overhang is at most SHK_SPLICE_MAX_OVERHANG, max_cost and min_gap at most 64")
    w.refused(lambda: h.pairs_enable(20, 1000, 1), "shk_pairs_enable", STATE, TICKETS)
    w.refused(lambda: h.rescue_enable(0, 1000, 8, 4), "shk_rescue_enable", STATE, TICKETS)
    w.refused(lambda: h.junctions_enable(8, (1 << 40) + 1), "shk_junctions_enable", STATE, TICKETS)
    w.refused(lambda: h.splice_sites_set(np.array([(3, 80, 140)])), "shk_splice_sites_set", STATE, TICKETS)
    h.wait(tk)

    # ---- pairs and rescue without alignments mode; the argument errors ----
    w.refused(lambda: h.pairs_enable(20, 1000, 32), "shk_pairs_enable", STATE, "alignments mode is off (shk_alignments_enable first)")
    w.refused(lambda: h.rescue_enable(20, 1000, 8, 4), "shk_rescue_enable", STATE, "alignments mode is off (shk_alignments_enable first)")
    for bad in ((20, 1000, 1), (20, 1000, 4097), (0, 1000, 32)):
        w.refused(lambda: h.pairs_enable(*bad), "shk_pairs_enable", ARG, "n_bins is 0 or 2 .. 4096 and min_intron at least 1")
    for bad in ((20, 4097, 8, 4), (0, 1000, 8, 4), (20, 1000, 256, 4), (20, 1000, 8, 256)):
        w.refused(lambda: h.rescue_enable(*bad), "shk_rescue_enable", ARG, "max_frag is 0 or 1 .. 4096, min_intron at least 1, max_cost and min_gap at most 255")
    for bad in ((49, 2, 2), (3, 65, 2), (3, 2, 65)):
        w.refused(lambda: h.alignments_splice(*bad), "shk_alignments_splice", ARG, "min_overhang is at most SHK_SPLICE_MAX_OVERHANG, max_cost and min_gap at most 64")
    w.refused(lambda: h.alignments_splice(3, 2, 2), "shk_alignments_splice", STATE, "no site list (shk_splice_sites_set first)")
    w.refused(lambda: h.junctions_enable(8, (1 << 40) + 1), "shk_junctions_enable", ARG, "capacity beyond 2^40 entries")
    w.refused(lambda: h.splice_sites_set(np.array([(3, 80, 140)])), "shk_splice_sites_set", ARG,
              "site 0 lies outside its record (gene < n_records, 1 <= donor < acceptor <= len - 1)")
    w.refused(lambda: h.splice_sites_set(np.array([(0, 80, 140), (0, 80, 140)])), "shk_splice_sites_set", ARG, "site 1 does not ascend in (gene, donor, acceptor)")

    # ---- every state on; a ticket outstanding: every switch, read-out and reset reports it ----
    sites = np.array([(0, 80, 140), (1, 75, 130), (2, 90, 150)], dtype=np.int64)
    switch_all_on(h, sites)
    tk = h.submit(*_args(batch))
    w.each([("shk_evidence_enable", lambda: h.evidence_enable(True)), ("shk_candidates_enable", lambda: h.candidates_enable(4))] + enables(h, site)
           + [("shk_alignments_extend", lambda: h.alignments_extend(4, 5)), ("shk_alignments_splice", lambda: h.alignments_splice(3, 2, 2))]
           + [c for calls in read_outs(h, total).values() for c in calls], STATE, TICKETS)
    first = read_everything(h, h.wait(tk))
    assert first["depth_mates"][0] > 0 and first["pileup_mates"][0] > 0 and len(first["junctions"]) > 0 and first["fragments_classes"].sum() > 0
    assert first["depth_all"].any() and first["pileup_all"].any() and len(first["variants"]) > 0
    # (refusals that set no text: shk_last_error still shows the one before)
    w.refused_without_text(lambda: h.depth(3), "shk_depth_get", ARG)
    w.refused_without_text(lambda: h.pileup(3), "shk_pileup_get", ARG)
    w.refused(lambda: h.variants(0, 1), "shk_variants_get", ARG, "parameters outside min_depth >= 1, min_alt >= 1, 1 <= frac_den <= 65535, frac_num <= frac_den")
    w.refused(lambda: h.pileup_add(np.zeros(4, np.uint32), 0), "shk_pileup_add", ARG, "n_entries is not 4 * gene_start[nidx]")
    w.refused(lambda: h.fragments(64), "shk_fragments_get", ARG, "n_bins is not the state's")

    # ---- the other kind, another capacity, another n_bins: refused on a dirty state, taken on a clean one, which reads zero ----
    w.refused(lambda: h.depth_enable(1), "shk_depth_enable", STATE, "the state holds depth of the other kind (plain / spliced): shk_depth_reset first")
    w.refused(lambda: h.pileup_enable(8), "shk_pileup_enable", STATE, "the state holds pileup of the other kind (owned / aligned): shk_pileup_reset first")
    w.refused(lambda: h.junctions_enable(8, 512), "shk_junctions_enable", ARG, "another capacity than the table's (shk_junctions_reset first)")
    w.refused(lambda: h.pairs_enable(20, 1000, 64), "shk_pairs_enable", ARG, "another n_bins than the state's (shk_fragments_reset first)")
    h.depth_enable_spliced(8)                                    # (its own kind, its own shapes: taken while dirty)
    h.pileup_enable_aligned(8)
    h.junctions_enable(8, 200)                                   # (rounded up to the table's 256)
    h.pairs_enable(20, 1000, 32)
    h.depth_reset()
    h.pileup_reset()
    h.junctions_reset()
    h.fragments_reset()
    h.depth_enable(1)
    h.pileup_enable(8)
    h.junctions_enable(8, 512)
    h.pairs_enable(20, 1000, 64)
    assert not h.depth_all().any() and h.depth_mates() == 0 and not h.pileup_all().any() and h.pileup_mates() == 0
    assert len(h.junctions_get()) == 0 and not h.fragments(64)[0].any() and not h.fragments(64)[1].any()
    w.refused(lambda: h.fragments(32), "shk_fragments_get", ARG, "n_bins is not the state's")
    h.depth_enable_spliced(8)                                    # (and back, still clean)
    h.pileup_enable_aligned(8)

    # ---- destroyed with every state, the splice list and the variants scratch allocated; a second context reads what the first read ----
    h.close()
    h = SharkHip(**KW)
    h.build(records, keep_bases=True)
    switch_all_on(h, sites)
    second = read_everything(h, h.classify(*_args(batch)))
    h.close()
    assert first.keys() == second.keys()
    for name in first:
        assert first[name].dtype == second[name].dtype and first[name].shape == second[name].shape and first[name].tobytes() == second[name].tobytes(), name
