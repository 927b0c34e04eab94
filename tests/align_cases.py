"""The geometry cases of tests/test_gpu_align.py and their non-vacuity conditions, in plain Python and numpy: the test runs them on the
GPU, tools/align_seeds.py finds their seeds with the model and the CPU oracle alone."""
import numpy as np

from tests.spliced_synth import spliced_gene, spliced_reads


def geometry_case(k, ref, seed):
    """(genes, s_min, batch): spliced_gene / spliced_reads, 150 pairs, 3 % substitutions"""
    rng = np.random.default_rng(seed)
    genes = [spliced_gene(rng, 4, k)] if ref == "one gene" else [spliced_gene(rng, 1 + i, k) for i in range(2)]
    if ref == "twins":
        genes = [genes[1], genes[1]]
    return genes, 3 if k == 5 else 8, spliced_reads(rng, genes, 150, sub=0.03)


def geometry_conditions(recs, stats):
    """the non-vacuity conditions of a geometry case, by name"""
    aligned = recs["n_blocks"] > 0
    return {"aligned": int(aligned.sum()) >= 100, "two blocks": bool((recs["n_blocks"] >= 2).any()), "trimmed": stats.get("trimmed", 0) >= 1,
            "closed": stats.get("closed", 0) >= 1, "open insertion": stats.get("open_insertion", 0) >= 1,
            "mismatches": int((recs["mismatches"] > 0).sum()) >= 20}
