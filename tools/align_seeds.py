#!/usr/bin/env python3
"""The seeds of tests/test_gpu_align.py's geometry cases: per (k, reference) the first seed, counting from 1, whose 150 pairs meet
every non-vacuity condition of geometry_conditions -- found with the model (tests/align_model.py) and the CPU oracle alone, no GPU.

    python tools/align_seeds.py [max_seed]

Prints one line per case: the seed, or, where no seed up to max_seed (default 300) meets them all, the first seed that misses exactly
one condition and that condition's name (the test then drops it for that case and says so)."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from oracle import pyoracle  # noqa: E402
from tests.align_cases import geometry_case, geometry_conditions  # noqa: E402
from tests.align_model import expected_alignments  # noqa: E402
from tests.segments_model import SegmentsModel, expected_segments  # noqa: E402


def conditions(k, ref, seed):
    genes, s_min, batch = geometry_case(k, ref, seed)
    records = [bytes(g) for g, _ in genes]
    o = pyoracle.Shark(k=k, c=0.0, bf_bits=1 << 26)
    o.build(records)
    goff, gids = o.classify(batch["seq1"], batch["off1"], batch["seq2"], batch["off2"], None, None)
    sm = SegmentsModel(records, k)
    rows = expected_segments(sm, batch, goff, gids, 4)[1]
    stats = {}
    recs = expected_alignments(sm, batch, goff, gids, rows, s_min, stats=stats)
    return geometry_conditions(recs, stats)


def main():
    max_seed = int(sys.argv[1]) if len(sys.argv) > 1 else 300
    for k in (5, 17, 31):
        for ref in ("one gene", "two genes", "twins"):
            near = None
            for seed in range(1, max_seed + 1):
                missed = [name for name, met in conditions(k, ref, seed).items() if not met]
                if not missed:
                    print("(%d, %r): %d" % (k, ref, seed), flush=True)
                    break
                if len(missed) == 1 and near is None:
                    near = (seed, missed[0])
            else:
                print("(%d, %r): none up to %d; all but one at %s" % (k, ref, max_seed, near), flush=True)


if __name__ == "__main__":
    main()
