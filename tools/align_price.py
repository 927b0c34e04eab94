#!/usr/bin/env python3
"""What alignments mode costs next to pileup, the consumer of the same records at the same floor.  Per workload, in
one process:

  batch   ms per 10 M pairs (2 x 150 bp, k = 17, 50 % on-target, resident batches through shk_classify_device, which returns when
          the stream has drained: wall clock around the call) with
            plain       no mode on: the classify kernels and the assembly of results
            pileup      shk_pileup_enable(8): segments_kernel at m = 4 + pileup_kernel
            align       shk_alignments_enable(8): segments_kernel at m = 4 + align_kernel
            both        the two together: one segments_kernel, pileup_kernel, align_kernel
          the four alternating, the same batch, median of --reps
  worst   the same for a batch in which EVERY pair is the same on-target pair of the longest gene (tools/pileup_price.py's contention
          case: alignments mode has no shared counters, so it should not care)

`plain` is the comparison: tools/pileup_price.py measures the same figure the same way (its "plain"), so the two documents can be held
against each other; --pileup-price PATH copies that document's plain figures in beside this run's.

Workloads: headline (one gene of 20 000 bases), genes1000.  One process per workload.  Writes one JSON document.
usage: python tools/align_price.py [--pairs 4000000] [--reps 5] [--workloads headline,genes1000] [--pileup-price profiles/pileup_price.json]
                                   [--out profiles/align_price.json]"""
import argparse, json, os, subprocess, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

WORKLOADS = {"headline": 1, "genes1000": 1000}
MODES = ("plain", "pileup", "align", "both")
S_MIN = 8


def child(a):
    import numpy as np
    import torch
    from shark_amd import SharkHip, capi, synth
    dev = torch.device("cuda:0")
    ng = WORKLOADS[a.workload]
    genes = synth.make_reference(1, 20000) if ng == 1 else synth.make_gencode_like_reference(ng)
    out = {"workload": a.workload, "genes": ng, "pairs": a.pairs, "reference_bases": int(sum(len(g) for g in genes))}
    h = SharkHip(k=17, c=0.6, bf_bits=1 << 33)
    h.build([g.tobytes() for g in genes], keep_bases=True)
    out["probe_mode"] = h.probe_mode()
    b = synth.make_pairs_device(a.pairs, genes, dev, seed=synth.SEED + 7, read_len=150, on_target=0.5)
    # worst case: one pair of the longest gene, a.pairs times
    g0 = max(genes, key=len)
    at = max(0, min(1000, len(g0) - 250))
    comp = np.zeros(256, dtype=np.uint8)
    comp[list(b"ACGT")] = list(b"TGCA")
    m1 = torch.from_numpy(np.ascontiguousarray(g0[at:at + 150])).to(dev)
    m2 = torch.from_numpy(np.ascontiguousarray(comp[g0[at + 100:at + 250]][::-1])).to(dev)
    w = {"seq1": m1.repeat(a.pairs), "seq2": m2.repeat(a.pairs), "off1": b["off1"], "off2": b["off2"]}
    torch.cuda.synchronize()

    def run(batch, mode):
        h.pileup_enable(S_MIN if mode in ("pileup", "both") else 0)
        h.alignments_enable(S_MIN if mode in ("align", "both") else 0)
        t = time.perf_counter()
        r = h.classify_device(a.pairs, batch["seq1"].data_ptr(), batch["off1"].data_ptr(), batch["seq2"].data_ptr(), batch["off2"].data_ptr(), 0, 0, max_read_len=150)
        return (time.perf_counter() - t) * 1e3, int(r.n_assoc)

    scale = 1e7 / a.pairs
    for name, batch in (("batch", b), ("worst", w)):
        for mode in MODES:                                  # (untimed: allocations, the first batch of a stream)
            run(batch, mode)
        ms = {mode: [] for mode in MODES}
        n_assoc = 0
        for _ in range(a.reps):
            for mode in MODES:
                t, n_assoc = run(batch, mode)
                ms[mode].append(t)
        out[name] = {"n_assoc": n_assoc, "ms_per_10M_pairs": {mode: round(sorted(v)[len(v) // 2] * scale, 3) for mode, v in ms.items()},
                     "all_ms_per_10M_pairs": {mode: [round(x * scale, 3) for x in v] for mode, v in ms.items()}}
        # what the last batch with the mode on produced: a sample of its records (the first 100 000 associations)
        run(batch, "align")
        n, ptr = h.alignments_last()
        recs = capi.alignments_from_device(min(n, 100000), ptr)
        out[name]["sampled_associations"] = int(len(recs))
        out[name]["sampled_aligned_mates"] = int((recs["n_blocks"] > 0).sum())
        out[name]["sampled_blocks"] = int(recs["n_blocks"].sum())
        out[name]["sampled_block_bases"] = int(recs["block"][..., 2].sum(dtype=np.uint64))
        out[name]["record_bytes_per_batch"] = 128 * n
        h.pileup_reset()
    print("ALIGN_PRICE " + json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=4_000_000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--workloads", default=",".join(WORKLOADS))
    ap.add_argument("--pileup-price", default="")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "align_price.json"))
    ap.add_argument("--workload", default="")
    a = ap.parse_args()
    if a.workload:
        return child(a)
    runs, failed = [], False
    for wl in a.workloads.split(","):
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--workload", wl, "--pairs", str(a.pairs), "--reps", str(a.reps)],
                           capture_output=True, text=True, timeout=600)
        line = [x for x in r.stdout.splitlines() if x.startswith("ALIGN_PRICE ")]
        if r.returncode != 0 or not line:
            sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
            runs.append({"workload": wl, "failed": "exit %d" % r.returncode, "stderr_tail": r.stderr[-1000:]})
            print(json.dumps(runs[-1]), flush=True)
            failed = True
            break                                           # (nothing more is started behind a run that failed)
        runs.append(json.loads(line[0][len("ALIGN_PRICE "):]))
        print(json.dumps(runs[-1]), flush=True)
    earlier = {}
    if a.pileup_price:
        with open(a.pileup_price) as f:
            for s in json.load(f).get("summary", []):
                earlier[(s["workload"], s["case"])] = s.get("plain_ms_at_baseline")
    summary = []
    for r in runs:
        for name in ("batch", "worst"):
            if name not in r:
                continue
            m = r[name]["ms_per_10M_pairs"]
            summary.append({"workload": r["workload"], "case": name, "plain_ms": m["plain"], "plain_ms_in_pileup_price": earlier.get((r["workload"], name)),
                            "pileup_ms": m["pileup"], "align_ms": m["align"], "both_ms": m["both"],
                            "align_over_plain": round(m["align"] / m["plain"], 4), "align_over_pileup": round(m["align"] / m["pileup"], 4),
                            "align_kernel_ms": round(m["both"] - m["pileup"], 3)})
    doc = {"what": "wall clock of shk_classify_device per 10 M pairs (2 x 150 bp, k = 17, 50 % on-target): no mode, pileup alone, alignments alone and both, s_min = 8; the "
                   "same for a batch of one repeated pair; medians of alternating runs on one batch.  align_kernel_ms = both - pileup (the two share segments_kernel's "
                   "launch).  plain_ms_in_pileup_price: the same figure as tools/pileup_price.py recorded it",
           "summary": summary, "runs": runs}
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    return 1 if failed else 0


if __name__ == "__main__":
    sys.exit(main())
