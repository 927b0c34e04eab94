#!/usr/bin/env python3
"""What end extension and aligned pileup cost, on tools/align_price.py's workloads and cases.  Per workload, in one
process:

  batch   ms per 10 M pairs (2 x 150 bp, k = 17, 50 % on-target, resident batches through shk_classify_device, which returns when
          the stream has drained: wall clock around the call) with
            align        shk_alignments_enable(8), extension off: align_kernel as it always was
            align_ext    the same with shk_alignments_extend(4, 5): the extending instantiation
            owned_align  shk_pileup_enable(8) + alignments: pileup_kernel and align_kernel
            aligned      shk_pileup_enable_aligned(8) + alignments, extension off: ONE kernel, the accumulating instantiation
            aligned_ext  the same with (4, 5)
          the five alternating, the same batch, median of --reps
  worst   the same for a batch in which EVERY pair is the same on-target pair of the longest gene (every atomic on the same lines)

`align` and `owned_align` are tools/align_price.py's `align` and `both`: run that tool on a build of the parent commit in the same
session and pass its document with --parent PATH to have the parent's figures copied in beside this run's.

Workloads: headline (one gene of 20 000 bases), genes1000.  One process per workload.  Writes one JSON document.
usage: python tools/extend_price.py [--pairs 4000000] [--reps 5] [--workloads headline,genes1000] [--parent parent_align_price.json]
                                    [--out profiles/extend_price.json]"""
import argparse, json, os, subprocess, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

WORKLOADS = {"headline": 1, "genes1000": 1000}
# mode: (kind of pileup or None, extension)
MODES = {"align": (None, (0, 0)), "align_ext": (None, (4, 5)), "owned_align": ("owned", (0, 0)), "aligned": ("aligned", (0, 0)),
         "aligned_ext": ("aligned", (4, 5))}
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
    b = synth.make_pairs_device(a.pairs, genes, dev, seed=synth.SEED + 7, read_len=150, on_target=0.5)
    g0 = max(genes, key=len)
    at = max(0, min(1000, len(g0) - 250))
    comp = np.zeros(256, dtype=np.uint8)
    comp[list(b"ACGT")] = list(b"TGCA")
    m1 = torch.from_numpy(np.ascontiguousarray(g0[at:at + 150])).to(dev)
    m2 = torch.from_numpy(np.ascontiguousarray(comp[g0[at + 100:at + 250]][::-1])).to(dev)
    w = {"seq1": m1.repeat(a.pairs), "seq2": m2.repeat(a.pairs), "off1": b["off1"], "off2": b["off2"]}
    torch.cuda.synchronize()

    def run(batch, mode):
        kind, (P, B) = MODES[mode]
        h.pileup_enable(0)
        h.pileup_reset() if kind else None                  # (one state holds one kind: the switch is free behind a reset)
        if kind == "owned":
            h.pileup_enable(S_MIN)
        elif kind == "aligned":
            h.pileup_enable_aligned(S_MIN)
        h.alignments_enable(S_MIN)
        h.alignments_extend(P, B)
        t = time.perf_counter()
        r = h.classify_device(a.pairs, batch["seq1"].data_ptr(), batch["off1"].data_ptr(), batch["seq2"].data_ptr(), batch["off2"].data_ptr(), 0, 0, max_read_len=150)
        return (time.perf_counter() - t) * 1e3, int(r.n_assoc)

    scale = 1e7 / a.pairs
    h.pileup_enable(S_MIN)                                   # (the state exists before the first reset)
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
        # what extension adds on this batch: block bases of a sample of its records (the first 100 000 associations), off and on
        for mode in ("align", "align_ext"):
            run(batch, mode)
            n, ptr = h.alignments_last()
            recs = capi.alignments_from_device(min(n, 100000), ptr)
            out[name]["sampled_block_bases_" + mode] = int(recs["block"][..., 2].sum(dtype=np.uint64))
    print("EXTEND_PRICE " + json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=4_000_000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--workloads", default=",".join(WORKLOADS))
    ap.add_argument("--parent", default="")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "extend_price.json"))
    ap.add_argument("--workload", default="")
    a = ap.parse_args()
    if a.workload:
        return child(a)
    runs, failed = [], False
    for wl in a.workloads.split(","):
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--workload", wl, "--pairs", str(a.pairs), "--reps", str(a.reps)],
                           capture_output=True, text=True, timeout=600)
        line = [x for x in r.stdout.splitlines() if x.startswith("EXTEND_PRICE ")]
        if r.returncode != 0 or not line:
            sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
            runs.append({"workload": wl, "failed": "exit %d" % r.returncode, "stderr_tail": r.stderr[-1000:]})
            print(json.dumps(runs[-1]), flush=True)
            failed = True
            break                                           # (nothing more is started behind a run that failed)
        runs.append(json.loads(line[0][len("EXTEND_PRICE "):]))
        print(json.dumps(runs[-1]), flush=True)
    parent = {}
    if a.parent:
        with open(a.parent) as f:
            for s in json.load(f).get("summary", []):
                parent[(s["workload"], s["case"])] = s
    summary = []
    for r in runs:
        for name in ("batch", "worst"):
            if name not in r:
                continue
            m = r[name]["ms_per_10M_pairs"]
            p = parent.get((r["workload"], name), {})
            summary.append({"workload": r["workload"], "case": name, "align_ms": m["align"], "align_ext_ms": m["align_ext"], "owned_align_ms": m["owned_align"],
                            "aligned_ms": m["aligned"], "aligned_ext_ms": m["aligned_ext"], "parent_align_ms": p.get("align_ms"), "parent_both_ms": p.get("both_ms"),
                            "ext_over_align": round(m["align_ext"] / m["align"], 4), "aligned_over_owned_align": round(m["aligned"] / m["owned_align"], 4)})
    doc = {"what": "wall clock of shk_classify_device per 10 M pairs (2 x 150 bp, k = 17, 50 % on-target), s_min = 8: alignments with extension off and at (4, 5); owned "
                   "pileup + alignments (two kernels) against aligned pileup + alignments (one), extension off and on; the same for a batch of one repeated pair; "
                   "medians of alternating runs on one batch.  parent_*: tools/align_price.py's align and both on a build of the parent commit in the same session",
           "summary": summary, "runs": runs}
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    return 1 if failed else 0


if __name__ == "__main__":
    sys.exit(main())
