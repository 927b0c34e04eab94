#!/usr/bin/env python3
"""What indels mode costs next to the kernel whose records it reads.  Per workload and sample, in one process:

  ms per 1 M pairs (2 x 150 bp, k = 17, 50 % on-target, resident batches through shk_classify_device, which returns when the stream has
  drained: wall clock around the call) with
    plain            no mode on: the classify kernels and the assembly of results
    align            shk_alignments_enable(8): segments_kernel at m = 4 + align_kernel
    align_indels     the same and shk_indels_enable(8) at the same floor: one align_kernel launch serves both, indel_kernel behind it
    align_pileup     alignments and shk_pileup_enable(8): the same launches as `align` and pileup_kernel
    indels           shk_indels_enable(8) alone: segments_kernel, the storing align_kernel into the context's own array, indel_kernel
  the five alternating, the same batch, median of --reps.  From these:
    align_kernel_ms      align - plain          (with segments_kernel: the price of the records this mode reads)
    indel_kernel_ms      align_indels - align   (on the sample without indels: the scan; on the sample with them: scan + events)
    pileup_kernel_ms     align_pileup - align   (the yardstick: another kernel behind the same records, on the same batch)

  Samples: `clean`, the generator's pairs (1 % substitutions, no indel), and `indels`, the same pairs with one base taken out of the
  middle of every --share-th mate 1 (the mate keeps its length: its last base is repeated), so that a fixed share of the on-target mates
  show a one-base deletion.  event_ms = indel_kernel_ms(indels) - indel_kernel_ms(clean), and per event with the table's own count.

Workloads: headline (one gene of 20 000 bases), genes1000.  One process per workload.  Writes one JSON document.
usage: python tools/indels_price.py [--pairs 1000000] [--reps 5] [--share 8] [--workloads headline,genes1000] [--out profiles/indels_price.json]"""
import argparse, json, os, subprocess, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

WORKLOADS = {"headline": 1, "genes1000": 1000}
MODES = ("plain", "align", "align_indels", "align_pileup", "indels")
S_MIN = 8


def child(a):
    import torch
    from shark_amd import SharkHip, synth
    dev = torch.device("cuda:0")
    ng = WORKLOADS[a.workload]
    genes = synth.make_reference(1, 20000) if ng == 1 else synth.make_gencode_like_reference(ng)
    out = {"workload": a.workload, "genes": ng, "pairs": a.pairs, "share": a.share, "reference_bases": int(sum(len(g) for g in genes))}
    h = SharkHip(k=17, c=0.6, bf_bits=1 << 33)
    h.build([g.tobytes() for g in genes], keep_bases=True)
    out["probe_mode"] = h.probe_mode()
    clean = synth.make_pairs_device(a.pairs, genes, dev, seed=synth.SEED + 7, read_len=150, on_target=0.5)
    # one base out of the middle of every share-th mate 1
    L = 150
    rows = clean["seq1"].view(a.pairs, L).clone()
    src = torch.arange(L, device=dev)
    src = torch.where(src >= L // 2, torch.clamp(src + 1, max=L - 1), src)
    rows[::a.share] = rows[::a.share][:, src]
    with_indels = dict(clean)
    with_indels["seq1"] = rows.reshape(-1).contiguous()
    torch.cuda.synchronize()

    def run(batch, mode):
        h.pileup_enable(S_MIN if mode == "align_pileup" else 0)
        h.alignments_enable(S_MIN if mode.startswith("align") else 0)
        h.indels_enable(S_MIN if mode in ("align_indels", "indels") else 0, 20, 1 << 20)
        t = time.perf_counter()
        r = h.classify_device(a.pairs, batch["seq1"].data_ptr(), batch["off1"].data_ptr(), batch["seq2"].data_ptr(), batch["off2"].data_ptr(), 0, 0, max_read_len=150)
        return (time.perf_counter() - t) * 1e3, int(r.n_assoc)

    scale = 1e6 / a.pairs
    for name, batch in (("clean", clean), ("indels", with_indels)):
        for mode in MODES:                                  # (untimed: allocations, the first batch of a stream)
            run(batch, mode)
        ms = {mode: [] for mode in MODES}
        n_assoc = 0
        for _ in range(a.reps):
            for mode in MODES:
                t, n_assoc = run(batch, mode)
                ms[mode].append(t)
        med = {mode: sorted(v)[len(v) // 2] * scale for mode, v in ms.items()}
        # what one batch adds to the table
        h.indels_enable(S_MIN, 20, 1 << 20)
        h.indels_reset()
        run(batch, "indels")
        st = h.indels_stats()
        keys = len(h.indels_get())
        h.indels_reset()
        out[name] = {"n_assoc": n_assoc, "ms_per_1M_pairs": {mode: round(v, 4) for mode, v in med.items()},
                     "all_ms_per_1M_pairs": {mode: [round(x * scale, 4) for x in v] for mode, v in ms.items()},
                     "align_kernel_ms": round(med["align"] - med["plain"], 4), "indel_kernel_ms": round(med["align_indels"] - med["align"], 4),
                     "pileup_kernel_ms": round(med["align_pileup"] - med["align"], 4), "indels_alone_over_plain_ms": round(med["indels"] - med["plain"], 4),
                     "stats_per_batch": st, "keys_per_batch": keys}
    ev = out["indels"]["stats_per_batch"]["deletions"] + out["indels"]["stats_per_batch"]["insertions"] - \
        out["clean"]["stats_per_batch"]["deletions"] - out["clean"]["stats_per_batch"]["insertions"]
    out["event_ms"] = round(out["indels"]["indel_kernel_ms"] - out["clean"]["indel_kernel_ms"], 4)
    out["events_added"] = ev
    out["ns_per_event"] = round(out["event_ms"] * 1e6 / scale / ev, 2) if ev > 0 else None
    print("INDELS_PRICE " + json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=1_000_000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--share", type=int, default=8)
    ap.add_argument("--workloads", default=",".join(WORKLOADS))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "indels_price.json"))
    ap.add_argument("--workload", default="")
    a = ap.parse_args()
    if a.workload:
        return child(a)
    runs, failed = [], False
    for wl in a.workloads.split(","):
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--workload", wl, "--pairs", str(a.pairs), "--reps", str(a.reps), "--share", str(a.share)],
                           capture_output=True, text=True, timeout=600)
        line = [x for x in r.stdout.splitlines() if x.startswith("INDELS_PRICE ")]
        if r.returncode != 0 or not line:
            sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
            runs.append({"workload": wl, "failed": "exit %d" % r.returncode, "stderr_tail": r.stderr[-1000:]})
            print(json.dumps(runs[-1]), flush=True)
            failed = True
            break                                           # (nothing more is started behind a run that failed)
        runs.append(json.loads(line[0][len("INDELS_PRICE "):]))
        print(json.dumps(runs[-1]), flush=True)
    summary = [{"workload": r["workload"], "align_kernel_ms": r["clean"]["align_kernel_ms"], "scan_ms": r["clean"]["indel_kernel_ms"],
                "pileup_kernel_ms": r["clean"]["pileup_kernel_ms"], "scan_and_events_ms": r["indels"]["indel_kernel_ms"], "event_ms": r["event_ms"],
                "events_added": r["events_added"], "ns_per_event": r["ns_per_event"], "indels_alone_over_plain_ms": r["clean"]["indels_alone_over_plain_ms"]}
               for r in runs if "clean" in r]
    doc = {"what": "wall clock of shk_classify_device per 1 M pairs (2 x 150 bp, k = 17, 50 % on-target): no mode, alignments, alignments with indels at the same floor, "
                   "alignments with pileup, indels alone; on the generator's pairs and on the same pairs with a base taken out of every share-th mate 1; medians of "
                   "alternating runs on one batch.  indel_kernel_ms = align_indels - align (one align_kernel launch serves both)",
           "summary": summary, "runs": runs}
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    return 1 if failed else 0


if __name__ == "__main__":
    sys.exit(main())
