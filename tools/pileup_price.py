#!/usr/bin/env python3
"""What pileup mode costs next to spliced depth, the consumer of the same records it is consistent with.  Per
workload, in one process:

  batch   ms per 10 M pairs (2 x 150 bp, k = 17, 50 % on-target, resident batches through shk_classify_device, which returns when
          the stream has drained: wall clock around the call) with
            plain            no mode on: the classify kernels and the assembly of results
            depth_spliced    shk_depth_enable_spliced(8): segments_kernel at m = 4 + spliced_accumulate_kernel
            pileup           shk_pileup_enable(8): segments_kernel at m = 4 + pileup_kernel
            both             the two together: one segments_kernel, spliced_accumulate_kernel, pileup_kernel
          the four alternating, the same batch, median of --reps
  worst   the same for a batch in which EVERY pair is the same on-target pair of the longest gene: all adds land on the same few
          hundred counters (tools/depth_price.py's contention case)

With --parent-lib PATH (a libsharkhip.so built from the parent commit) plain and depth_spliced are measured on that library too, in
a process of its own between this tree's, as the baseline `at_parent`.

Workloads: headline (one gene of 20 000 bases), genes1000.  One process per workload and library.  Writes one JSON document.
usage: python tools/pileup_price.py [--pairs 4000000] [--reps 5] [--workloads headline,genes1000] [--parent-lib PATH] [--out profiles/pileup_price.json]"""
import argparse, json, os, subprocess, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

WORKLOADS = {"headline": 1, "genes1000": 1000}
MODES = ("plain", "depth_spliced", "pileup", "both")
PARENT_MODES = ("plain", "depth_spliced")
S_MIN = 8


def child(a):
    import numpy as np
    import torch
    from shark_amd import SharkHip, synth
    dev = torch.device("cuda:0")
    ng = WORKLOADS[a.workload]
    modes = PARENT_MODES if a.parent else MODES
    genes = synth.make_reference(1, 20000) if ng == 1 else synth.make_gencode_like_reference(ng)
    out = {"workload": a.workload, "genes": ng, "pairs": a.pairs, "library": "parent" if a.parent else "this tree",
           "reference_bases": int(sum(len(g) for g in genes))}
    h = SharkHip(k=17, c=0.6, bf_bits=1 << 33)
    h.build([g.tobytes() for g in genes], keep_positions=True)
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
        h.depth_enable_spliced(S_MIN if mode in ("depth_spliced", "both") else 0)
        if not a.parent:
            h.pileup_enable(S_MIN if mode in ("pileup", "both") else 0)
        t = time.perf_counter()
        r = h.classify_device(a.pairs, batch["seq1"].data_ptr(), batch["off1"].data_ptr(), batch["seq2"].data_ptr(), batch["off2"].data_ptr(), 0, 0, max_read_len=150)
        return (time.perf_counter() - t) * 1e3, int(r.n_assoc)

    scale = 1e7 / a.pairs
    for name, batch in (("batch", b), ("worst", w)):
        for mode in modes:                                  # (untimed: allocations, the first batch of a stream)
            run(batch, mode)
        ms = {mode: [] for mode in modes}
        n_assoc = 0
        for _ in range(a.reps):
            for mode in modes:
                t, n_assoc = run(batch, mode)
                ms[mode].append(t)
        out[name] = {"n_assoc": n_assoc, "ms_per_10M_pairs": {mode: round(sorted(v)[len(v) // 2] * scale, 3) for mode, v in ms.items()},
                     "all_ms_per_10M_pairs": {mode: [round(x * scale, 3) for x in v] for mode, v in ms.items()}}
        if not a.parent:
            # what the last batch with both modes on added: the observations per pair are the atomics pileup_kernel issued
            h.pileup_reset()
            run(batch, "pileup")
            counts = h.pileup_all()
            out[name]["pileup_mates_per_batch"] = h.pileup_mates()
            out[name]["observations_per_batch"] = int(counts.sum(dtype=np.uint64))
            out[name]["counters_touched"] = int((counts != 0).sum())
            out[name]["largest_counter"] = int(counts.max()) if counts.size else 0
            h.pileup_reset()
    if not a.parent:
        out["state_bytes"] = {"pileup": 16 * out["reference_bases"], "depth": 4 * (out["reference_bases"] + 1)}
    print("PILEUP_PRICE " + json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=4_000_000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--workloads", default=",".join(WORKLOADS))
    ap.add_argument("--parent-lib", default="")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pileup_price.json"))
    ap.add_argument("--workload", default="")
    ap.add_argument("--parent", action="store_true")
    a = ap.parse_args()
    if a.workload:
        return child(a)
    runs, failed = [], False
    for wl in a.workloads.split(","):
        for parent in ([False, True, False] if a.parent_lib else [False]):          # (this tree, the parent, this tree again: the spread between the two outer runs is the noise)
            env = dict(os.environ)
            if parent:
                env["SHK_LIB_PATH"] = os.path.abspath(a.parent_lib)
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--workload", wl, "--pairs", str(a.pairs), "--reps", str(a.reps)] + (["--parent"] if parent else []),
                               capture_output=True, text=True, timeout=600, env=env)
            line = [x for x in r.stdout.splitlines() if x.startswith("PILEUP_PRICE ")]
            if r.returncode != 0 or not line:
                sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
                runs.append({"workload": wl, "failed": "exit %d" % r.returncode, "stderr_tail": r.stderr[-1000:]})
                print(json.dumps(runs[-1]), flush=True)
                failed = True
                break                                       # (nothing more is started behind a run that failed)
            runs.append(json.loads(line[0][len("PILEUP_PRICE "):]))
            print(json.dumps(runs[-1]), flush=True)
        if failed:
            break
    summary = []
    for wl in a.workloads.split(","):
        mine = [r for r in runs if r.get("workload") == wl and r.get("library") == "this tree" and "batch" in r]
        base = [r for r in runs if r.get("workload") == wl and r.get("library") == "parent" and "batch" in r]
        if not mine:
            continue
        for name in ("batch", "worst"):
            m = mine[0][name]["ms_per_10M_pairs"]
            ref = base[0][name]["ms_per_10M_pairs"] if base else m
            summary.append({"workload": wl, "case": name, "baseline": "parent library" if base else "this tree's unchanged mode",
                            "depth_spliced_ms_at_baseline": ref["depth_spliced"], "plain_ms_at_baseline": ref["plain"],
                            "depth_spliced_over_baseline": round(m["depth_spliced"] / ref["depth_spliced"], 4),
                            "pileup_over_baseline_depth_spliced": round(m["pileup"] / ref["depth_spliced"], 4),
                            "both_over_baseline_depth_spliced": round(m["both"] / ref["depth_spliced"], 4),
                            "pileup_kernel_ms": round(m["both"] - m["depth_spliced"], 3),
                            "pileup_kernel_over_plain": round((m["both"] - m["depth_spliced"]) / ref["plain"], 4)})
    doc = {"what": "wall clock of shk_classify_device per 10 M pairs (2 x 150 bp, k = 17, 50 % on-target): no mode, spliced depth alone, pileup alone and both; the same for "
                   "a batch of one repeated pair; medians of alternating runs on one batch.  pileup_kernel_ms = both - depth_spliced (the two share segments_kernel's launch)",
           "summary": summary, "runs": runs}
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    return 1 if failed else 0


if __name__ == "__main__":
    sys.exit(main())
