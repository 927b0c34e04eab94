#!/usr/bin/env python3
"""What pairs mode costs behind alignments mode (DESIGN.md 6 "Pairs", 17).  On the headline shape -- one gene of 20 000 bases, 2 x 150 bp,
k = 17, 50 % on-target, resident batches through shk_classify_device, which returns when the stream has drained: wall clock around the
call -- ms per 10 M pairs with

  parent   a library built from the PARENT commit (--parent-lib), alignments mode on: the tail pairs mode is held against
  align    this tree's library, alignments mode on, pairs mode off: must be the parent's tail (no launch, no allocation added)
  pairs    this tree's library, pairs mode on: pair_kernel behind align_kernel, the histogram staged in LDS
  global   the same with SHK_PAIRS_GLOBAL_ATOMICS=1: one global atomic per pair and per association instead of the LDS stage

One process per library / variant (the library is chosen when the process starts); within a process the modes alternate on one batch and
the median of --reps is taken.  Writes one JSON document.
usage: python tools/pairs_price.py [--pairs 4000000] [--reps 7] [--parent-lib PATH] [--out profiles/pairs_price.json]"""
import argparse, json, os, subprocess, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

S_MIN = 8
N_BINS = 1024


def child(a):
    import torch
    from shark_amd import SharkHip, synth
    dev = torch.device("cuda:0")
    genes = synth.make_reference(1, 20000)
    h = SharkHip(k=17, c=0.6, bf_bits=1 << 33)
    h.build([g.tobytes() for g in genes], keep_bases=True)
    b = synth.make_pairs_device(a.pairs, genes, dev, seed=synth.SEED + 7, read_len=150, on_target=0.5)
    torch.cuda.synchronize()
    has_pairs = h.L.shk_pairs_enable is not None
    modes = ("align", "pairs") if has_pairs and a.variant != "parent" else ("align",)
    h.alignments_enable(S_MIN)

    def run(mode):
        if has_pairs:
            h.pairs_enable(20, 1000, N_BINS if mode == "pairs" else 0)
        t = time.perf_counter()
        r = h.classify_device(a.pairs, b["seq1"].data_ptr(), b["off1"].data_ptr(), b["seq2"].data_ptr(), b["off2"].data_ptr(), 0, 0, max_read_len=150)
        return (time.perf_counter() - t) * 1e3, int(r.n_assoc)

    for mode in modes:                                          # (untimed: allocations, the first batch of a stream)
        run(mode)
        run(mode)
    ms = {mode: [] for mode in modes}
    n_assoc = 0
    for _ in range(a.reps):
        for mode in modes:
            t, n_assoc = run(mode)
            ms[mode].append(t)
    scale = 1e7 / a.pairs
    out = {"variant": a.variant, "pairs": a.pairs, "n_assoc": n_assoc, "ms_per_10M_pairs": {m: round(sorted(v)[len(v) // 2] * scale, 3) for m, v in ms.items()},
           "all_ms_per_10M_pairs": {m: [round(x * scale, 3) for x in v] for m, v in ms.items()}}
    if "pairs" in modes:
        hist, classes = h.fragments(N_BINS)
        out["classes"] = [int(c) for c in classes]
        out["hist_total"] = int(hist.sum())
        out["hist_nonzero_bins"] = int((hist > 0).sum())
    print("PAIRS_PRICE " + json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=4_000_000)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--parent-lib", default="")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pairs_price.json"))
    ap.add_argument("--variant", default="")
    a = ap.parse_args()
    if a.variant:
        return child(a)
    runs, failed = [], False
    variants = (["parent"] if a.parent_lib else []) + ["staged", "global"]
    for v in variants:
        env = dict(os.environ)
        env.pop("SHK_PAIRS_GLOBAL_ATOMICS", None)
        if v == "parent":
            env["SHK_LIB_PATH"] = os.path.abspath(a.parent_lib)
        if v == "global":
            env["SHK_PAIRS_GLOBAL_ATOMICS"] = "1"
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--variant", v, "--pairs", str(a.pairs), "--reps", str(a.reps)],
                           capture_output=True, text=True, timeout=300, env=env)
        line = [x for x in r.stdout.splitlines() if x.startswith("PAIRS_PRICE ")]
        if r.returncode != 0 or not line:
            sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
            runs.append({"variant": v, "failed": "exit %d" % r.returncode, "stderr_tail": r.stderr[-1000:]})
            print(json.dumps(runs[-1]), flush=True)
            failed = True
            break                                               # (nothing more is started behind a run that failed)
        runs.append(json.loads(line[0][len("PAIRS_PRICE "):]))
        print(json.dumps(runs[-1]), flush=True)
    by = {r["variant"]: r.get("ms_per_10M_pairs", {}) for r in runs}
    summary = {"parent_align_ms": by.get("parent", {}).get("align"), "align_ms": by.get("staged", {}).get("align"), "pairs_ms": by.get("staged", {}).get("pairs"),
               "global_align_ms": by.get("global", {}).get("align"), "global_pairs_ms": by.get("global", {}).get("pairs")}
    if summary["align_ms"] and summary["pairs_ms"]:
        summary["pair_kernel_ms"] = round(summary["pairs_ms"] - summary["align_ms"], 3)
        summary["pairs_over_align"] = round(summary["pairs_ms"] / summary["align_ms"], 4)
    if summary["parent_align_ms"] and summary["pairs_ms"]:
        summary["pairs_over_parent"] = round(summary["pairs_ms"] / summary["parent_align_ms"], 4)
        summary["align_over_parent"] = round(summary["align_ms"] / summary["parent_align_ms"], 4)
    if summary["global_align_ms"] and summary["global_pairs_ms"]:
        summary["pair_kernel_global_ms"] = round(summary["global_pairs_ms"] - summary["global_align_ms"], 3)
    doc = {"what": "wall clock of shk_classify_device per 10 M pairs (headline shape: one gene of 20 000 bases, 2 x 150 bp, k = 17, 50 % on-target), alignments mode on "
                   "at s_min = 8: the parent commit's library, this library with pairs mode off and on (1 024 bins), and the variant with one global atomic per pair; "
                   "medians of alternating runs on one batch, one process per library / variant.  pair_kernel_ms = pairs - align within one process",
           "summary": summary, "runs": runs}
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(json.dumps(summary), flush=True)
    return 1 if failed else 0


if __name__ == "__main__":
    sys.exit(main())
