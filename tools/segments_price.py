#!/usr/bin/env python3
"""What segments mode costs next to placement mode.  Per workload, in one process:

  batch   ms per 10 M pairs (2 x 150 bp, k = 17, 50 % on-target, resident batches through shk_classify_device, which returns when
          the stream has drained: wall clock around the call) with no mode on, in placement mode, and in segments mode with m = 1 and
          m = 4 entries per mate (placement mode off) -- the four alternating, the same batch

segments_kernel makes placement_kernel's passes and stores 8 + 40 m bytes per association where that stores 24: a cost well above
placement mode's would point to work per key that the ballots make unnecessary.

Workloads: headline (one gene of 20 000 bases), genes1000.  One process per workload.  Writes one JSON document.
usage: python tools/segments_price.py [--pairs 4000000] [--reps 4] [--workloads headline,genes1000] [--out profiles/segments_price.json]"""
import argparse, json, os, subprocess, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

WORKLOADS = {"headline": 1, "genes1000": 1000}
MODES = ("plain", "placement", "segments_m1", "segments_m4")


def child(a):
    import torch
    from shark_amd import SharkHip, synth
    dev = torch.device("cuda:0")
    ng = WORKLOADS[a.workload]
    genes = synth.make_reference(1, 20000) if ng == 1 else synth.make_gencode_like_reference(ng)
    out = {"workload": a.workload, "genes": ng, "pairs": a.pairs, "reference_bases": int(sum(len(g) for g in genes))}
    h = SharkHip(k=17, c=0.6, bf_bits=1 << 33)
    h.build([g.tobytes() for g in genes], keep_positions=True)
    out["probe_mode"] = h.probe_mode()
    b = synth.make_pairs_device(a.pairs, genes, dev, seed=synth.SEED + 7, read_len=150, on_target=0.5)
    torch.cuda.synchronize()

    def run(mode):
        h.placement_enable(mode == "placement")
        h.segments_enable({"segments_m1": 1, "segments_m4": 4}.get(mode, 0))
        t = time.perf_counter()
        r = h.classify_device(a.pairs, b["seq1"].data_ptr(), b["off1"].data_ptr(), b["seq2"].data_ptr(), b["off2"].data_ptr(), 0, 0, max_read_len=150)
        return (time.perf_counter() - t) * 1e3, int(r.n_assoc)

    for mode in MODES:                                      # (untimed: allocations, the first batch of a stream)
        run(mode)
    ms = {mode: [] for mode in MODES}
    n_assoc = 0
    for _ in range(a.reps):
        for mode in MODES:
            t, n_assoc = run(mode)
            ms[mode].append(t)
    scale = 1e7 / a.pairs
    med = {mode: sorted(v)[len(v) // 2] * scale for mode, v in ms.items()}
    out["n_assoc"] = n_assoc
    out["ms_per_10M_pairs"] = {mode: round(med[mode], 3) for mode in MODES}
    out["all_ms_per_10M_pairs"] = {mode: [round(x * scale, 3) for x in v] for mode, v in ms.items()}
    out["over_placement"] = {mode: round(med[mode] / med["placement"], 4) for mode in ("segments_m1", "segments_m4")}
    out["bytes_stored_per_association"] = {"placement": 24, "segments_m1": 8 + 40 * 1, "segments_m4": 8 + 40 * 4}
    print("SEGMENTS_PRICE " + json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=4_000_000)
    ap.add_argument("--reps", type=int, default=4)
    ap.add_argument("--workloads", default=",".join(WORKLOADS))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "segments_price.json"))
    ap.add_argument("--workload", default="")
    a = ap.parse_args()
    if a.workload:
        return child(a)
    runs = []
    for wl in a.workloads.split(","):
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--workload", wl, "--pairs", str(a.pairs), "--reps", str(a.reps)], capture_output=True, text=True,
                           timeout=600)
        line = [x for x in r.stdout.splitlines() if x.startswith("SEGMENTS_PRICE ")]
        if r.returncode != 0 or not line:
            sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
            runs.append({"workload": wl, "failed": "exit %d" % r.returncode, "stderr_tail": r.stderr[-1000:]})
            print(json.dumps(runs[-1]), flush=True)
            break                                           # (nothing more is started behind a run that failed)
        runs.append(json.loads(line[0][len("SEGMENTS_PRICE "):]))
        print(json.dumps(runs[-1]), flush=True)
    doc = {"what": "wall clock of shk_classify_device per 10 M pairs (2 x 150 bp, k = 17, 50 % on-target) with no mode, in placement mode and in segments mode "
                   "(m = 1, m = 4; placement mode off), medians of alternating runs on one batch", "runs": runs}
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
