#!/usr/bin/env python3
"""What spliced depth and the device junction table cost next to what they replace.  Per workload, in one process:

  batch   ms per 10 M pairs (2 x 150 bp, k = 17, 50 % on-target, resident batches through shk_classify_device, which returns when
          the stream has drained: wall clock around the call) with
            plain              no mode on
            depth_plain        shk_depth_enable(8): placement_kernel + depth_accumulate_kernel
            depth_spliced      shk_depth_enable_spliced(8): segments_kernel at m = 4 + spliced_accumulate_kernel
            segments_m4_copy   shk_segments_enable(4) and the batch's 8 + 160 bytes per association copied to the host inside the
                               timed window: what a caller of the resident pipeline pays today to learn its junctions
            junctions_device   shk_junctions_enable(8, 2^20): segments_kernel at m = 4 + spliced_accumulate_kernel, nothing copied
            both               spliced depth and the table: one segments_kernel, one spliced_accumulate_kernel
          the six alternating, the same batch; the depth state is reset (untimed) between the two kinds

With --parent-lib PATH (a libsharkhip.so built from the parent commit) the three modes that exist there -- plain, depth_plain,
segments_m4_copy -- are measured on that library too, in a process of its own between this tree's, as the baselines `at_parent`.

Workloads: headline (one gene of 20 000 bases), genes1000.  One process per workload and library.  Writes one JSON document.
usage: python tools/spliced_price.py [--pairs 4000000] [--reps 5] [--workloads headline,genes1000] [--parent-lib PATH] [--out profiles/spliced_price.json]"""
import argparse, json, os, subprocess, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

WORKLOADS = {"headline": 1, "genes1000": 1000}
MODES = ("plain", "depth_plain", "depth_spliced", "segments_m4_copy", "junctions_device", "both")
PARENT_MODES = ("plain", "depth_plain", "segments_m4_copy")
S_MIN = 8


def child(a):
    import torch
    from shark_amd import SharkHip, synth
    from shark_amd.capi import segments_from_device
    dev = torch.device("cuda:0")
    ng = WORKLOADS[a.workload]
    modes = PARENT_MODES if a.parent else MODES
    genes = synth.make_reference(1, 20000) if ng == 1 else synth.make_gencode_like_reference(ng)
    out = {"workload": a.workload, "genes": ng, "pairs": a.pairs, "library": "parent" if a.parent else "this tree"}
    h = SharkHip(k=17, c=0.6, bf_bits=1 << 33)
    h.build([g.tobytes() for g in genes], keep_positions=True)
    out["probe_mode"] = h.probe_mode()
    b = synth.make_pairs_device(a.pairs, genes, dev, seed=synth.SEED + 7, read_len=150, on_target=0.5)
    torch.cuda.synchronize()
    state = {"depth": False}

    def run(mode):
        h.segments_enable(4 if mode == "segments_m4_copy" else 0)
        if not a.parent:
            h.junctions_enable(S_MIN if mode in ("junctions_device", "both") else 0, 1 << 20)
        h.depth_enable(0)
        if mode in ("depth_plain", "depth_spliced", "both"):
            if state["depth"]:
                h.depth_reset()                             # (one state holds one kind)
            state["depth"] = True
            h.depth_enable(S_MIN) if mode == "depth_plain" else h.depth_enable_spliced(S_MIN)
        t = time.perf_counter()
        r = h.classify_device(a.pairs, b["seq1"].data_ptr(), b["off1"].data_ptr(), b["seq2"].data_ptr(), b["off2"].data_ptr(), 0, 0, max_read_len=150)
        if mode == "segments_m4_copy":
            segments_from_device(*h.segments_last())
        return (time.perf_counter() - t) * 1e3, int(r.n_assoc)

    for mode in modes:                                      # (untimed: allocations, the first batch of a stream)
        run(mode)
    ms = {mode: [] for mode in modes}
    n_assoc = 0
    for _ in range(a.reps):
        for mode in modes:
            t, n_assoc = run(mode)
            ms[mode].append(t)
    scale = 1e7 / a.pairs
    out["n_assoc"] = n_assoc
    out["ms_per_10M_pairs"] = {mode: round(sorted(v)[len(v) // 2] * scale, 3) for mode, v in ms.items()}
    out["all_ms_per_10M_pairs"] = {mode: [round(x * scale, 3) for x in v] for mode, v in ms.items()}
    if not a.parent:
        out["junction_keys"] = int(len(h.junctions_get()))
        out["depth_mates_last_batch"] = h.depth_mates()
    print("SPLICED_PRICE " + json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=4_000_000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--workloads", default=",".join(WORKLOADS))
    ap.add_argument("--parent-lib", default="")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "spliced_price.json"))
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
            line = [x for x in r.stdout.splitlines() if x.startswith("SPLICED_PRICE ")]
            if r.returncode != 0 or not line:
                sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
                runs.append({"workload": wl, "failed": "exit %d" % r.returncode, "stderr_tail": r.stderr[-1000:]})
                print(json.dumps(runs[-1]), flush=True)
                failed = True
                break                                       # (nothing more is started behind a run that failed)
            runs.append(json.loads(line[0][len("SPLICED_PRICE "):]))
            print(json.dumps(runs[-1]), flush=True)
        if failed:
            break
    summary = []
    for wl in a.workloads.split(","):
        mine = [r for r in runs if r.get("workload") == wl and r.get("library") == "this tree" and "ms_per_10M_pairs" in r]
        base = [r for r in runs if r.get("workload") == wl and r.get("library") == "parent" and "ms_per_10M_pairs" in r]
        if not mine:
            continue
        m = mine[0]["ms_per_10M_pairs"]
        ref = base[0]["ms_per_10M_pairs"] if base else m
        summary.append({"workload": wl, "baselines": "parent library" if base else "this tree's unchanged modes",
                        "depth_spliced_over_depth_plain": round(m["depth_spliced"] / ref["depth_plain"], 4),
                        "junctions_device_over_segments_m4_copy": round(m["junctions_device"] / ref["segments_m4_copy"], 4),
                        "both_over_depth_plain_plus_segments_m4_copy_minus_plain": round(m["both"] / (ref["depth_plain"] + ref["segments_m4_copy"] - ref["plain"]), 4)})
    doc = {"what": "wall clock of shk_classify_device per 10 M pairs (2 x 150 bp, k = 17, 50 % on-target): plain depth against spliced depth, segments mode at m = 4 with "
                   "its records copied to the host against the device junction table, and both new modes together; medians of alternating runs on one batch",
           "summary": summary, "runs": runs}
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    return 1 if failed else 0


if __name__ == "__main__":
    sys.exit(main())
