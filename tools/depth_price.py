#!/usr/bin/env python3
"""What depth mode costs, and what its read-outs cost.  Per workload, in one process:

  batch     ms per 10 M pairs (2 x 150 bp, k = 17, 50 % on-target, resident batches through shk_classify_device, which returns
            when the stream has drained: wall clock around the call) in placement mode, and in placement mode with depth mode
            also on -- the two alternating, the same batch
  worst     the same two figures for a batch in which EVERY pair is the same on-target pair of one gene: all mates add at the same
            two entries per mate, the worst case for the atomic adds
  read-outs shk_depth_summary and shk_depth_get_all(device = 1), ms each: behind a batch (the state is scanned first) and again (the
            scan is kept)

Workloads: headline (one gene of 20 000 bases), genes1000, genes60000 (placement's table of that reference has never been built
on a device: whatever happens is recorded).  One process per workload.  Writes one JSON document.
usage: python tools/depth_price.py [--pairs 10000000] [--reps 4] [--workloads headline,genes1000,genes60000] [--out profiles/depth_price.json]"""
import argparse, json, os, subprocess, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

WORKLOADS = {"headline": 1, "genes1000": 1000, "genes60000": 60000}


def child(a):
    import numpy as np
    import torch
    from shark_amd import SharkHip, synth
    dev = torch.device("cuda:0")
    ng = WORKLOADS[a.workload]
    genes = synth.make_reference(1, 20000) if ng == 1 else synth.make_gencode_like_reference(ng)
    out = {"workload": a.workload, "genes": ng, "pairs": a.pairs, "reference_bases": int(sum(len(g) for g in genes))}
    h = SharkHip(k=17, c=0.6, bf_bits=1 << 33)
    t0 = time.perf_counter()
    try:
        h.build([g.tobytes() for g in genes], keep_positions=True)
        h.placement_enable(True)
        h.depth_enable(1)
    except Exception as e:                                  # (recorded, not hidden: the 60 000-gene table may not fit)
        out["failed"] = str(e)
        print("DEPTH_PRICE " + json.dumps(out), flush=True)
        return
    out["build_s"] = round(time.perf_counter() - t0, 3)
    out["probe_mode"] = h.probe_mode()
    free, total = torch.cuda.mem_get_info()
    out["device_bytes_in_use_after_build"] = int(total - free)
    b = synth.make_pairs_device(a.pairs, genes, dev, seed=synth.SEED + 7, read_len=150, on_target=0.5)
    # worst case: one pair of the longest gene, a.pairs times
    g0 = max(genes, key=len)
    at = max(0, min(1000, len(g0) - 250))
    m1 = torch.from_numpy(np.ascontiguousarray(g0[at:at + 150])).to(dev)
    m2 = torch.from_numpy(np.ascontiguousarray(synth_revcomp(g0[at + 100:at + 250]))).to(dev)
    w = {"seq1": m1.repeat(a.pairs), "seq2": m2.repeat(a.pairs), "off1": b["off1"], "off2": b["off2"]}
    torch.cuda.synchronize()

    def run(batch, depth):
        h.depth_enable(1 if depth else 0)
        t = time.perf_counter()
        r = h.classify_device(a.pairs, batch["seq1"].data_ptr(), batch["off1"].data_ptr(), batch["seq2"].data_ptr(), batch["off2"].data_ptr(), 0, 0, max_read_len=150)
        return (time.perf_counter() - t) * 1e3, int(r.n_assoc)

    for name, batch in (("batch", b), ("worst", w)):
        for depth in (False, True):                         # (untimed: allocations, the first batch of a stream)
            run(batch, depth)
        ms = {False: [], True: []}
        for _ in range(a.reps):
            for depth in (False, True):
                t, n_assoc = run(batch, depth)
                ms[depth].append(t)
        scale = 1e7 / a.pairs
        p, d = sorted(ms[False])[len(ms[False]) // 2] * scale, sorted(ms[True])[len(ms[True]) // 2] * scale
        out[name] = {"placement_ms_per_10M_pairs": round(p, 3), "placement_and_depth_ms_per_10M_pairs": round(d, 3), "ratio": round(d / p, 4),
                     "all_placement": [round(x * scale, 3) for x in ms[False]], "all_depth": [round(x * scale, 3) for x in ms[True]], "n_assoc": n_assoc}
    out["depth_mates"] = h.depth_mates()
    tot = int(h.depth_layout()[-1])
    buf = torch.zeros(tot, dtype=torch.int32, device=dev)
    # a read-out behind a batch scans the state first; the scan is then kept until the next batch adds to it.  Both are timed: in
    # front of every "first" read-out one pair is classified with depth mode on (untimed)
    h.depth_enable(1)

    def touch():
        h.classify_device(1, b["seq1"].data_ptr(), b["off1"].data_ptr(), b["seq2"].data_ptr(), b["off2"].data_ptr(), 0, 0, max_read_len=150)

    for name, fn in (("summary", h.depth_summary), ("get_all_device", lambda: h.depth_all(device_ptr=buf.data_ptr()))):
        first, again = [], []
        for _ in range(6):
            touch()
            t = time.perf_counter()
            fn()
            first.append((time.perf_counter() - t) * 1e3)
            t = time.perf_counter()
            fn()
            again.append((time.perf_counter() - t) * 1e3)
        out[name + "_ms"] = round(sorted(first[1:])[2], 3)              # (the first round allocates)
        out[name + "_scan_kept_ms"] = round(sorted(again[1:])[2], 3)
    s = h.depth_summary()
    assert int(s["sum"].sum()) == int(buf.to(torch.int64).sum().item())     # (the two read-outs agree)
    print("DEPTH_PRICE " + json.dumps(out), flush=True)


def synth_revcomp(a):
    import numpy as np
    comp = np.zeros(256, np.uint8)
    for x, y in zip(b"ACGTN", b"TGCAN"):
        comp[x] = y
    return comp[a[::-1]]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=10_000_000)
    ap.add_argument("--reps", type=int, default=4)
    ap.add_argument("--workloads", default=",".join(WORKLOADS))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "depth_price.json"))
    ap.add_argument("--workload", default="")
    a = ap.parse_args()
    if a.workload:
        return child(a)
    runs = []
    for wl in a.workloads.split(","):
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--workload", wl, "--pairs", str(a.pairs), "--reps", str(a.reps)], capture_output=True, text=True,
                           timeout=900)
        line = [x for x in r.stdout.splitlines() if x.startswith("DEPTH_PRICE ")]
        if r.returncode != 0 or not line:
            sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
            runs.append({"workload": wl, "failed": "exit %d" % r.returncode, "stderr_tail": r.stderr[-1000:]})
            print(json.dumps(runs[-1]), flush=True)
            break                                           # (nothing more is started behind a run that failed)
        runs.append(json.loads(line[0][len("DEPTH_PRICE "):]))
        print(json.dumps(runs[-1]), flush=True)
    doc = {"what": "wall clock of shk_classify_device per 10 M pairs (2 x 150 bp, k = 17, 50 % on-target) in placement mode without and with depth mode, the same for a "
                   "batch of one repeated pair, and the read-outs' ms", "runs": runs}
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
