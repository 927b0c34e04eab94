#!/usr/bin/env python3
"""What placement mode costs: ms per 10 M pairs of shk_classify_device (2 x 150 bp, k = 17, 50 % on-target) with the mode off and
on -- the classify kernels' own time (shk_timing: the mode must not change it) and the whole call's wall time (the placement
kernel runs in the tail, which shk_timing does not cover) -- on the headline index (one gene), the 1 000-gene and the 60 000-gene
index; and finalize time and device memory with and without shk_ref_keep_positions.

One child process per (workload, build): "plain" (finalize as always), "keep" (with shk_ref_keep_positions: mode off, then on)
and, with --parent-lib, "parent": the same shapes through another libsharkhip.so (SHK_LIB_PATH; a build of the parent commit,
which lacks the mode's calls) -- the figures "plain" is judged against, from the same session.  Every rep is reported, so the
run-to-run spread of each build is in the output.  Each child runs under its own time limit (per workload); the first failure
ends the run.  Prints one JSON line per child.
usage: python tools/placement_rate.py [--pairs 2000000] [--reps 6] [--workloads headline,genes1000,genes60000]
                                      [--parent-lib PATH] [--limit SECONDS] [--out FILE]"""
import argparse, json, os, subprocess, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

WORKLOADS = {"headline": 1, "genes1000": 1000, "genes60000": 60000}
LIMITS = {"headline": 120, "genes1000": 180, "genes60000": 420}     # seconds per child: one index build, reps x 2 or 3 runs


def child(a):
    import torch
    from shark_amd import SharkHip, synth
    dev = torch.device("cuda:0")
    ng = WORKLOADS[a.workload]
    genes = synth.make_reference(1, 20000) if ng == 1 else synth.make_gencode_like_reference(ng)
    b = synth.make_pairs_device(a.pairs, genes, dev, seed=synth.SEED + 7, read_len=150, on_target=0.5)
    torch.cuda.synchronize()
    ptr = {k: (v.data_ptr() if v is not None else 0) for k, v in b.items()}
    keep = a.build == "keep"

    def run(h, on):
        if h.L.shk_placement_enable is not None:          # (a parent build has no such call, and no mode to switch off)
            h.placement_enable(on)
        h.timing_enable(False)
        for _ in range(2):                                # (untimed: allocations; a stream's second batch may take other kernels)
            h.classify_device(a.pairs, ptr["seq1"], ptr["off1"], ptr["seq2"], ptr["off2"], 0, 0, max_read_len=150)
        h.timing_enable(True)
        walls, kern, seen = [], [], 0.0
        scale = 1e7 / a.pairs
        for _ in range(a.reps):
            t0 = time.perf_counter()
            r = h.classify_device(a.pairs, ptr["seq1"], ptr["off1"], ptr["seq2"], ptr["off2"], 0, 0, max_read_len=150)
            walls.append(round((time.perf_counter() - t0) * 1e3 * scale, 3))
            tm = h.timing()
            kern.append(round((tm["total_ms"] + tm["prepass_ms"] - seen) * scale, 3))
            seen = tm["total_ms"] + tm["prepass_ms"]
        return {"kernel_ms_per_10M_pairs": kern, "call_ms_per_10M_pairs": walls, "kernel": h.last_kernel(), "n_assoc": int(r.n_assoc)}

    free0 = torch.cuda.mem_get_info()[0]
    h = SharkHip(k=17, c=0.6, bf_bits=1 << (33 if ng < 20000 else 36))
    for g in genes:
        h.ref_add(g.tobytes())
    if keep:
        h.keep_positions()
    t0 = time.perf_counter()
    rc = h.ref_finalize()
    dt = time.perf_counter() - t0
    assert rc == 0, rc
    out = {"workload": a.workload, "genes": ng, "pairs": a.pairs, "build": a.build, "finalize_s": round(dt, 4),
           "device_bytes": int(free0 - torch.cuda.mem_get_info()[0]), "probe_mode": h.probe_mode(), "off": run(h, False)}
    if keep:
        out["on"] = run(h, True)
    h.close()
    print("PLACEMENT_RATE " + json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=2_000_000)
    ap.add_argument("--reps", type=int, default=6)
    ap.add_argument("--workloads", default=",".join(WORKLOADS))
    ap.add_argument("--parent-lib", default="", help="a libsharkhip.so of the parent commit: measured first, per workload")
    ap.add_argument("--limit", type=int, default=0, help="seconds per child process (default: by workload)")
    ap.add_argument("--out", default="")
    ap.add_argument("--workload", default="")
    ap.add_argument("--build", default="plain")
    a = ap.parse_args()
    if a.workload:
        return child(a)
    docs = []
    for wl in a.workloads.split(","):
        for build in (["parent"] if a.parent_lib else []) + ["plain", "keep"]:
            env = dict(os.environ)
            env.pop("SHK_LIB_PATH", None)
            if build == "parent":
                env["SHK_LIB_PATH"] = os.path.abspath(a.parent_lib)
            r = subprocess.run(["timeout", "-k", "10", str(a.limit or LIMITS[wl]), sys.executable, os.path.abspath(__file__), "--workload", wl, "--build", build,
                                "--pairs", str(a.pairs), "--reps", str(a.reps)], capture_output=True, text=True, env=env)
            line = [x for x in r.stdout.splitlines() if x.startswith("PLACEMENT_RATE ")]
            if r.returncode != 0 or not line:
                sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
                raise SystemExit("tools/placement_rate.py: the %s run of %s failed (exit %d); nothing more is started" % (build, wl, r.returncode))
            docs.append(json.loads(line[0][len("PLACEMENT_RATE "):]))
            print(json.dumps(docs[-1]), flush=True)
            if a.out:                                     # (rewritten after every child: what was measured survives a later failure)
                with open(a.out, "w") as f:
                    json.dump({"what": "placement mode: ms per 10 M pairs (2 x 150 bp, k = 17, 50 % on-target), finalize time, device memory", "runs": docs}, f, indent=1)
                    f.write("\n")


if __name__ == "__main__":
    main()
