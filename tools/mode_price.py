#!/usr/bin/env python3
"""What evidence mode and candidates mode cost: kernel ms per 10 M pairs (2 x 150 bp, k = 17, 50 % on-target, shk_timing) with the
mode off, evidence on, candidates at m = 2 and candidates at m = 8, on the headline workload (one gene: the exact table in LDS) and
on a 1 000-gene position-table index -- and, with --base-lib, the ordinary and the evidence kernels of another build of the
library (the commit before: tools/build_variant.sh) on the same batches, runs alternating.  One process per library and workload
(SHK_LIB_PATH is read when the binding loads).  Writes one JSON document.
usage: python tools/mode_price.py [--pairs 10000000] [--reps 4] [--rounds 2] [--base-lib tools/variants/parent.so] [--out profiles/candidates_mode_price.json]"""
import argparse, json, os, subprocess, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

WORKLOADS = {"headline": 1, "genes1000": 1000}
MODES = ("off", "evidence", "candidates2", "candidates8")


def child(a):
    import numpy as np
    import torch
    from shark_amd import SharkHip, synth
    dev = torch.device("cuda:0")
    ng = WORKLOADS[a.workload]
    genes = synth.make_reference(1, 20000) if ng == 1 else synth.make_gencode_like_reference(ng)
    b = synth.make_pairs_device(a.pairs, genes, dev, seed=synth.SEED + 7, read_len=150, on_target=0.5)
    torch.cuda.synchronize()
    ptr = {k: (v.data_ptr() if v is not None else 0) for k, v in b.items()}
    h = SharkHip(k=17, c=0.6, bf_bits=1 << 33)
    h.build([g.tobytes() for g in genes])
    out = {"workload": a.workload, "genes": ng, "pairs": a.pairs, "lib": a.tag, "probe_mode": h.probe_mode(), "modes": {}}
    assoc = set()
    for mode in a.modes.split(","):
        if mode != "off" and (h.L.shk_evidence_enable is None or (mode.startswith("candidates") and h.L.shk_candidates_enable is None)):
            continue                                      # (an older library without the mode)
        if h.L.shk_evidence_enable is not None:
            h.evidence_enable(mode == "evidence")
        if h.L.shk_candidates_enable is not None:
            h.candidates_enable(int(mode[10:]) if mode.startswith("candidates") else 0)
        h.timing_enable(False)
        for _ in range(2):                                # (untimed: allocations; the second batch of a stream may take other kernels than the first)
            h.classify_device(a.pairs, ptr["seq1"], ptr["off1"], ptr["seq2"], ptr["off2"], 0, 0, max_read_len=150)
        h.timing_enable(True)
        t0 = h.timing()                                   # (the totals run on across modes: differences)
        for _ in range(a.reps):
            r = h.classify_device(a.pairs, ptr["seq1"], ptr["off1"], ptr["seq2"], ptr["off2"], 0, 0, max_read_len=150)
        tm = h.timing()
        assoc.add(int(r.n_assoc))
        out["modes"][mode] = {"kernel_ms_per_10M_pairs": round((tm["total_ms"] - t0["total_ms"]) / (tm["n_launches"] - t0["n_launches"]) * 1e7 / a.pairs, 3),
                              "launches": int(tm["n_launches"] - t0["n_launches"]),
                              "kernel": h.last_kernel(), "n_assoc": int(r.n_assoc)}
    assert len(assoc) == 1, assoc                         # every mode returns the same associations
    print("MODE_PRICE " + json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=10_000_000)
    ap.add_argument("--reps", type=int, default=4)
    ap.add_argument("--rounds", type=int, default=2, help="how often each (library, workload) process is run; the libraries alternate")
    ap.add_argument("--base-lib", default="", help="another build of libsharkhip.so to run the ordinary and evidence kernels of")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "candidates_mode_price.json"))
    ap.add_argument("--workload", default="")
    ap.add_argument("--tag", default="this")
    ap.add_argument("--modes", default=",".join(MODES))
    a = ap.parse_args()
    if a.workload:
        return child(a)
    runs = []
    for wl in WORKLOADS:
        for rnd in range(a.rounds):
            for tag, lib, modes in (("this", "", ",".join(MODES)), ("base", a.base_lib, "off,evidence")):
                if tag == "base" and not lib:
                    continue
                env = dict(os.environ)
                env.pop("SHK_LIB_PATH", None)
                if lib:
                    env["SHK_LIB_PATH"] = os.path.abspath(lib)
                r = subprocess.run([sys.executable, os.path.abspath(__file__), "--workload", wl, "--tag", tag, "--modes", modes, "--pairs", str(a.pairs),
                                    "--reps", str(a.reps)], env=env, capture_output=True, text=True, timeout=900)
                line = [x for x in r.stdout.splitlines() if x.startswith("MODE_PRICE ")]
                if r.returncode != 0 or not line:
                    sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
                    raise SystemExit("tools/mode_price.py: the %s run of %s failed (exit %d); nothing more is started" % (tag, wl, r.returncode))
                rec = json.loads(line[0][len("MODE_PRICE "):])
                rec["round"] = rnd
                runs.append(rec)
                print(json.dumps(rec), flush=True)
    doc = {"what": "kernel ms per 10 M pairs, 2 x 150 bp, k = 17, 50 % on-target, shk_timing (the main classify launch)", "runs": runs}
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
