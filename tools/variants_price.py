#!/usr/bin/env python3
"""What a variant call costs on the device, against what a user has to do for the same answer without it.  Per
workload, after --batches accumulated batches (2 x 150 bp, k = 17, 50 % on-target, pileup at s_min = 8, 1 % substitutions in the reads):

  this tree (index built with keep_bases)
    variants_get_ms       wall clock of shk_variants_get with a buffer that holds every site (one call: count, scan, write, copy)
    variants_count_ms     the same with out == NULL (count and scan only)
    variants_summary_ms   wall clock of shk_variants_summary
    achieved_GBps         17 bytes per record base (16 of state, 1 of recbase) over each of the three
    classify_ms           shk_classify_device per batch with pileup on, on an index with and without keep_bases
    finalize_ms           shk_ref_finalize with keep_positions, and with keep_bases
  --parent-lib PATH (a libsharkhip.so built from the parent commit), in a process of its own
    host_route_ms         shk_pileup_get_all into host memory + the same predicate in vectorised numpy against the FASTA's bytes
                          (get_all_ms and numpy_ms apart), the number of sites it finds
    classify_ms           shk_classify_device per batch with pileup on

medians of --reps.  Workloads: headline (one gene of 20 000 bases), genes1000.  Writes one JSON document.
usage: python tools/variants_price.py [--pairs 2000000] [--batches 3] [--reps 5] [--workloads headline,genes1000] [--parent-lib PATH] [--out profiles/variants_price.json]"""
import argparse, ctypes as C, json, os, subprocess, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

WORKLOADS = {"headline": 1, "genes1000": 1000}
S_MIN = 8
PARAMS = (8, 3, 1, 5)


def median(v):
    return sorted(v)[len(v) // 2]


def host_sites(counts, rec_bytes, params):
    """the header's predicate in vectorised numpy: the number of sites (what a caller of the parent's library computes on the host)"""
    import numpy as np
    min_depth, min_alt, num, den = params
    code = np.full(256, 4, dtype=np.uint8)
    for i, ch in enumerate(b"ACGT"):
        code[ch] = code[ch | 0x20] = i
    r = code[rec_bytes]
    ok = r < 4
    T = counts.sum(axis=1, dtype=np.uint64)
    others = counts.astype(np.int64)
    others[np.nonzero(ok)[0], r[ok]] = -1                      # (the record's own count does not compete; argmax takes the first maximum)
    alt = others.max(axis=1).astype(np.uint64)
    site = ok & (T >= min_depth) & (alt >= min_alt) & (alt * np.uint64(den) >= np.uint64(num) * T)
    return int(site.sum())


def child(a):
    import numpy as np
    import torch
    from shark_amd import SharkHip, capi, synth
    dev = torch.device("cuda:0")
    ng = WORKLOADS[a.workload]
    genes = synth.make_reference(1, 20000) if ng == 1 else synth.make_gencode_like_reference(ng)
    bases = int(sum(len(g) for g in genes))
    out = {"workload": a.workload, "genes": ng, "pairs": a.pairs, "batches": a.batches, "library": "parent" if a.parent else "this tree", "reference_bases": bases}
    b = synth.make_pairs_device(a.pairs, genes, dev, seed=synth.SEED + 7, read_len=150, on_target=0.5)
    # 1 % substitutions in the reads, so that there is something to call
    rng = np.random.default_rng(11)
    for key in ("seq1", "seq2"):
        s = b[key].cpu().numpy()
        hit = np.nonzero(rng.random(len(s)) < 0.01)[0]
        s[hit] = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, size=len(hit))]
        b[key] = torch.from_numpy(s).to(dev)
    torch.cuda.synchronize()

    def make(keep_bases):
        h = SharkHip(k=17, c=0.6, bf_bits=1 << 33)
        h.keep_positions()
        if keep_bases:
            h.keep_bases()
        for g in genes:
            h.ref_add(g.tobytes())
        t = time.perf_counter()
        assert h.ref_finalize() == 0
        ms = (time.perf_counter() - t) * 1e3
        h.pileup_enable(S_MIN)
        return h, ms

    def classify(h):
        t = time.perf_counter()
        h.classify_device(a.pairs, b["seq1"].data_ptr(), b["off1"].data_ptr(), b["seq2"].data_ptr(), b["off2"].data_ptr(), 0, 0, max_read_len=150)
        return (time.perf_counter() - t) * 1e3

    def accumulate(h):
        classify(h)                                             # (untimed: allocations, the first batch of a stream)
        h.pileup_reset()
        return [classify(h) for _ in range(max(a.batches, a.reps))]

    fin = {}
    kinds = (False,) if a.parent else (False, True, False, True)
    ctxs = {}
    for kb in kinds:                                            # (finalize alternating; the last context of each kind is kept)
        if kb in ctxs:
            ctxs[kb].close()
        ctxs[kb], ms = make(kb)
        fin.setdefault("keep_bases" if kb else "keep_positions", []).append(round(ms, 3))
    out["finalize_ms"] = fin
    out["classify_ms"] = {("keep_bases" if kb else "keep_positions"): round(median(accumulate(h)), 3) for kb, h in ctxs.items()}
    h = ctxs[True] if not a.parent else ctxs[False]
    out["pileup_mates"] = h.pileup_mates()
    if a.parent:
        rec = np.concatenate([np.frombuffer(g.tobytes(), np.uint8) for g in genes])
        assert int(h.depth_layout()[-1]) == len(rec)            # (every record carries an id on these references)
        t_get, t_np, n = [], [], 0
        for _ in range(a.reps):
            t0 = time.perf_counter()
            counts = h.pileup_all()
            t1 = time.perf_counter()
            n = host_sites(counts, rec, PARAMS)
            t2 = time.perf_counter()
            t_get.append((t1 - t0) * 1e3)
            t_np.append((t2 - t1) * 1e3)
        out["host_route"] = {"get_all_ms": round(median(t_get), 3), "numpy_ms": round(median(t_np), 3), "host_route_ms": round(median(t_get) + median(t_np), 3),
                             "get_all_GBps": round(16 * bases / median(t_get) / 1e6, 2), "sites": n}
    else:
        prm = capi.ShkVariantParams(*PARAMS)
        n = C.c_uint64()
        sites = h.variants(*PARAMS[:2], PARAMS[2:])             # (untimed: the scratch allocations)
        buf = np.zeros(max(len(sites), 1), dtype=capi.VARIANT_DTYPE)
        summ = np.zeros(int(h.index_info()["nidx"]), dtype=capi.GENE_VARIANTS_DTYPE)
        t_get, t_cnt, t_sum = [], [], []
        for _ in range(a.reps):
            t0 = time.perf_counter()
            assert h.L.shk_variants_get(h.h, C.byref(prm), capi._ptr(buf), len(buf), C.byref(n)) == 0
            t1 = time.perf_counter()
            assert h.L.shk_variants_get(h.h, C.byref(prm), None, 0, C.byref(n)) == 0
            t2 = time.perf_counter()
            assert h.L.shk_variants_summary(h.h, C.byref(prm), capi._ptr(summ), len(summ)) == 0
            t3 = time.perf_counter()
            t_get.append((t1 - t0) * 1e3); t_cnt.append((t2 - t1) * 1e3); t_sum.append((t3 - t2) * 1e3)
        gbps = lambda ms: round(17 * bases / ms / 1e6, 2)       # noqa: E731
        out["device_route"] = {"variants_get_ms": round(median(t_get), 4), "variants_count_ms": round(median(t_cnt), 4), "variants_summary_ms": round(median(t_sum), 4),
                               "achieved_GBps": {"get": gbps(median(t_get)), "count": gbps(median(t_cnt)), "summary": gbps(median(t_sum))},
                               "sites": int(n.value), "summary_sites": int(summ["sites"].sum()), "observed": int(summ["observed"].sum()),
                               "mismatches": int(summ["mismatches"].sum())}
        out["added_bytes_keep_bases"] = int(len(h.debug_index_array("recbase")))
    print("VARIANTS_PRICE " + json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=2_000_000)
    ap.add_argument("--batches", type=int, default=3)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--workloads", default=",".join(WORKLOADS))
    ap.add_argument("--parent-lib", default="")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "variants_price.json"))
    ap.add_argument("--workload", default="")
    ap.add_argument("--parent", action="store_true")
    a = ap.parse_args()
    if a.workload:
        return child(a)
    runs, failed = [], False
    for wl in a.workloads.split(","):
        for parent in ([False, True] if a.parent_lib else [False]):
            env = dict(os.environ)
            if parent:
                env["SHK_LIB_PATH"] = os.path.abspath(a.parent_lib)
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--workload", wl, "--pairs", str(a.pairs), "--batches", str(a.batches), "--reps", str(a.reps)]
                               + (["--parent"] if parent else []), capture_output=True, text=True, timeout=500, env=env)
            line = [x for x in r.stdout.splitlines() if x.startswith("VARIANTS_PRICE ")]
            if r.returncode != 0 or not line:
                sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
                runs.append({"workload": wl, "failed": "exit %d" % r.returncode, "stderr_tail": r.stderr[-1000:]})
                print(json.dumps(runs[-1]), flush=True)
                failed = True
                break                                       # (nothing more is started behind a run that failed)
            runs.append(json.loads(line[0][len("VARIANTS_PRICE "):]))
            print(json.dumps(runs[-1]), flush=True)
        if failed:
            break
    summary = []
    for wl in a.workloads.split(","):
        mine = [r for r in runs if r.get("workload") == wl and r.get("library") == "this tree" and "device_route" in r]
        base = [r for r in runs if r.get("workload") == wl and r.get("library") == "parent" and "host_route" in r]
        if not mine:
            continue
        d = mine[0]["device_route"]
        row = {"workload": wl, "reference_bases": mine[0]["reference_bases"], "variants_get_ms": d["variants_get_ms"], "variants_summary_ms": d["variants_summary_ms"],
               "get_GBps": d["achieved_GBps"]["get"], "summary_GBps": d["achieved_GBps"]["summary"], "sites": d["sites"],
               "classify_ms_keep_bases": mine[0]["classify_ms"]["keep_bases"], "classify_ms_keep_positions": mine[0]["classify_ms"]["keep_positions"],
               "finalize_ms_added": round(median(mine[0]["finalize_ms"]["keep_bases"]) - median(mine[0]["finalize_ms"]["keep_positions"]), 3),
               "added_bytes_keep_bases": mine[0]["added_bytes_keep_bases"]}
        if base:
            hr = base[0]["host_route"]
            row.update({"host_route_ms_at_parent": hr["host_route_ms"], "get_all_ms_at_parent": hr["get_all_ms"], "numpy_ms_at_parent": hr["numpy_ms"],
                        "host_over_device": round(hr["host_route_ms"] / d["variants_get_ms"], 1), "sites_agree": hr["sites"] == d["sites"],
                        "classify_ms_at_parent": base[0]["classify_ms"]["keep_positions"]})
        summary.append(row)
    doc = {"what": "wall clock (ms, medians) of shk_variants_get / shk_variants_summary on the accumulated pileup of a few batches, against shk_pileup_get_all to the host "
                   "plus the same predicate in numpy on a library built from the parent commit; shk_classify_device per batch with pileup on, on an index with and "
                   "without keep_bases and at the parent; finalize with and without keep_bases; GB/s = 17 bytes per record base over the call",
           "summary": summary, "runs": runs}
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    return 1 if failed else 0


if __name__ == "__main__":
    sys.exit(main())
