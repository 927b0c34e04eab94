#!/usr/bin/env python3
"""What rescue mode costs behind alignments and pairs mode (DESIGN.md 6 "Rescue", 18).  On the headline shape -- one gene of 20 000
bases, 2 x 150 bp, k = 17, 50 % on-target, resident batches through shk_classify_device, which returns when the stream has drained:
wall clock around the call -- ms per 10 M pairs, alignments mode (s_min = 40) and pairs mode (1 024 bins) on, with

  parent     a library built from the PARENT commit (--parent-lib): the tail rescue mode is held against
  off        this tree's library, rescue mode off: must be the parent's tail (no launch, no allocation added)
  on         this tree's library, rescue mode on over the headline sample, in which nearly nothing is attempted: the price of the scan
  on@5, @50  rescue mode off and on over a sample in which that share (percent) of the on-target pairs has a SILENCED mate 2: six
             substitutions 21 bases apart, which leave 32 clean windows of 134 -- fewer than s_min, so the mate gets no block -- and 144
             bases under a k-mer that hits, so the pair stays classified at c = 0.6 (a mate with NO clean window takes the pair's
             coverage below c, and the pair is gone, not rescued; that is why s_min is 40 here and not the 8 of tools/pairs_price.py).
             The difference per attempted association is the price of rescue_kernel (max_cost 16, so that such a mate is rescued
             with the sample's own 1 % substitutions on top)

One process per library (the library is chosen when the process starts); within a process the modes alternate on one batch and the
median of --reps is taken.  Writes one JSON document.  `--variant counters` is the one batch a counter run wants (the 50 % sample with
the mode on, once behind the untimed runs): rocprofv3 --pmc ... -- python tools/rescue_price.py --variant counters --pairs 1000000.
usage: python tools/rescue_price.py [--pairs 4000000] [--reps 7] [--parent-lib PATH] [--out profiles/rescue_price.json]"""
import argparse, json, os, subprocess, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

S_MIN = 40
N_BINS = 1024
MAX_FRAG = 1000
SHARES = (5, 50)


def silence_mate2(torch, b, n, share, read_len, seed):
    """a copy of the batch in which mate 2 of `share` percent of the pairs carries a substitution at 20, 41, 62, ... (every 21st base)"""
    g = torch.Generator(device=b["seq2"].device)
    g.manual_seed(seed)
    rows = torch.rand(n, generator=g, device=b["seq2"].device) < share / 100.0
    seq2 = b["seq2"].clone().reshape(n, read_len)
    lut = torch.arange(256, dtype=torch.uint8, device=seq2.device)
    for x, y in zip(b"ACGT", b"CGTA"):
        lut[x] = y
    cols = torch.arange(20, read_len - 21, 21, device=seq2.device)
    sub = seq2[:, cols]
    seq2[:, cols] = torch.where(rows[:, None], lut[sub.to(torch.int64)], sub)
    out = dict(b)
    out["seq2"] = seq2.reshape(-1)
    torch.cuda.synchronize()
    return out


def child(a):
    import torch
    from shark_amd import SharkHip, synth, capi
    dev = torch.device("cuda:0")
    genes = synth.make_reference(1, 20000)
    h = SharkHip(k=17, c=0.6, bf_bits=1 << 33)
    h.build([g.tobytes() for g in genes], keep_bases=True)
    b = synth.make_pairs_device(a.pairs, genes, dev, seed=synth.SEED + 7, read_len=150, on_target=0.5)
    torch.cuda.synchronize()
    has_rescue = getattr(h.L, "shk_rescue_enable", None) is not None and a.variant != "parent"
    samples = {"headline": b}
    if has_rescue:
        for share in SHARES:
            samples["silenced %d %%" % share] = silence_mate2(torch, b, a.pairs, share, 150, synth.SEED + 11 + share)
    h.alignments_enable(S_MIN)
    h.pairs_enable(20, MAX_FRAG, N_BINS)
    cells = [(s, m) for s in samples for m in (("off", "on") if has_rescue else ("off",))]
    if a.variant == "counters":
        cells, a.reps = [("silenced 50 %", "on")], 0

    def run(sample, mode):
        s = samples[sample]
        if has_rescue:
            h.rescue_enable(20, MAX_FRAG if mode == "on" else 0, 16, 4)
        t = time.perf_counter()
        r = h.classify_device(a.pairs, s["seq1"].data_ptr(), s["off1"].data_ptr(), s["seq2"].data_ptr(), s["off2"].data_ptr(), 0, 0, max_read_len=150)
        return (time.perf_counter() - t) * 1e3, int(r.n_assoc)

    states = {}
    for cell in cells:                                          # (untimed: allocations, the first batch of a stream)
        run(*cell)
        run(*cell)
        if cell[1] == "on":
            n, ptr = h.rescue_last()
            rs = capi.rescues_from_device(n, ptr)
            import numpy as np
            states[cell[0]] = [int(x) for x in np.bincount(rs["state"], minlength=6)]
    ms = {cell: [] for cell in cells}
    n_assoc = {}
    for _ in range(a.reps):
        for cell in cells:
            t, n_assoc[cell[0]] = run(*cell)
            ms[cell].append(t)
    scale = 1e7 / a.pairs
    out = {"variant": a.variant, "pairs": a.pairs, "n_assoc": n_assoc,
           "ms_per_10M_pairs": {"%s / %s" % c: round(sorted(v)[len(v) // 2] * scale, 3) for c, v in ms.items() if v},
           "all_ms_per_10M_pairs": {"%s / %s" % c: [round(x * scale, 3) for x in v] for c, v in ms.items()},
           "rescue_states": states}
    print("RESCUE_PRICE " + json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=4_000_000)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--parent-lib", default="")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rescue_price.json"))
    ap.add_argument("--variant", default="")
    a = ap.parse_args()
    if a.variant:
        return child(a)
    runs, failed = [], False
    # parent and this tree by turns: parent, this, parent, this
    variants = (["parent", "this", "parent", "this"] if a.parent_lib else ["this"])
    for v in variants:
        env = dict(os.environ)
        if v == "parent":
            env["SHK_LIB_PATH"] = os.path.abspath(a.parent_lib)
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--variant", v, "--pairs", str(a.pairs), "--reps", str(a.reps)],
                           capture_output=True, text=True, timeout=400, env=env)
        line = [x for x in r.stdout.splitlines() if x.startswith("RESCUE_PRICE ")]
        if r.returncode != 0 or not line:
            sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
            runs.append({"variant": v, "failed": "exit %d" % r.returncode, "stderr_tail": r.stderr[-1000:]})
            print(json.dumps(runs[-1]), flush=True)
            failed = True
            break                                               # (nothing more is started behind a run that failed)
        runs.append(json.loads(line[0][len("RESCUE_PRICE "):]))
        print(json.dumps(runs[-1]), flush=True)
    med = lambda xs: sorted(xs)[len(xs) // 2] if xs else None  # noqa: E731
    pooled = {}
    for r in runs:
        for cell, v in r.get("all_ms_per_10M_pairs", {}).items():
            pooled.setdefault((r["variant"], cell), []).extend(v)
    summary = {}
    parent = pooled.get(("parent", "headline / off"), [])
    summary["parent_ms"] = med(parent)
    summary["parent_min_ms"], summary["parent_max_ms"] = (min(parent), max(parent)) if parent else (None, None)
    summary["off_ms"] = med(pooled.get(("this", "headline / off"), []))
    summary["on_headline_ms"] = med(pooled.get(("this", "headline / on"), []))
    if summary["off_ms"] and summary["on_headline_ms"]:
        summary["scan_ms"] = round(summary["on_headline_ms"] - summary["off_ms"], 3)
    if parent and summary["off_ms"]:
        summary["off_inside_parent_spread"] = bool(min(parent) <= summary["off_ms"] <= max(parent))
    last = next((r for r in reversed(runs) if r.get("variant") == "this" and "rescue_states" in r), None)
    for share in SHARES:
        name = "silenced %d %%" % share
        off, on = med(pooled.get(("this", name + " / off"), [])), med(pooled.get(("this", name + " / on"), []))
        summary["silenced_%d_off_ms" % share], summary["silenced_%d_on_ms" % share] = off, on
        if last and off and on and name in last["rescue_states"]:
            st = last["rescue_states"][name]
            attempted = sum(st[1:]) * 1e7 / last["pairs"]
            summary["silenced_%d_attempted_per_10M_pairs" % share] = int(attempted)
            summary["silenced_%d_rescued_per_10M_pairs" % share] = int((st[4] + st[5]) * 1e7 / last["pairs"])
            summary["silenced_%d_ns_per_attempted" % share] = round((on - off) * 1e6 / attempted, 2) if attempted else None
    doc = {"what": "wall clock of shk_classify_device per 10 M pairs (headline shape: one gene of 20 000 bases, 2 x 150 bp, k = 17, 50 % on-target), alignments mode "
                   "at s_min = 40 and pairs mode (1 024 bins, max_frag 1 000) on: the parent commit's library, this library with rescue mode off and on (max_frag 1 000, "
                   "max_cost 16, min_gap 4) over the headline sample and over samples in which 5 % and 50 % of the pairs carry a silenced mate 2 (six substitutions 21 "
                   "bases apart); medians over alternating runs on one batch, the libraries by turns in processes of their own, their repetitions pooled",
           "summary": summary, "runs": runs}
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(json.dumps(summary), flush=True)
    return 1 if failed else 0


if __name__ == "__main__":
    sys.exit(main())
