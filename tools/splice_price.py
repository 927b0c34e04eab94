#!/usr/bin/env python3
"""What spliced ends (step 3b of alignments mode; DESIGN.md 6 "Spliced ends", 19) cost.  The alignments workload of DESIGN.md 6 --
2 x 150 bp, k = 17, 50 % on-target, resident batches through shk_classify_device, which returns when the stream has drained: wall clock
around the call -- over a SPLICED gene: the index holds a record of 20 000 bases, exons of 180 to 420 bases with introns of 120 to 300
between them, and the pairs are drawn from its transcript, so a mate of 150 bases crosses a junction about every second time.
ms per 10 M pairs, alignments mode at s_min = 8 with end extension (4, 5), with

  parent     a library built from the PARENT commit (--parent-lib): the kernel the step is held against
  off        this tree's library, the step off: must lie inside the parent's run-to-run spread (the same kernel is launched)
  on         this tree's library, the step on at the command's defaults (3, 2, 2); the site list is the sample's own junction table
             (shk_junctions_enable over the same batch at floor 8, read back once: (gene, donor, donor + intron) per row)

One process per library (the library is chosen when the process starts), parent and this tree by turns; within a process the modes
alternate on one batch and the median of --reps is taken.  The shares are counted over the first 200 000 associations' records: mates
with a block, ends whose overhang lies in 3 .. 48 in the records before extension (the ends the step attempts, but for the few a
fourth block rules out), mates with at least one such end, and mates that gain a block.  Writes one JSON document.
usage: python tools/splice_price.py [--pairs 2000000] [--reps 7] [--parent-lib PATH] [--out profiles/splice_price.json]"""
import argparse, json, os, subprocess, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

S_MIN = 8
EXT = (4, 5)
PARAMS = (3, 2, 2)
SAMPLE = 200000


def spliced_reference(np, total=20000, seed=4242):
    """(record, transcript): exons of 180 .. 420 bases, introns of 120 .. 300, about `total` record bases"""
    rng = np.random.default_rng(seed)
    acgt = np.frombuffer(b"ACGT", dtype=np.uint8)
    parts, exons, n = [], [], 0
    while n < total:
        e = acgt[rng.integers(0, 4, size=int(rng.integers(180, 421)))]
        parts.append(e)
        exons.append(e)
        n += len(e)
        if n < total:
            i = acgt[rng.integers(0, 4, size=int(rng.integers(120, 301)))]
            parts.append(i)
            n += len(i)
    return np.concatenate(parts), np.concatenate(exons)


def child(a):
    import numpy as np
    import torch
    from shark_amd import SharkHip, capi, synth
    dev = torch.device("cuda:0")
    record, transcript = spliced_reference(np)
    h = SharkHip(k=17, c=0.6, bf_bits=1 << 33)
    h.build([record.tobytes()], keep_bases=True)
    b = synth.make_pairs_device(a.pairs, [transcript], dev, seed=synth.SEED + 7, read_len=150, on_target=0.5)
    torch.cuda.synchronize()
    has_step = getattr(h.L, "shk_splice_sites_set", None) is not None and a.variant != "parent"

    def classify():
        t = time.perf_counter()
        r = h.classify_device(a.pairs, b["seq1"].data_ptr(), b["off1"].data_ptr(), b["seq2"].data_ptr(), b["off2"].data_ptr(), 0, 0, max_read_len=150)
        return (time.perf_counter() - t) * 1e3, int(r.n_assoc)

    out = {"variant": a.variant, "pairs": a.pairs, "record_bases": int(len(record)), "transcript_bases": int(len(transcript))}
    sites = np.zeros((0, 3), dtype=np.int64)
    if has_step:
        # the sample's own junction table, once
        h.junctions_enable(S_MIN, 1 << 16)
        classify()
        rows = h.junctions_get()
        h.junctions_enable(0, 1 << 16)
        sites = np.unique(np.stack([rows["gene"].astype(np.int64), rows["donor"].astype(np.int64),
                                    rows["donor"].astype(np.int64) + rows["intron"].astype(np.int64)], axis=1), axis=0)
        keep = (sites[:, 1] >= 1) & (sites[:, 2] <= len(record) - 1)
        sites = sites[keep]
        out["junction_rows"], out["sites"] = int(len(rows)), int(len(sites))
        h.splice_sites_set(sites)
    h.alignments_enable(S_MIN)
    modes = ("off", "on") if has_step and len(sites) else ("off",)

    def run(mode, ext=EXT):
        h.alignments_extend(*ext)
        if has_step and len(sites):
            h.alignments_splice(*(PARAMS if mode == "on" else (0, 0, 0)))
        return classify()

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
    out["n_assoc"] = n_assoc
    out["ms_per_10M_pairs"] = {m: round(sorted(v)[len(v) // 2] * scale, 3) for m, v in ms.items()}
    out["all_ms_per_10M_pairs"] = {m: [round(x * scale, 3) for x in v] for m, v in ms.items()}
    if "on" in modes:
        def records(mode, ext):
            run(mode, ext)
            n, ptr = h.alignments_last()
            return capi.alignments_from_device(min(n, SAMPLE), ptr)
        plain, placed = records("off", (0, 0)), records("on", (0, 0))
        nb = plain["n_blocks"].astype(np.int64)
        has = nb > 0
        first_q = plain["block"][..., 0, 1].astype(np.int64)
        last = np.maximum(nb - 1, 0)
        lq = np.take_along_axis(plain["block"][..., 1].astype(np.int64), last[..., None], axis=-1)[..., 0]
        ll = np.take_along_axis(plain["block"][..., 2].astype(np.int64), last[..., None], axis=-1)[..., 0]
        right = 150 - (lq + ll)
        ok = has & (nb <= 3)
        left_in, right_in = ok & (first_q >= PARAMS[0]) & (first_q <= 48), ok & (right >= PARAMS[0]) & (right <= 48)
        ends = int(left_in.sum() + right_in.sum())
        attempted = int((left_in | right_in).sum())
        mates = int(has.sum())
        gained = int((placed["n_blocks"] > plain["n_blocks"]).sum())
        out["sample"] = {"associations": int(len(plain)), "mates_with_a_block": mates, "ends_attempted": ends, "mates_attempted": attempted, "mates_that_gain_a_block": gained,
                         "blocks_gained": int(placed["n_blocks"].astype(np.int64).sum() - nb.sum()),
                         "ends_attempted_per_mate": round(ends / max(mates, 1), 4), "share_of_mates_attempted": round(attempted / max(mates, 1), 4), "share_of_mates_placed": round(gained / max(mates, 1), 4)}
    print("SPLICE_PRICE " + json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=2_000_000)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--parent-lib", default="")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "splice_price.json"))
    ap.add_argument("--variant", default="")
    a = ap.parse_args()
    if a.variant:
        return child(a)
    runs, failed = [], False
    variants = ["parent", "this", "parent", "this"] if a.parent_lib else ["this"]
    for v in variants:
        env = dict(os.environ)
        if v == "parent":
            env["SHK_LIB_PATH"] = os.path.abspath(a.parent_lib)
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--variant", v, "--pairs", str(a.pairs), "--reps", str(a.reps)],
                           capture_output=True, text=True, timeout=400, env=env)
        line = [x for x in r.stdout.splitlines() if x.startswith("SPLICE_PRICE ")]
        if r.returncode != 0 or not line:
            sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
            runs.append({"variant": v, "failed": "exit %d" % r.returncode, "stderr_tail": r.stderr[-1000:]})
            print(json.dumps(runs[-1]), flush=True)
            failed = True
            break                                               # (nothing more is started behind a run that failed)
        runs.append(json.loads(line[0][len("SPLICE_PRICE "):]))
        print(json.dumps(runs[-1]), flush=True)
    med = lambda xs: sorted(xs)[len(xs) // 2] if xs else None  # noqa: E731
    pooled = {}
    for r in runs:
        for mode, v in r.get("all_ms_per_10M_pairs", {}).items():
            pooled.setdefault((r["variant"], mode), []).extend(v)
    parent, off, on = pooled.get(("parent", "off"), []), pooled.get(("this", "off"), []), pooled.get(("this", "on"), [])
    summary = {"parent_ms": med(parent), "parent_min_ms": min(parent) if parent else None, "parent_max_ms": max(parent) if parent else None,
               "off_ms": med(off), "on_ms": med(on)}
    if parent and off:
        summary["off_inside_parent_spread"] = bool(min(parent) <= med(off) <= max(parent))
    if off and on:
        summary["on_over_off"] = round(med(on) / med(off), 4)
    last = next((r for r in reversed(runs) if r.get("variant") == "this" and "sample" in r), None)
    if last:
        summary.update({k: last["sample"][k] for k in ("ends_attempted_per_mate", "share_of_mates_attempted", "share_of_mates_placed")})
        summary["sites"] = last.get("sites")
    doc = {"what": "wall clock of shk_classify_device per 10 M pairs (one spliced gene: a record of 20 000 bases, pairs of 2 x 150 bp from its transcript, k = 17, "
                   "50 % on-target), alignments mode at s_min = 8 with end extension (4, 5): the parent commit's library, this library with spliced ends off and on "
                   "at (3, 2, 2) with the sites of the sample's own junction table; medians over alternating runs on one batch, the libraries by turns in processes of "
                   "their own, their repetitions pooled; shares over the first 200 000 associations' records",
           "summary": summary, "runs": runs}
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(json.dumps(summary), flush=True)
    return 1 if failed else 0


if __name__ == "__main__":
    sys.exit(main())
