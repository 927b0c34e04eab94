#!/usr/bin/env python3
"""What a missed speculation costs (shark_hip.hip, enqueue_classify): wall clock per call of shk_classify_device on resident streams of the
bench's shape (one gene of 20 kb, 2 x 150 bp, 50 % on-target), a speculating handle against one made under SHK_NO_SPECULATE=1.
usage: python tools/speculation_price.py [pairs] [rounds]
  uniform        every batch uniform: every batch behind the first is speculated on and holds
  alternating    uniform and trimmed batches (20 % of the mates cut to 100 ... 150 bases) by turns: the trimmed one is speculated on
                 and run again -- its launch returns from the guard, so about one extra synchronisation --; the uniform one is not
  compensating   every second batch has reads 0 and 1 of 151 and 149 bases: it passes the guard, a whole kernel pass is wasted"""
import json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from shark_amd import SharkHip, synth

n = int(sys.argv[1]) if len(sys.argv) > 1 else 10_000_000
rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 8
dev = torch.device("cuda:0")
genes = synth.make_reference(1, 20000)


def handle(no_speculate):
    if no_speculate:
        os.environ["SHK_NO_SPECULATE"] = "1"
    else:
        os.environ.pop("SHK_NO_SPECULATE", None)
    h = SharkHip(k=17, c=0.6, bf_bits=1 << 33)
    h.build([g.tobytes() for g in genes])
    os.environ.pop("SHK_NO_SPECULATE", None)
    return h


b = synth.make_pairs_device(n, genes, dev, seed=synth.SEED + 1)
uniform = {"seq1": b["seq1"], "seq2": b["seq2"]}
for m in "12":
    uniform["off" + m] = torch.arange(n + 1, dtype=torch.int64, device=dev) * 150
comp = dict(uniform)
for m, d in (("1", 1), ("2", -1)):
    comp["off" + m] = uniform["off" + m].clone()
    comp["off" + m][1] += d
g = torch.Generator(device=dev); g.manual_seed(7)
trimmed = {}
for key in ("seq1", "seq2"):
    L = torch.randint(100, 151, (n,), generator=g, device=dev)
    L = torch.where(torch.rand(n, generator=g, device=dev) < 0.8, torch.full_like(L, 150), L)
    keep = torch.arange(150, device=dev)[None, :] < L[:, None]
    trimmed[key] = b[key].view(n, 150)[keep].contiguous()
    off = torch.zeros(n + 1, dtype=torch.int64, device=dev)
    off[1:] = torch.cumsum(L, 0)
    trimmed["off" + key[-1]] = off
torch.cuda.synchronize()


def stream(h, batches):
    """-> (median wall clock per call in ms per batch of the cycle, shk_debug_last_speculation per batch of the cycle, associations)"""
    wall, spec, assoc = [[] for _ in batches], [None] * len(batches), [0] * len(batches)
    for r in range(rounds + 1):     # (the first round: buffers, code objects)
        for i, x in enumerate(batches):
            t = time.perf_counter()
            res = h.classify_device(n, x["seq1"].data_ptr(), x["off1"].data_ptr(), x["seq2"].data_ptr(), x["off2"].data_ptr(), max_read_len=150)
            dt = (time.perf_counter() - t) * 1e3
            if r:
                wall[i].append(dt)
            spec[i], assoc[i] = h.debug_last_speculation(), int(res.n_assoc)
    return [round(sorted(w)[len(w) // 2], 4) for w in wall], spec, assoc


out = {"pairs": n, "rounds": rounds}
hs, hn = handle(False), handle(True)
for name, batches in (("uniform", [uniform, uniform]), ("alternating", [uniform, trimmed]), ("compensating", [uniform, comp])):
    ws, ss, as_ = stream(hs, batches)
    wn, sn, an = stream(hn, batches)
    assert as_ == an and sn == [0, 0], (name, as_, an, sn)
    out[name] = {"wall_ms_per_call": ws, "wall_ms_per_call_no_speculate": wn, "speculation": ss, "assoc": as_}
print(json.dumps(out))
