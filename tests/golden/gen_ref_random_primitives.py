#!/usr/bin/env python3
"""Generates tests/golden/ref_random_primitives.npz by running the REAL reference code (oracle/_ref/libsharkref.so, built by
`make -C oracle ref` where the reference tree is present) on seeded random inputs: 2000 k-mers (revcompl / lsappend / rsprepend /
_get_hash at random k and appended character) and 300 random strings over "ACGTacgtNn." (build_kmer from every third start
position).  The file holds the inputs and the reference's outputs; tests/test_oracle.py checks the oracle against it."""
import ctypes as C
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
from oracle import pyoracle  # noqa: E402

R = pyoracle.ref()
assert R is not None, "oracle/_ref/libsharkref.so missing: run `make -C oracle ref`"
rng = np.random.default_rng(99)
prim = {name: [] for name in ("k", "kmer", "c", "revcompl", "lsappend", "rsprepend", "hash")}
for _ in range(2000):
    k = int(rng.integers(1, 32))
    v = int(rng.integers(0, 1 << 62)) & ((1 << (2 * k)) - 1)
    c = int(rng.integers(0, 4))
    for name, x in (("k", k), ("kmer", v), ("c", c), ("revcompl", R.ref_revcompl(v, k)), ("lsappend", R.ref_lsappend(v, c, k)),
                    ("rsprepend", R.ref_rsprepend(v, c, k)), ("hash", R.ref_get_hash(v))):
        prim[name].append(x)
alpha = np.frombuffer(b"ACGTacgtNn.", dtype=np.uint8)
text, str_off, str_k, bk_start, bk_value, bk_pos = [], [0], [], [], [], []
for _ in range(300):
    n = int(rng.integers(0, 120))
    s = alpha[rng.integers(0, len(alpha), size=n)].tobytes()
    k = int(rng.integers(1, 32))
    text.append(s)
    str_off.append(str_off[-1] + n)
    str_k.append(k)
    for p0 in range(0, n + 1, 3):
        q = C.c_int(p0)
        bk_value.append(R.ref_build_kmer(s, n, C.byref(q), k))
        bk_start.append(p0)
        bk_pos.append(q.value)
np.savez_compressed(os.path.join(HERE, "ref_random_primitives.npz"),
                    **{"prim_" + name: np.array(v, dtype=np.uint8 if name in ("k", "c") else np.uint64) for name, v in prim.items()},
                    text=np.frombuffer(b"".join(text), dtype=np.uint8), str_off=np.array(str_off, np.int64), str_k=np.array(str_k, np.uint8),
                    bk_start=np.array(bk_start, np.int32), bk_value=np.array(bk_value, np.int64), bk_pos=np.array(bk_pos, np.int32))
print("wrote ref_random_primitives.npz: %d k-mers, %d strings, %d build_kmer calls" % (len(prim["k"]), len(str_k), len(bk_value)))
