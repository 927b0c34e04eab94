"""ctypes binding of libsharkhip.so (include/shark_hip.h).

Plumbing for tests and bench.py; the product is the C ABI itself.  There is no
fallback of any kind: if the HIP library is missing this module raises, and if
no GPU is present every computing call returns an error that is raised here.
"""
import ctypes as C
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("SHK_LIB_PATH") or os.path.join(HERE, "libsharkhip.so")   # (SHK_LIB_PATH: kernel experiments, tools/)

SHK_INLINE_IDS = 4


class ShkParams(C.Structure):
    _fields_ = [("k", C.c_uint32), ("c", C.c_double), ("bf_bits", C.c_uint64),
                ("min_quality", C.c_int32), ("single", C.c_int32), ("device", C.c_int32)]


class ShkIndexInfo(C.Structure):
    _fields_ = [("n_records", C.c_uint64), ("nidx", C.c_uint64), ("bf_bits", C.c_uint64),
                ("n_set_bits", C.c_uint64), ("tot_idx", C.c_uint64), ("n_ref_kmers", C.c_uint64)]


class ShkBatch(C.Structure):
    _fields_ = [("n", C.c_uint64), ("seq1", C.c_void_p), ("off1", C.c_void_p), ("seq2", C.c_void_p),
                ("off2", C.c_void_p), ("qual1", C.c_void_p), ("qual2", C.c_void_p)]


class ShkResult(C.Structure):
    _fields_ = [("n", C.c_uint64), ("gene_off", C.c_void_p), ("gene_ids", C.c_void_p), ("n_assoc", C.c_uint64)]


class ShkTiming(C.Structure):
    _fields_ = [("n_launches", C.c_uint64), ("total_ms", C.c_double), ("last_n_reads", C.c_uint64),
                ("last_n_long", C.c_uint64), ("last_n_tie", C.c_uint64), ("last_n_assoc", C.c_uint64), ("prepass_ms", C.c_double)]


class ShkEvidence(C.Structure):
    _fields_ = [("n", C.c_uint64), ("reads", C.c_void_p)]


class ShkCandidates(C.Structure):
    _fields_ = [("n", C.c_uint64), ("m", C.c_uint32), ("reads", C.c_void_p), ("entries", C.c_void_p)]


class ShkPlacements(C.Structure):
    _fields_ = [("n_assoc", C.c_uint64), ("entries", C.c_void_p)]


class ShkSegments(C.Structure):
    _fields_ = [("n_assoc", C.c_uint64), ("m", C.c_uint32), ("n_keys", C.c_void_p), ("entries", C.c_void_p)]


# shk_gene_depth as a numpy record (24 bytes)
GENE_DEPTH_DTYPE = np.dtype([("len", np.uint32), ("covered", np.uint32), ("max", np.uint32), ("pad", np.uint32), ("sum", np.uint64)])


# shk_junction as a numpy record (24 bytes)
JUNCTION_DTYPE = np.dtype([("gene", np.uint32), ("donor", np.uint32), ("acceptor", np.uint32), ("intron", np.uint32), ("mates", np.uint64)])
JUNCTIONS_DEFAULT_CAPACITY = 1 << 16


class ShkAlignments(C.Structure):
    _fields_ = [("n_assoc", C.c_uint64), ("entries", C.c_void_p)]


# shk_mate_alignment as a numpy record (64 bytes): n_blocks, strand, matches, mismatches and four blocks {x, q, len}
ALIGNMENT_DTYPE = np.dtype([("n_blocks", np.uint32), ("strand", np.uint32), ("matches", np.uint32), ("mismatches", np.uint32),
                            ("block", np.uint32, (4, 3))])
assert ALIGNMENT_DTYPE.itemsize == 64
SAM_DEFAULT_MIN_INTRON = 20


# shk_indel as a numpy record (32 bytes) and shk_indel_stats' counters in their order
INDEL_DTYPE = np.dtype([("gene", np.uint32), ("x", np.uint32), ("kind", np.uint32), ("len", np.uint32), ("seq", np.uint32),
                        ("fwd", np.uint32), ("rev", np.uint32), ("reserved", np.uint32)])
assert INDEL_DTYPE.itemsize == 32
INDEL_STAT_NAMES = ("mates", "deletions", "insertions", "complex_gaps", "long_insertions", "nonbase_insertions", "dropped")
SHK_INDEL_MAX_INS = 12
INDELS_DEFAULT_CAPACITY = 1 << 20
INDELS_DEFAULT_MIN_MATES = 2


class ShkIndelStats(C.Structure):
    _fields_ = [(name, C.c_uint64) for name in INDEL_STAT_NAMES]


class ShkPairs(C.Structure):
    _fields_ = [("n_assoc", C.c_uint64), ("entries", C.c_void_p)]


# shk_pair as a numpy record (32 bytes)
PAIR_DTYPE = np.dtype([("cls", np.uint32), ("left", np.uint32), ("proper", np.uint32), ("mapq", np.uint32),
                       ("tstart", np.int32), ("tend", np.int32), ("introns", np.uint32), ("frag", np.uint32)])
assert PAIR_DTYPE.itemsize == 32
PAIR_CLASS_NAMES = ("none", "mate1", "mate2", "inward", "outward", "tandem")
FRAGMENTS_DEFAULT_MAX = 1000
FRAGMENTS_DEFAULT_BINS = 1024


class ShkRescues(C.Structure):
    _fields_ = [("n_assoc", C.c_uint64), ("entries", C.c_void_p)]


# shk_rescue as a numpy record (16 bytes)
RESCUE_DTYPE = np.dtype([("state", np.uint32), ("cost", np.uint32), ("cost2", np.uint32), ("n_cand", np.uint32)])
assert RESCUE_DTYPE.itemsize == 16
RESCUE_STATE_NAMES = ("not attempted", "no candidate", "too costly", "ambiguous", "mate1 rescued", "mate2 rescued")
RESCUE_MIN_LEN = 32
RESCUE_MAX_LEN = 512
RESCUE_DEFAULT_MAX_COST = 8
RESCUE_DEFAULT_MIN_GAP = 4


class ShkVariantParams(C.Structure):
    _fields_ = [("min_depth", C.c_uint32), ("min_alt", C.c_uint32), ("frac_num", C.c_uint32), ("frac_den", C.c_uint32)]


# shk_variant (32 bytes) and shk_gene_variants (24 bytes) as numpy records
VARIANT_DTYPE = np.dtype([("gene", np.uint32), ("x", np.uint32), ("ref", np.uint32), ("alt", np.uint32), ("n", np.uint32, (4,))])
GENE_VARIANTS_DTYPE = np.dtype([("observed", np.uint64), ("mismatches", np.uint64), ("covered", np.uint32), ("sites", np.uint32)])


class ShkWorkCounters(C.Structure):
    _fields_ = [("n_kmers", C.c_uint64), ("n_hits", C.c_uint64), ("n_list_ids", C.c_uint64), ("n_bases", C.c_uint64)]


# every symbol include/shark_hip.h declares
EXPORTS = [
    "shk_create", "shk_destroy", "shk_strerror", "shk_last_error", "shk_ref_add", "shk_ref_finalize",
    "shk_index_info_get", "shk_index_copy_bf", "shk_index_copy_lists", "shk_classify", "shk_classify_device",
    "shk_gene_counts", "shk_gene_counts_reset", "shk_timing_enable", "shk_timing_get", "shk_count_work",
    "shk_alloc_pinned", "shk_free_pinned", "shk_version", "shk_probe_mode", "shk_gene_counts_allreduce",
    "shk_classify_submit", "shk_classify_wait", "shk_dist_unique_id", "shk_dist_init", "shk_dist_gene_counts_allreduce",
    "shk_dist_info", "shk_measure_random_lookups", "shk_last_kernel", "shk_classify_device_submit",
    "shk_measure_valu_mix",
    "shk_measure_valu_mix_clock",
    "shk_evidence_enable", "shk_evidence_last",
    "shk_candidates_enable", "shk_candidates_last",
    "shk_ref_keep_positions", "shk_placement_enable", "shk_placement_last",
    "shk_segments_enable", "shk_segments_last",
    "shk_depth_enable", "shk_depth_layout", "shk_depth_get", "shk_depth_get_all", "shk_depth_summary", "shk_depth_mates", "shk_depth_reset",
    "shk_depth_enable_spliced", "shk_junctions_enable", "shk_junctions_get", "shk_junctions_reset",
    "shk_pileup_enable", "shk_pileup_get", "shk_pileup_get_all", "shk_pileup_mates", "shk_pileup_reset",
    "shk_pileup_add", "shk_ref_keep_bases", "shk_variants_get", "shk_variants_summary",
    "shk_ref_kmer_table",
    "shk_alignments_enable", "shk_alignments_last", "shk_alignment_cigar", "shk_alignments_extend", "shk_pileup_enable_aligned",
    "shk_pairs_enable", "shk_pairs_last", "shk_fragments_get", "shk_fragments_reset",
    "shk_rescue_enable", "shk_rescue_last",
    "shk_splice_sites_set", "shk_alignments_splice",
    "shk_indels_enable", "shk_indels_get", "shk_indels_stats", "shk_indels_add", "shk_indels_reset",
    "shk_debug_assemble_one",
    "shk_debug_last_speculation",
]
SHK_PIPE_DEPTH = 3
SHK_DIST_ID_BYTES = 128
SHK_MAX_CANDIDATES = 8
SHK_MAX_SEGMENTS = 4
SHK_SPLICE_MAX_OVERHANG = 48
SHK_SPLICE_BACK = 16
SPLICE_SITE_DTYPE = np.dtype([("gene", "<u4"), ("donor", "<u4"), ("acceptor", "<u4")])   # shk_splice_site, 12 bytes

_lib = None


class SharkHipError(RuntimeError):
    pass


def load():
    """Load libsharkhip.so; raises if it has not been built (no fallback)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise SharkHipError("libsharkhip.so is not built (run `python -c 'import __graft_entry__ as g; g.build()'` "
                            "or `make -C shark_amd/csrc`); there is no CPU fallback")
    L = C.CDLL(LIB_PATH)
    p = C.c_void_p
    L.shk_create.restype = C.c_int; L.shk_create.argtypes = [C.POINTER(ShkParams), C.POINTER(p)]
    L.shk_destroy.restype = None; L.shk_destroy.argtypes = [p]
    L.shk_strerror.restype = C.c_char_p; L.shk_strerror.argtypes = [C.c_int]
    L.shk_last_error.restype = C.c_char_p; L.shk_last_error.argtypes = [p]
    L.shk_ref_add.restype = C.c_int; L.shk_ref_add.argtypes = [p, C.c_char_p, C.c_uint64]
    L.shk_ref_finalize.restype = C.c_int; L.shk_ref_finalize.argtypes = [p]
    L.shk_index_info_get.restype = C.c_int; L.shk_index_info_get.argtypes = [p, C.POINTER(ShkIndexInfo)]
    L.shk_index_copy_bf.restype = C.c_int; L.shk_index_copy_bf.argtypes = [p, p, C.c_uint64]
    L.shk_index_copy_lists.restype = C.c_int; L.shk_index_copy_lists.argtypes = [p, p, p]
    L.shk_classify.restype = C.c_int; L.shk_classify.argtypes = [p, C.POINTER(ShkBatch), C.POINTER(ShkResult)]
    L.shk_classify_device.restype = C.c_int
    L.shk_classify_device.argtypes = [p, C.POINTER(ShkBatch), C.c_uint32, C.POINTER(ShkResult)]
    L.shk_gene_counts.restype = C.c_int; L.shk_gene_counts.argtypes = [p, p, C.c_uint32]
    L.shk_gene_counts_reset.restype = C.c_int; L.shk_gene_counts_reset.argtypes = [p]
    L.shk_timing_enable.restype = C.c_int; L.shk_timing_enable.argtypes = [p, C.c_int]
    L.shk_timing_get.restype = C.c_int; L.shk_timing_get.argtypes = [p, C.POINTER(ShkTiming)]
    L.shk_count_work.restype = C.c_int; L.shk_count_work.argtypes = [p, C.POINTER(ShkBatch), C.POINTER(ShkWorkCounters)]
    L.shk_alloc_pinned.restype = p; L.shk_alloc_pinned.argtypes = [C.c_size_t]
    L.shk_free_pinned.restype = None; L.shk_free_pinned.argtypes = [p]
    L.shk_version.restype = C.c_char_p; L.shk_version.argtypes = []
    L.shk_probe_mode.restype = C.c_char_p; L.shk_probe_mode.argtypes = [p]
    L.shk_last_kernel.restype = C.c_char_p; L.shk_last_kernel.argtypes = [p]
    L.shk_gene_counts_allreduce.restype = C.c_int; L.shk_gene_counts_allreduce.argtypes = [C.POINTER(p), C.c_int, p, C.c_uint32]
    L.shk_classify_submit.restype = C.c_int; L.shk_classify_submit.argtypes = [p, C.POINTER(ShkBatch), C.POINTER(C.c_uint64)]
    L.shk_classify_wait.restype = C.c_int; L.shk_classify_wait.argtypes = [p, C.c_uint64, C.POINTER(ShkResult)]
    # The later entry points, prototype by prototype: a library variant named by SHK_LIB_PATH (A/B timing, tools/build_variant.sh) may
    # come from an older tree and lack some of them -- such a name is set to None ("not callable") and every name that exists gets its
    # prototype, so that no call ever goes through ctypes' default int conversion.  The product library is checked symbol by symbol
    # in tests/test_cabi_cpu.py; without SHK_LIB_PATH a missing symbol is an error here as well.
    later = {
        "shk_classify_device_submit": (C.c_int, [p, C.POINTER(ShkBatch), C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(C.c_uint64)]),
        "shk_dist_unique_id": (C.c_int, [p]),
        "shk_dist_init": (C.c_int, [p, p, C.c_int, C.c_int]),
        "shk_dist_gene_counts_allreduce": (C.c_int, [p, p, C.c_uint32]),
        "shk_dist_info": (C.c_int, [p, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
        "shk_measure_random_lookups": (C.c_int, [p, C.c_uint64, C.c_uint64, C.c_int, C.POINTER(C.c_double)]),
        "shk_measure_valu_mix": (C.c_int, [p, C.c_int, C.c_uint32, C.POINTER(C.c_double), C.POINTER(C.c_uint64)]),
        "shk_measure_valu_mix_clock": (C.c_int, [p, C.c_int, C.c_uint32, C.POINTER(C.c_double), C.POINTER(C.c_uint64), C.POINTER(C.c_double)]),
        "shk_evidence_enable": (C.c_int, [p, C.c_int]),
        "shk_evidence_last": (C.c_int, [p, C.POINTER(ShkEvidence)]),
        "shk_candidates_enable": (C.c_int, [p, C.c_uint32]),
        "shk_candidates_last": (C.c_int, [p, C.POINTER(ShkCandidates)]),
        "shk_ref_keep_positions": (C.c_int, [p]),
        "shk_placement_enable": (C.c_int, [p, C.c_int]),
        "shk_placement_last": (C.c_int, [p, C.POINTER(ShkPlacements)]),
        "shk_segments_enable": (C.c_int, [p, C.c_uint32]),
        "shk_segments_last": (C.c_int, [p, C.POINTER(ShkSegments)]),
        "shk_depth_enable": (C.c_int, [p, C.c_uint32]),
        "shk_depth_layout": (C.c_int, [p, p, C.c_uint32]),
        "shk_depth_get": (C.c_int, [p, C.c_uint32, p, C.c_uint64]),
        "shk_depth_get_all": (C.c_int, [p, p, C.c_uint64, C.c_int]),
        "shk_depth_summary": (C.c_int, [p, p, C.c_uint32]),
        "shk_depth_mates": (C.c_int, [p, C.POINTER(C.c_uint64)]),
        "shk_depth_reset": (C.c_int, [p]),
        "shk_depth_enable_spliced": (C.c_int, [p, C.c_uint32]),
        "shk_junctions_enable": (C.c_int, [p, C.c_uint32, C.c_uint64]),
        "shk_junctions_get": (C.c_int, [p, p, C.c_uint64, C.POINTER(C.c_uint64)]),
        "shk_junctions_reset": (C.c_int, [p]),
        "shk_pileup_enable": (C.c_int, [p, C.c_uint32]),
        "shk_pileup_get": (C.c_int, [p, C.c_uint32, p, C.c_uint64]),
        "shk_pileup_get_all": (C.c_int, [p, p, C.c_uint64, C.c_int]),
        "shk_pileup_mates": (C.c_int, [p, C.POINTER(C.c_uint64)]),
        "shk_pileup_reset": (C.c_int, [p]),
        "shk_pileup_add": (C.c_int, [p, p, C.c_uint64, C.c_uint64, C.c_int]),
        "shk_ref_keep_bases": (C.c_int, [p]),
        "shk_ref_kmer_table": (C.c_int, [p, C.c_int]),
        "shk_variants_get": (C.c_int, [p, C.POINTER(ShkVariantParams), p, C.c_uint64, C.POINTER(C.c_uint64)]),
        "shk_variants_summary": (C.c_int, [p, C.POINTER(ShkVariantParams), p, C.c_uint32]),
        "shk_alignments_enable": (C.c_int, [p, C.c_uint32]),
        "shk_alignments_extend": (C.c_int, [p, C.c_uint32, C.c_uint32]),
        "shk_pileup_enable_aligned": (C.c_int, [p, C.c_uint32]),
        "shk_alignments_last": (C.c_int, [p, C.POINTER(ShkAlignments)]),
        "shk_alignment_cigar": (C.c_int, [p, C.c_uint32, C.c_uint32, C.c_char_p, C.c_size_t, C.POINTER(C.c_uint32)]),
        "shk_pairs_enable": (C.c_int, [p, C.c_uint32, C.c_uint32, C.c_uint32]),
        "shk_pairs_last": (C.c_int, [p, C.POINTER(ShkPairs)]),
        "shk_fragments_get": (C.c_int, [p, p, C.c_uint32, p]),
        "shk_fragments_reset": (C.c_int, [p]),
        "shk_rescue_enable": (C.c_int, [p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32]),
        "shk_rescue_last": (C.c_int, [p, C.POINTER(ShkRescues)]),
        "shk_splice_sites_set": (C.c_int, [p, p, C.c_uint64]),
        "shk_alignments_splice": (C.c_int, [p, C.c_uint32, C.c_uint32, C.c_uint32]),
        "shk_indels_enable": (C.c_int, [p, C.c_uint32, C.c_uint32, C.c_uint64]),
        "shk_indels_get": (C.c_int, [p, C.c_uint32, p, C.c_uint64, C.POINTER(C.c_uint64)]),
        "shk_indels_stats": (C.c_int, [p, C.POINTER(ShkIndelStats)]),
        "shk_indels_add": (C.c_int, [p, p, C.c_uint64, C.POINTER(ShkIndelStats)]),
        "shk_indels_reset": (C.c_int, [p]),
        "shk_debug_assemble_one": (C.c_int, [p, p, C.c_uint64, C.c_uint32, C.c_uint32, C.c_uint64, C.c_uint32, C.c_int, C.c_int, p, p, p,
                                             C.POINTER(C.c_uint64), p]),
        "shk_debug_last_speculation": (C.c_int, [p]),
    }
    variant = bool(os.environ.get("SHK_LIB_PATH"))
    for name, (res, args) in later.items():
        if hasattr(L, name):
            fn = getattr(L, name)
            fn.restype = res
            fn.argtypes = args
        elif variant:
            setattr(L, name, None)
        else:
            raise SharkHipError("libsharkhip.so lacks %s: rebuild it (make -C shark_amd/csrc)" % name)
    _lib = L
    return L


def _u8(a):
    if a is None:
        return None
    if isinstance(a, (bytes, bytearray)):
        return np.frombuffer(bytes(a), dtype=np.uint8)
    return np.ascontiguousarray(a, dtype=np.uint8)


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


class SharkHip:
    """One classification context on one GPU (shk_ctx)."""

    def __init__(self, k=17, c=0.6, bf_bits=1 << 33, min_quality=0, single=False, device=0):
        self.L = load()
        self.h = C.c_void_p()
        prm = ShkParams(k, c, bf_bits, min_quality, int(bool(single)), device)
        rc = self.L.shk_create(C.byref(prm), C.byref(self.h))
        if rc != 0:
            self.h = C.c_void_p()
            raise SharkHipError("shk_create: %s" % self.L.shk_strerror(rc).decode())
        self.k, self.c, self.bf_bits = k, c, bf_bits
        self._last_on_host = True     # which memory space the last result handed out lives in (evidence_last)

    def _check(self, rc, what):
        if rc != 0:
            raise SharkHipError("%s: %s (%s)" % (what, self.L.shk_strerror(rc).decode(),
                                                 self.L.shk_last_error(self.h).decode()))

    def close(self):
        if self.h:
            self.L.shk_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- index -----------------------------------------------------------------
    def ref_add(self, seq):
        return self.L.shk_ref_add(self.h, bytes(seq), len(seq))

    def ref_finalize(self):
        return self.L.shk_ref_finalize(self.h)

    def keep_positions(self):
        """ask ref_finalize / build to build placement mode's table as well (before the index is finalized only)"""
        self._check(self.L.shk_ref_keep_positions(self.h), "shk_ref_keep_positions")

    def keep_bases(self):
        """ask ref_finalize / build to keep the records' bases on the device as well (variants, variants_summary); implies
        keep_positions; before the index is finalized only"""
        self._check(self.L.shk_ref_keep_bases(self.h), "shk_ref_keep_bases")

    def kmer_table(self, on):
        """whether ref_finalize / build may build the one-gene index's table keyed by the canonical k-mer (on by default; before the
        index is finalized only)"""
        self._check(self.L.shk_ref_kmer_table(self.h, 1 if on else 0), "shk_ref_kmer_table")

    def build(self, seqs, keep_positions=False, keep_bases=False):
        if keep_positions:
            self.keep_positions()
        if keep_bases:
            self.keep_bases()
        for s in seqs:
            self._check(self.ref_add(s), "shk_ref_add")
        self._check(self.ref_finalize(), "shk_ref_finalize")
        return self.index_info()

    def index_info(self):
        info = ShkIndexInfo()
        self._check(self.L.shk_index_info_get(self.h, C.byref(info)), "shk_index_info_get")
        return {f: getattr(info, f) for f, _ in ShkIndexInfo._fields_}

    def probe_mode(self):
        return self.L.shk_probe_mode(self.h).decode()

    def last_kernel(self):
        """the classify kernel instantiation the last batch ran (rocprofv3's name for it)"""
        return self.L.shk_last_kernel(self.h).decode()

    def debug_last_speculation(self):
        """test-only: 0 = the last batch was not speculated on, 1 = speculated and held, 2 = speculated and run again (include/shark_hip.h)"""
        return int(self.L.shk_debug_last_speculation(self.h))

    def copy_bf(self):
        nw = (self.bf_bits + 63) // 64
        w = np.zeros(nw, dtype=np.uint64)
        self._check(self.L.shk_index_copy_bf(self.h, _ptr(w), nw), "shk_index_copy_bf")
        return w

    def copy_lists(self):
        info = self.index_info()
        off = np.zeros(info["n_set_bits"] + 1, dtype=np.uint32)
        ids = np.zeros(max(info["tot_idx"], 1), dtype=np.uint16)
        self._check(self.L.shk_index_copy_lists(self.h, _ptr(off), _ptr(ids)), "shk_index_copy_lists")
        return off, ids[:info["tot_idx"]]

    # ---- test-only read-back of the derived index arrays (shk_debug_index_array: exported, not in the header, not in EXPORTS) ----
    DEBUG_ARRAYS = {"rank_w": np.uint32, "ent": np.uint32, "ids": np.uint16, "sum32": np.uint32, "lsum32": np.uint32,
                    "lbig32": np.uint32, "tab": np.uint64, "atab": np.uint64, "ltab": np.uint32, "ref2": np.uint32,
                    "refpay": np.uint32, "refext": np.uint32, "refmul": np.uint32, "recbase": np.uint8,
                    "kxtab": np.uint8, "kxkeys": np.uint64, "kxmeta": np.uint64,
                    "ptab": np.uint32, "pdir": np.uint32, "pmeta": np.uint64,      # (ptab: 4 words per entry; pmeta: DEBUG_PMETA)
                    "ktab": np.uint64, "ktmeta": np.uint64}                        # (ktab: the slots as allocated; ktmeta: DEBUG_KTMETA)
    DEBUG_PMETA = ("ptab_lg", "ptab_n")
    DEBUG_KTMETA = ("ktab_lg", "ktab_w", "ktab_keys")
    DEBUG_META = ("tab_lg", "sum_shift", "lsum_shift", "lbig_shift", "ltab_mul", "ref_total", "n_set", "tot_idx", "pow2", "wrap",
                  "ent_len", "ids_len", "bf_bits", "bf_words64", "sum_bits", "ktab_lg")
    DEBUG_KXMETA = ("kx_in_use", "kx_m1", "kx_m2", "kx_keys", "kx_enum_us", "kx_build_us")

    def _debug_read(self, name, dtype):
        fn = self.L.shk_debug_index_array
        fn.restype = C.c_int
        fn.argtypes = [C.c_void_p, C.c_char_p, C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64)]
        need = C.c_uint64()
        self._check(fn(self.h, name.encode(), None, 0, C.byref(need)), "shk_debug_index_array(%s)" % name)
        a = np.zeros(need.value // np.dtype(dtype).itemsize, dtype=dtype)
        if need.value:
            self._check(fn(self.h, name.encode(), _ptr(a), need.value, C.byref(need)), "shk_debug_index_array(%s)" % name)
        return a

    def debug_index_array(self, name):
        """the named device array as allocated, padding included (`ent`: u32 words, two per entry -- start, len | gene0 << 16);
        empty when this index does not carry it"""
        return self._debug_read(name, self.DEBUG_ARRAYS[name])

    def debug_index_meta(self):
        """the scalars that decode the arrays"""
        return dict(zip(self.DEBUG_META, (int(x) for x in self._debug_read("meta", np.uint64))))

    def debug_kx_meta(self):
        """the k-mer keyed table of a one-gene index (kmer_table.hpp): is it in use, its multipliers, its key count, what building it took"""
        return dict(zip(self.DEBUG_KXMETA, (int(x) for x in self._debug_read("kxmeta", np.uint64))))

    def debug_ktab_meta(self):
        """the minimiser-bucketed table (tests/ktab_audit.py): log2 of its buckets (0 = not built), the minimiser's length, its key count"""
        return dict(zip(self.DEBUG_KTMETA, (int(x) for x in self._debug_read("ktmeta", np.uint64))))

    # ---- test-only runs of the device scan and radix sort (shk_debug_scan_u32 / shk_debug_sort_u64: as shk_debug_index_array) ----
    DEBUG_SCAN_GUARDS = ("in_front", "in_back", "out_front", "out_back", "temp_front", "temp_back")
    DEBUG_SORT_GUARDS = ("a_front", "a_back", "b_front", "b_back", "hist_front", "hist_back", "scan_tmp_front", "scan_tmp_back")

    def debug_scan_u32(self, values, in_off=0, out_off=0, in_place=False):
        """exclusive_scan_u32 over `values` (uint32) with in / out placed in_off / out_off words behind a 16-byte aligned address
        (in_place: out is in).  Returns (out, total, in_after, guards): out and in_after as uint32 arrays, the 64-bit total as an
        int, guards = changed guard words per band in the order of DEBUG_SCAN_GUARDS (uint32; all zero on a clean run)"""
        fn = self.L.shk_debug_scan_u32
        fn.restype = C.c_int
        fn.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32, C.c_uint32, C.c_int, C.c_void_p, C.c_void_p,
                       C.POINTER(C.c_uint64), C.c_void_p]
        a = np.ascontiguousarray(values, dtype=np.uint32)
        out, after = np.zeros(len(a), dtype=np.uint32), np.zeros(len(a), dtype=np.uint32)
        guards = np.zeros(len(self.DEBUG_SCAN_GUARDS), dtype=np.uint32)
        total = C.c_uint64()
        self._check(fn(self.h, _ptr(a), len(a), in_off, out_off, 1 if in_place else 0, _ptr(out), _ptr(after), C.byref(total), _ptr(guards)),
                    "shk_debug_scan_u32")
        return out, int(total.value), after, guards

    def debug_sort_u64(self, keys, end_bit=64):
        """radix_sort_u64 over `keys` (uint64).  Returns (sorted, which, guards): the keys of the buffer the sort returned, which one
        that was (0 = a, the input's; 1 = b), guards = changed guard words per band in the order of DEBUG_SORT_GUARDS"""
        fn = self.L.shk_debug_sort_u64
        fn.restype = C.c_int
        fn.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32, C.c_void_p, C.POINTER(C.c_int), C.c_void_p]
        a = np.ascontiguousarray(keys, dtype=np.uint64)
        out = np.zeros(len(a), dtype=np.uint64)
        guards = np.zeros(len(self.DEBUG_SORT_GUARDS), dtype=np.uint32)
        which = C.c_int(-1)
        self._check(fn(self.h, _ptr(a), len(a), end_bit, _ptr(out), C.byref(which), _ptr(guards)), "shk_debug_sort_u64")
        return out, int(which.value), guards

    # ---- test-only run of the one-record assembly (shk_debug_assemble_one, include/shark_hip.h) ----
    DEBUG_ASSEMBLE_GUARDS = ("count_front", "count_back", "off_front", "off_back", "temp_front", "temp_back", "ids_front", "ids_back",
                             "counters_front", "counters_back", "gene0_front", "gene0_back")
    DEBUG_FILL16 = 0x0FF2
    DEBUG_COUNTER_WORDS = 16
    DEBUG_CTR_LONG, DEBUG_CTR_OVERFLOW, DEBUG_CTR_ASSOC_LO, DEBUG_CTR_ASSOC_HI = 0, 2, 6, 7

    def debug_assemble_one(self, count, gene_ids_cap, count_off=0, off_off=0, ctr_long=0, skip_if_long=False, count_genes=True):
        """the three launches that assemble a one-record index's result over `count` (uint32, at least one word).  Returns (gene_off,
        gene_ids, counters, gene0_added, guards): gene_off uint32[len(count)]; gene_ids uint16[gene_ids_cap], DEBUG_FILL16 where nothing was
        written; the counter block; what was added to gene 0's counter; changed guard words per band in the order of DEBUG_ASSEMBLE_GUARDS"""
        a = np.ascontiguousarray(count, dtype=np.uint32)
        gene_off = np.zeros(len(a), dtype=np.uint32)
        gene_ids = np.zeros(max(int(gene_ids_cap), 1), dtype=np.uint16)
        counters = np.zeros(self.DEBUG_COUNTER_WORDS, dtype=np.uint32)
        guards = np.zeros(len(self.DEBUG_ASSEMBLE_GUARDS), dtype=np.uint32)
        added = C.c_uint64()
        self._check(self.L.shk_debug_assemble_one(self.h, _ptr(a), len(a), count_off, off_off, int(gene_ids_cap), ctr_long, int(bool(skip_if_long)),
                                                  int(bool(count_genes)), _ptr(gene_off), _ptr(gene_ids), _ptr(counters), C.byref(added), _ptr(guards)),
                    "shk_debug_assemble_one")
        return gene_off, gene_ids[:int(gene_ids_cap)], counters, int(added.value), guards

    # ---- classification --------------------------------------------------------
    def _host_batch(self, seq1, off1, seq2, off2, qual1, qual2):
        seq1, seq2, qual1, qual2 = _u8(seq1), _u8(seq2), _u8(qual1), _u8(qual2)
        off1 = np.ascontiguousarray(off1, dtype=np.uint64)
        off2 = np.ascontiguousarray(off2, dtype=np.uint64) if off2 is not None else None
        n = len(off1) - 1
        keep = (seq1, off1, seq2, off2, qual1, qual2)      # the library reads them until the ticket is waited for
        return ShkBatch(n, _ptr(seq1), _ptr(off1), _ptr(seq2), _ptr(off2), _ptr(qual1), _ptr(qual2)), keep

    @staticmethod
    def _host_result(r, copy=True):
        n, tot = int(r.n), int(r.n_assoc)
        gene_off = np.ctypeslib.as_array(C.cast(r.gene_off, C.POINTER(C.c_uint32)), shape=(n + 1,))
        ids = np.ctypeslib.as_array(C.cast(r.gene_ids, C.POINTER(C.c_uint16)), shape=(tot,)) if tot else np.zeros(0, np.uint16)
        return (gene_off.copy(), ids.copy()) if copy else (gene_off, ids)

    def classify(self, seq1, off1, seq2=None, off2=None, qual1=None, qual2=None):
        """host SoA batch -> (gene_off[n+1] u32, gene_ids u16)"""
        b, keep = self._host_batch(seq1, off1, seq2, off2, qual1, qual2)
        r = ShkResult()
        self._check(self.L.shk_classify(self.h, C.byref(b), C.byref(r)), "shk_classify")
        self._last_on_host = True
        return self._host_result(r)

    def submit(self, seq1, off1, seq2=None, off2=None, qual1=None, qual2=None):
        """pipelined form: returns a ticket (an object that also keeps the host arrays alive)"""
        b, keep = self._host_batch(seq1, off1, seq2, off2, qual1, qual2)
        t = C.c_uint64()
        self._check(self.L.shk_classify_submit(self.h, C.byref(b), C.byref(t)), "shk_classify_submit")
        return (t.value, keep)

    def wait(self, ticket, copy=True):
        r = ShkResult()
        self._check(self.L.shk_classify_wait(self.h, ticket[0], C.byref(r)), "shk_classify_wait")
        self._last_on_host = True
        return self._host_result(r, copy)

    def classify_device(self, n, seq1, off1, seq2=0, off2=0, qual1=0, qual2=0, max_read_len=0):
        """device pointers (ints) -> ShkResult with DEVICE pointers"""
        b = ShkBatch(n, seq1 or None, off1 or None, seq2 or None, off2 or None, qual1 or None, qual2 or None)
        r = ShkResult()
        self._check(self.L.shk_classify_device(self.h, C.byref(b), max_read_len, C.byref(r)), "shk_classify_device")
        self._last_on_host = False
        return r

    def submit_device(self, n, seq1, off1, seq2=0, off2=0, qual1=0, qual2=0, max_read_len=0, uniform_len1=0, uniform_len2=0):
        """device pointers (ints) -> ticket; wait_device(ticket) gives the ShkResult with DEVICE pointers"""
        b = ShkBatch(n, seq1 or None, off1 or None, seq2 or None, off2 or None, qual1 or None, qual2 or None)
        t = C.c_uint64()
        self._check(self.L.shk_classify_device_submit(self.h, C.byref(b), max_read_len, uniform_len1, uniform_len2, C.byref(t)), "shk_classify_device_submit")
        return t.value

    def wait_device(self, ticket):
        r = ShkResult()
        self._check(self.L.shk_classify_wait(self.h, ticket, C.byref(r)), "shk_classify_wait")
        self._last_on_host = False
        return r

    def count_work(self, n, seq1, off1, seq2=0, off2=0, qual1=0, qual2=0):
        b = ShkBatch(n, seq1 or None, off1 or None, seq2 or None, off2 or None, qual1 or None, qual2 or None)
        w = ShkWorkCounters()
        self._check(self.L.shk_count_work(self.h, C.byref(b), C.byref(w)), "shk_count_work")
        return {f: getattr(w, f) for f, _ in ShkWorkCounters._fields_}

    # ---- evidence: per read the best gene's coverage, its k-mer count, the read's valid length --------
    def evidence_enable(self, on=True):
        """batches submitted from now on carry evidence (and run the full-probe kernels); refused while tickets are outstanding"""
        self._check(self.L.shk_evidence_enable(self.h, int(bool(on))), "shk_evidence_enable")

    def evidence_last(self):
        """evidence of the batch whose result was handed out last: an (n, 3) uint32 array (cov, nk, len) copied from the context's
        pinned memory for a host batch (classify, wait); for a resident one (classify_device, wait_device) the DEVICE pointer of its
        n records, 12 bytes each -- read them back with hip_memcpy_dtoh.  Raises (SHK_ERR_STATE) when that batch was submitted
        with evidence off"""
        e = ShkEvidence()
        self._check(self.L.shk_evidence_last(self.h, C.byref(e)), "shk_evidence_last")
        n = int(e.n)
        if not self._last_on_host:
            return e.reads
        if n == 0:
            return np.zeros((0, 3), dtype=np.uint32)
        return np.ctypeslib.as_array(C.cast(e.reads, C.POINTER(C.c_uint32)), shape=(n, 3)).copy()

    # ---- candidates: per read its best m genes in the reference's ranking, with coverage and k-mer count --------
    def candidates_enable(self, m=4):
        """batches submitted from now on carry their reads' top m candidates (1 .. SHK_MAX_CANDIDATES; 0 switches the mode off) and
        run the full-probe kernels; refused while tickets are outstanding"""
        self._check(self.L.shk_candidates_enable(self.h, int(m)), "shk_candidates_enable")

    def candidates_last(self):
        """candidates of the batch whose result was handed out last: (reads, entries) -- an (n, 2) uint32 array (len, n_genes) and an
        (n, m, 3) uint32 array (gene, cov, nk; rank order, empty slots all 0) copied from the context's pinned memory for a host
        batch (classify, wait); for a resident one (classify_device, wait_device) (n, m, reads, entries) with the two DEVICE pointers
        (8 bytes per read, 12 bytes per entry) -- read them back with hip_memcpy_dtoh.  Raises (SHK_ERR_STATE) when that batch
        was submitted with candidates off"""
        c = ShkCandidates()
        self._check(self.L.shk_candidates_last(self.h, C.byref(c)), "shk_candidates_last")
        n, m = int(c.n), int(c.m)
        if not self._last_on_host:
            return n, m, c.reads, c.entries
        if n == 0:
            return np.zeros((0, 2), dtype=np.uint32), np.zeros((0, m, 3), dtype=np.uint32)
        reads = np.ctypeslib.as_array(C.cast(c.reads, C.POINTER(C.c_uint32)), shape=(n, 2)).copy()
        entries = np.ctypeslib.as_array(C.cast(c.entries, C.POINTER(C.c_uint32)), shape=(n, m, 3)).copy()
        return reads, entries

    # ---- placement: per association and mate the best diagonal of the gene's record (strand, pos, support) --------
    def placement_enable(self, on=True):
        """batches submitted from now on carry one placement per association (the classify kernels run unchanged, placement_kernel
        behind them); needs an index built with keep_positions; refused while tickets are outstanding"""
        self._check(self.L.shk_placement_enable(self.h, int(bool(on))), "shk_placement_enable")

    def placement_last(self):
        """placements of the batch whose result was handed out last: an (n_assoc, 2, 3) int64 array -- per association (parallel to
        gene_ids) and mate (strand, pos, support) -- copied from the context's pinned memory for a host batch (classify, wait); for a
        resident one (classify_device, wait_device) (n_assoc, DEVICE pointer) of 24-byte records {pos i32, support u32, strand u32} x 2
        -- placements_from_device reads them back.  Raises (SHK_ERR_STATE) when that batch was submitted with the mode off"""
        pl = ShkPlacements()
        self._check(self.L.shk_placement_last(self.h, C.byref(pl)), "shk_placement_last")
        n = int(pl.n_assoc)
        if not self._last_on_host:
            return n, pl.entries
        if n == 0:
            return np.zeros((0, 2, 3), dtype=np.int64)
        raw = np.ctypeslib.as_array(C.cast(pl.entries, C.POINTER(C.c_uint32)), shape=(n, 2, 3)).copy()
        return placements_from_raw(raw)

    # ---- segments: per association and mate the best m diagonals with their first and last voting slot --------
    def segments_enable(self, m=SHK_MAX_SEGMENTS):
        """batches submitted from now on carry, per association and mate, the m diagonals with the most votes (1 .. SHK_MAX_SEGMENTS;
        0 switches the mode off); needs an index built with keep_positions; refused while tickets are outstanding"""
        self._check(self.L.shk_segments_enable(self.h, int(m)), "shk_segments_enable")

    def segments_last(self):
        """segments of the batch whose result was handed out last: (n_keys, entries) -- an (n_assoc, 2) uint32 array and an
        (n_assoc, 2, m, 5) int64 array (strand, pos, support, first, last; rank order, empty slots all 0), both parallel to gene_ids
        -- copied from the context's pinned memory for a host batch (classify, wait); for a resident one (classify_device,
        wait_device) (n_assoc, m, n_keys, entries) with the two DEVICE pointers (8 bytes per association, 20 bytes per entry
        {pos i32, support, strand, first, last u32}) -- segments_from_device reads them back.  Raises (SHK_ERR_STATE) when that
        batch was submitted with the mode off"""
        sg = ShkSegments()
        self._check(self.L.shk_segments_last(self.h, C.byref(sg)), "shk_segments_last")
        n, m = int(sg.n_assoc), int(sg.m)
        if not self._last_on_host:
            return n, m, sg.n_keys, sg.entries
        if n == 0:
            return np.zeros((0, 2), dtype=np.uint32), np.zeros((0, 2, m, 5), dtype=np.int64)
        keys = np.ctypeslib.as_array(C.cast(sg.n_keys, C.POINTER(C.c_uint32)), shape=(n, 2)).copy()
        raw = np.ctypeslib.as_array(C.cast(sg.entries, C.POINTER(C.c_uint32)), shape=(n, 2, m, 5)).copy()
        return keys, segments_from_raw(raw)

    # ---- depth: per-base read depth along each gene, accumulated on the device over the batches counted since the last reset --------
    def depth_enable(self, min_support=1):
        """batches submitted from now on add their placed mates (support >= min_support) to the context's depth state; 0 switches
        the mode off and keeps the state; needs an index built with keep_positions; refused while tickets are outstanding"""
        self._check(self.L.shk_depth_enable(self.h, int(min_support)), "shk_depth_enable")

    def depth_layout(self):
        """gene_start[0 .. nidx] (uint64): the depth of gene g lies at [gene_start[g], gene_start[g + 1]) of depth_all()"""
        gs = getattr(self, "_depth_layout", None)          # (a property of the finalized index: fetched once)
        if gs is None:
            gs = np.zeros(int(self.index_info()["nidx"]) + 1, dtype=np.uint64)
            self._check(self.L.shk_depth_layout(self.h, _ptr(gs), len(gs) - 1), "shk_depth_layout")
            self._depth_layout = gs
        return gs.copy()

    def depth(self, gene):
        """the depth of one gene: uint32[len_g]"""
        gs = self.depth_layout()
        d = np.zeros(int(gs[gene + 1] - gs[gene]) if 0 <= gene < len(gs) - 1 else 0, dtype=np.uint32)     # (no such gene: the call says so)
        self._check(self.L.shk_depth_get(self.h, int(gene), _ptr(d), len(d)), "shk_depth_get")
        return d

    def depth_all(self, device_ptr=None):
        """the depth of every base, gene after gene (depth_layout): a uint32 array; with device_ptr (the address of a DEVICE buffer
        of at least gene_start[nidx] uint32) the copy stays on the device and the number of entries is returned"""
        total = int(self.depth_layout()[-1])
        if device_ptr is not None:
            self._check(self.L.shk_depth_get_all(self.h, C.c_void_p(device_ptr), total, 1), "shk_depth_get_all")
            return total
        d = np.zeros(total, dtype=np.uint32)
        self._check(self.L.shk_depth_get_all(self.h, _ptr(d), total, 0), "shk_depth_get_all")
        return d

    def depth_summary(self):
        """per gene (len, covered, max, pad, sum): a structured array of nidx records (GENE_DEPTH_DTYPE)"""
        out = np.zeros(int(self.index_info()["nidx"]), dtype=GENE_DEPTH_DTYPE)
        self._check(self.L.shk_depth_summary(self.h, _ptr(out), len(out)), "shk_depth_summary")
        return out

    def depth_mates(self):
        """mates counted since the last reset"""
        n = C.c_uint64()
        self._check(self.L.shk_depth_mates(self.h, C.byref(n)), "shk_depth_mates")
        return int(n.value)

    def depth_reset(self):
        self._check(self.L.shk_depth_reset(self.h), "shk_depth_reset")

    # ---- spliced depth and the junction table: segments mode's two consumers on the device --------
    def depth_enable_spliced(self, min_support=8):
        """as depth_enable, but a counted mate covers the union of its kept spans (kept_spans, span_union) instead of [pos, pos + L);
        the state and every depth read-out are shared with plain depth, one kind at a time (switching on a state that holds the other
        kind raises until depth_reset); 0 switches the mode off"""
        self._check(self.L.shk_depth_enable_spliced(self.h, int(min_support)), "shk_depth_enable_spliced")

    def junctions_enable(self, min_support=8, capacity=JUNCTIONS_DEFAULT_CAPACITY):
        """batches submitted from now on add their mates' junctions (junctions() at m = 4 and s_min = min_support) to a table on the
        device of `capacity` entries (rounded up to a power of two >= 64); 0 switches the mode off and keeps the table"""
        self._check(self.L.shk_junctions_enable(self.h, int(min_support), int(capacity)), "shk_junctions_enable")

    def junctions_get(self):
        """the table: a structured array (JUNCTION_DTYPE: gene, donor, acceptor, intron, mates) sorted by (gene, donor, acceptor)"""
        n = C.c_uint64()
        self._check(self.L.shk_junctions_get(self.h, None, 0, C.byref(n)), "shk_junctions_get")
        out = np.zeros(int(n.value), dtype=JUNCTION_DTYPE)
        if len(out):
            self._check(self.L.shk_junctions_get(self.h, _ptr(out), len(out), C.byref(n)), "shk_junctions_get")
        return out[:int(n.value)]

    def junctions_reset(self):
        self._check(self.L.shk_junctions_reset(self.h), "shk_junctions_reset")

    # ---- pileup: per record base the counted mates that show A, C, G or T there -- segments mode's third consumer on the device --------
    def pileup_enable(self, min_support=8):
        """batches submitted from now on add, per mate, the bases under its kept spans (kept_spans at s_min = min_support; a base owned
        by the earliest span that holds it) to the context's pileup state; 0 switches the mode off and keeps the state"""
        self._check(self.L.shk_pileup_enable(self.h, int(min_support)), "shk_pileup_enable")

    def pileup_enable_aligned(self, min_support=8):
        """as pileup_enable, but batches submitted from now on add every base of the alignment's final blocks (alignments mode's walk at
        s_min = min_support with the context's alignments_extend parameters) instead of the owned pieces; one state holds one kind;
        needs an index built with keep_bases; 0 switches pileup off"""
        self._check(self.L.shk_pileup_enable_aligned(self.h, int(min_support)), "shk_pileup_enable_aligned")

    def pileup(self, gene):
        """the counts of one gene: uint32 (len_g, 4), columns A, C, G, T on the record's strand"""
        gs = self.depth_layout()
        d = np.zeros((int(gs[gene + 1] - gs[gene]) if 0 <= gene < len(gs) - 1 else 0, 4), dtype=np.uint32)     # (no such gene: the call says so)
        self._check(self.L.shk_pileup_get(self.h, int(gene), _ptr(d), d.size), "shk_pileup_get")
        return d

    def pileup_all(self, device_ptr=None):
        """the counts of every base, gene after gene (depth_layout): uint32 (n_bases, 4); with device_ptr (the address of a DEVICE buffer
        of at least 4 * gene_start[nidx] uint32) the copy stays on the device and the number of entries is returned"""
        total = int(self.depth_layout()[-1])
        if device_ptr is not None:
            self._check(self.L.shk_pileup_get_all(self.h, C.c_void_p(device_ptr), 4 * total, 1), "shk_pileup_get_all")
            return 4 * total
        d = np.zeros((total, 4), dtype=np.uint32)
        self._check(self.L.shk_pileup_get_all(self.h, _ptr(d), d.size, 0), "shk_pileup_get_all")
        return d

    def pileup_mates(self):
        """mates that owned at least one record base since the last reset"""
        n = C.c_uint64()
        self._check(self.L.shk_pileup_mates(self.h, C.byref(n)), "shk_pileup_mates")
        return int(n.value)

    def pileup_reset(self):
        self._check(self.L.shk_pileup_reset(self.h), "shk_pileup_reset")

    def pileup_add(self, counts, mates, device_ptr=None):
        """adds an array in pileup_all()'s layout -- uint32 (n_bases, 4), or flat -- element by element to the state and `mates` to the
        mate counter (the caller vouches that no counter exceeds `mates`); with device_ptr (the address of a DEVICE buffer of
        4 * gene_start[nidx] uint32) `counts` is ignored and the buffer is added"""
        total = 4 * int(self.depth_layout()[-1])
        if device_ptr is not None:
            self._check(self.L.shk_pileup_add(self.h, C.c_void_p(device_ptr), total, int(mates), 1), "shk_pileup_add")
            return
        a = np.ascontiguousarray(counts, dtype=np.uint32)
        self._check(self.L.shk_pileup_add(self.h, _ptr(a), a.size, int(mates), 0), "shk_pileup_add")

    # ---- alignments: per association and mate the blocks of the mate on its gene's record -- segments mode's fourth consumer on the device --------
    def alignments_enable(self, min_support=8):
        """batches submitted from now on carry, per association and mate, the mate's gapped alignment to the gene's record (at most four
        blocks from its kept spans at s_min = min_support, with match and mismatch counts); 0 switches the mode off; needs an index
        built with keep_bases; refused while tickets are outstanding"""
        self._check(self.L.shk_alignments_enable(self.h, int(min_support)), "shk_alignments_enable")

    def alignments_extend(self, penalty=4, bonus=5):
        """end extension for the batches submitted from now on: a mate's outermost blocks grow over the clipped ends base by base, match
        +1, mismatch -penalty, +bonus for reaching the mate's end; penalty 0 switches it off (the default), 1 .. 15 on; bonus 0 .. 15"""
        self._check(self.L.shk_alignments_extend(self.h, int(penalty), int(bonus)), "shk_alignments_extend")

    def splice_sites_set(self, sites):
        """the site list of spliced ends (step 3b): an array of SPLICE_SITE_DTYPE records, or anything np.asarray turns into an (n, 3)
        array of (gene, donor, acceptor) -- the intron is record bases [donor, acceptor) of gene --, strictly ascending; replaces an
        earlier list; an empty one drops the list and switches the step off; refused while tickets are outstanding"""
        a = np.asarray(sites)
        if a.dtype != SPLICE_SITE_DTYPE:
            a = np.ascontiguousarray(np.asarray(a, dtype=np.int64).reshape(-1, 3))
            if a.size and (a.min() < 0 or a.max() > 0xFFFFFFFF):
                raise SharkHipError("shk_splice_sites_set: a site's fields are 32-bit unsigned numbers")
            a = a.astype("<u4")
        a = np.ascontiguousarray(a)
        n = a.shape[0]
        self._check(self.L.shk_splice_sites_set(self.h, _ptr(a) if n else None, n), "shk_splice_sites_set")

    def alignments_splice(self, min_overhang=3, max_cost=2, min_gap=2):
        """spliced ends for the batches submitted from now on: a clipped end of min_overhang .. 48 bases is tried across every listed
        junction it could have crossed and placed where the best costs at most max_cost not-a-matches and every other placement
        (staying on the block's diagonal included) at least min_gap more; min_overhang 0 switches the step off (the default); needs
        a site list"""
        self._check(self.L.shk_alignments_splice(self.h, int(min_overhang), int(max_cost), int(min_gap)), "shk_alignments_splice")

    def alignments_last(self):
        """alignments of the batch whose result was handed out last: an (n_assoc, 2) array of ALIGNMENT_DTYPE records, parallel to
        gene_ids, copied from the context's pinned memory for a host batch (classify, wait); for a resident one (classify_device,
        wait_device) (n_assoc, DEVICE pointer) of 64-byte records, two per association -- alignments_from_device reads them back.
        Raises (SHK_ERR_STATE) when that batch was submitted with the mode off"""
        al = ShkAlignments()
        self._check(self.L.shk_alignments_last(self.h, C.byref(al)), "shk_alignments_last")
        n = int(al.n_assoc)
        if not self._last_on_host:
            return n, al.entries
        if n == 0:
            return np.zeros((0, 2), dtype=ALIGNMENT_DTYPE)
        raw = np.ctypeslib.as_array(C.cast(al.entries, C.POINTER(C.c_uint32)), shape=(n, 2, 16)).copy()
        return alignments_from_raw(raw)

    # ---- indels: the insertions and deletions the mates' alignments show, tabled on the device over all batches --------
    def indels_enable(self, min_support=8, min_intron=SAM_DEFAULT_MIN_INTRON, capacity=INDELS_DEFAULT_CAPACITY):
        """batches submitted from now on add the gaps between their mates' final blocks (alignments mode's walk at s_min = min_support
        with the context's extension and splice parameters) to a table on the device of `capacity` entries (rounded up to a power of
        two >= 64): deletions shorter than min_intron and insertions of at most SHK_INDEL_MAX_INS bases, left-normalised; 0 switches
        the mode off and keeps the table; needs an index built with keep_bases"""
        self._check(self.L.shk_indels_enable(self.h, int(min_support), int(min_intron), int(capacity)), "shk_indels_enable")

    def indels_get(self, min_mates=0):
        """the table's keys with fwd + rev >= min_mates: a structured array (INDEL_DTYPE) sorted by (gene, x, kind, len, seq)"""
        n = C.c_uint64()
        self._check(self.L.shk_indels_get(self.h, int(min_mates), None, 0, C.byref(n)), "shk_indels_get")
        out = np.zeros(int(n.value), dtype=INDEL_DTYPE)
        if len(out):
            self._check(self.L.shk_indels_get(self.h, int(min_mates), _ptr(out), len(out), C.byref(n)), "shk_indels_get")
        return out[:int(n.value)]

    def indels_stats(self):
        """the seven counters since the last reset, as a dict keyed by INDEL_STAT_NAMES"""
        st = ShkIndelStats()
        self._check(self.L.shk_indels_stats(self.h, C.byref(st)), "shk_indels_stats")
        return {name: int(getattr(st, name)) for name in INDEL_STAT_NAMES}

    def indels_add(self, entries, stats=None):
        """adds another context's table (INDEL_DTYPE records, as indels_get hands them out) and, with `stats` (indels_stats' dict), its
        counters to this context's: how several workers' tables become one"""
        a = np.ascontiguousarray(entries, dtype=INDEL_DTYPE)
        st = None
        if stats is not None:
            st = ShkIndelStats(*[int(stats[name]) for name in INDEL_STAT_NAMES])
        self._check(self.L.shk_indels_add(self.h, _ptr(a) if len(a) else None, len(a), C.byref(st) if st is not None else None), "shk_indels_add")

    def indels_reset(self):
        self._check(self.L.shk_indels_reset(self.h), "shk_indels_reset")

    # ---- pairs: per association what its two mates' alignments say together, and the sample's fragment-size histogram --------
    def pairs_enable(self, min_intron=SAM_DEFAULT_MIN_INTRON, max_frag=FRAGMENTS_DEFAULT_MAX, n_bins=FRAGMENTS_DEFAULT_BINS):
        """batches submitted from now on (with alignments mode on) carry one PAIR_DTYPE record per association and are added to the
        fragments state (classes[6], hist[n_bins]); n_bins 0 switches the mode off and keeps the state; needs alignments mode on"""
        self._check(self.L.shk_pairs_enable(self.h, int(min_intron), int(max_frag), int(n_bins)), "shk_pairs_enable")

    def pairs_last(self):
        """pair records of the batch whose result was handed out last: (n_assoc,) records of PAIR_DTYPE, parallel to gene_ids, copied
        from the context's pinned memory for a host batch; for a resident one (n_assoc, DEVICE pointer) -- pairs_from_device reads them
        back.  Raises (SHK_ERR_STATE) when that batch was submitted without the mode"""
        pr = ShkPairs()
        self._check(self.L.shk_pairs_last(self.h, C.byref(pr)), "shk_pairs_last")
        n = int(pr.n_assoc)
        if not self._last_on_host:
            return n, pr.entries
        if n == 0:
            return np.zeros(0, dtype=PAIR_DTYPE)
        raw = np.ctypeslib.as_array(C.cast(pr.entries, C.POINTER(C.c_uint32)), shape=(n, 8)).copy()
        return raw.view(PAIR_DTYPE).reshape(-1)

    def fragments(self, n_bins=FRAGMENTS_DEFAULT_BINS):
        """the fragments state: (hist uint64 (n_bins,), classes uint64 (6,)); n_bins must be the state's"""
        hist = np.zeros(int(n_bins), dtype=np.uint64)
        classes = np.zeros(6, dtype=np.uint64)
        self._check(self.L.shk_fragments_get(self.h, _ptr(hist), int(n_bins), _ptr(classes)), "shk_fragments_get")
        return hist, classes

    def fragments_reset(self):
        self._check(self.L.shk_fragments_reset(self.h), "shk_fragments_reset")

    # ---- rescue: a mate without a block placed beside its placed partner ------------------------------------------------------
    def rescue_enable(self, min_intron=SAM_DEFAULT_MIN_INTRON, max_frag=FRAGMENTS_DEFAULT_MAX, max_cost=RESCUE_DEFAULT_MAX_COST,
                      min_gap=RESCUE_DEFAULT_MIN_GAP):
        """batches submitted from now on (with alignments mode on) carry one RESCUE_DTYPE record per association, and a rescued mate's
        alignment record holds its one block; max_frag 0 switches the mode off; needs alignments mode on"""
        self._check(self.L.shk_rescue_enable(self.h, int(min_intron), int(max_frag), int(max_cost), int(min_gap)), "shk_rescue_enable")

    def rescue_last(self):
        """rescue records of the batch whose result was handed out last: (n_assoc,) records of RESCUE_DTYPE, parallel to gene_ids, copied
        from the context's pinned memory for a host batch; for a resident one (n_assoc, DEVICE pointer) -- rescues_from_device reads them
        back.  Raises (SHK_ERR_STATE) when that batch was submitted without the mode"""
        rs = ShkRescues()
        self._check(self.L.shk_rescue_last(self.h, C.byref(rs)), "shk_rescue_last")
        n = int(rs.n_assoc)
        if not self._last_on_host:
            return n, rs.entries
        if n == 0:
            return np.zeros(0, dtype=RESCUE_DTYPE)
        raw = np.ctypeslib.as_array(C.cast(rs.entries, C.POINTER(C.c_uint32)), shape=(n, 4)).copy()
        return raw.view(RESCUE_DTYPE).reshape(-1)

    # ---- variants: the record positions where the pileup shows another base than the record (needs an index built with keep_bases) --------
    def variants(self, min_depth=8, min_alt=3, frac=(1, 5)):
        """the sites of the pileup state at these thresholds (include/shark_hip.h, "variants"): a structured array (VARIANT_DTYPE: gene,
        x, ref, alt, n[4]) sorted by (gene, x)"""
        prm = ShkVariantParams(int(min_depth), int(min_alt), int(frac[0]), int(frac[1]))
        n = C.c_uint64()
        self._check(self.L.shk_variants_get(self.h, C.byref(prm), None, 0, C.byref(n)), "shk_variants_get")
        out = np.zeros(int(n.value), dtype=VARIANT_DTYPE)
        if len(out):
            self._check(self.L.shk_variants_get(self.h, C.byref(prm), _ptr(out), len(out), C.byref(n)), "shk_variants_get")
        return out[:int(n.value)]

    def variants_summary(self, min_depth=8, min_alt=3, frac=(1, 5)):
        """per gene (observed, mismatches, covered, sites): a structured array of nidx records (GENE_VARIANTS_DTYPE)"""
        prm = ShkVariantParams(int(min_depth), int(min_alt), int(frac[0]), int(frac[1]))
        out = np.zeros(int(self.index_info()["nidx"]), dtype=GENE_VARIANTS_DTYPE)
        self._check(self.L.shk_variants_summary(self.h, C.byref(prm), _ptr(out), len(out)), "shk_variants_summary")
        return out

    def gene_counts(self, n=65536):
        a = np.zeros(n, dtype=np.uint64)
        self._check(self.L.shk_gene_counts(self.h, _ptr(a), n), "shk_gene_counts")
        return a

    def gene_counts_allreduce(self, others=(), n=65536):
        """sum the per-gene counters of this context and `others` (one per GPU) over RCCL"""
        ctxs = [self] + list(others)
        arr = (C.c_void_p * len(ctxs))(*[c.h for c in ctxs])
        a = np.zeros(n, dtype=np.uint64)
        self._check(self.L.shk_gene_counts_allreduce(arr, len(ctxs), _ptr(a), n), "shk_gene_counts_allreduce")
        return a

    def gene_counts_reset(self):
        self._check(self.L.shk_gene_counts_reset(self.h), "shk_gene_counts_reset")

    # ---- one process per GPU ------------------------------------------------------
    def dist_init(self, sdist):
        """join the RCCL communicator of a torch.distributed job (shark_amd.dist): rank 0's unique id is
        broadcast over the job's own channel.  A gloo job (CPU tests, single-GPU dry runs) has no RCCL
        communicator; dist_gene_counts_allreduce then reduces the local counters over gloo."""
        import torch
        import torch.distributed as td
        self._td = None
        if not (td.is_available() and td.is_initialized()) or td.get_world_size() == 1:
            return
        if td.get_backend() != "nccl":
            self._td = td
            return
        rank, world = td.get_rank(), td.get_world_size()
        buf = (C.c_uint8 * SHK_DIST_ID_BYTES)()
        if rank == 0:
            rc = self.L.shk_dist_unique_id(buf)
            if rc != 0:
                raise SharkHipError("shk_dist_unique_id: %s" % self.L.shk_strerror(rc).decode())
        t = torch.tensor(list(buf), dtype=torch.uint8, device="cuda")
        td.broadcast(t, 0)
        ident = (C.c_uint8 * SHK_DIST_ID_BYTES)(*t.cpu().tolist())
        self._check(self.L.shk_dist_init(self.h, ident, rank, world), "shk_dist_init")

    def dist_info(self):
        """(rank, world) as the communicator the collective runs over reports them: RCCL's own ncclCommUserRank /
        ncclCommCount for an RCCL job, torch.distributed's for a gloo dry run, (0, 1) without a job"""
        td = getattr(self, "_td", None)
        if td is not None:
            return td.get_rank(), td.get_world_size()
        r, w = C.c_int(), C.c_int()
        self._check(self.L.shk_dist_info(self.h, C.byref(r), C.byref(w)), "shk_dist_info")
        return r.value, w.value

    def dist_gene_counts_allreduce(self, n=65536):
        a = np.zeros(n, dtype=np.uint64)
        self._check(self.L.shk_dist_gene_counts_allreduce(self.h, _ptr(a), n), "shk_dist_gene_counts_allreduce")
        td = getattr(self, "_td", None)
        if td is not None:
            import torch
            t = torch.from_numpy(a.astype(np.int64))
            td.all_reduce(t)
            a = t.numpy().astype(np.uint64)
        return a

    def measure_random_lookups(self, table_bytes, n_lookups=1 << 31, nontemporal=False, both_halves=False):
        """G independent random 16-byte lookups per second in a table of table_bytes on this context's GPU (both_halves: each lookup
        also reads the other 64-byte half of its 128-byte line; the figure is lines per second either way)"""
        g = C.c_double()
        self._check(self.L.shk_measure_random_lookups(self.h, table_bytes, n_lookups, int(bool(nontemporal)) | (2 if both_halves else 0), C.byref(g)),
                    "shk_measure_random_lookups")
        return g.value

    @staticmethod
    def random_lookups_made(n_lookups):
        """how many lookups (lines) shk_measure_random_lookups(…, n_lookups, …) really makes in its timed launch: 2 048 workgroups x 256
        lanes x 5 per iteration, whole iterations"""
        per_iter = 2048 * 256 * 5
        return per_iter * max(1, min(n_lookups // per_iter, 1 << 20))

    def measure_valu_mix(self, waves_per_simd=4, iters=20000):
        """(ms, wave_iterations) of the exact-table kernel's instruction mix on register operands, `waves_per_simd` waves per SIMD"""
        ms, wi = C.c_double(), C.c_uint64()
        self._check(self.L.shk_measure_valu_mix(self.h, waves_per_simd, iters, C.byref(ms), C.byref(wi)), "shk_measure_valu_mix")
        return ms.value, wi.value

    def measure_valu_mix_clock(self, waves_per_simd=4, iters=20000):
        """(ms, wave_iterations, shader_ghz): measure_valu_mix and the clock the SIMDs held meanwhile (s_memtime over s_memrealtime)"""
        ms, wi, ghz = C.c_double(), C.c_uint64(), C.c_double()
        self._check(self.L.shk_measure_valu_mix_clock(self.h, waves_per_simd, iters, C.byref(ms), C.byref(wi), C.byref(ghz)), "shk_measure_valu_mix_clock")
        return ms.value, wi.value, ghz.value

    def timing_enable(self, on=True):
        self._check(self.L.shk_timing_enable(self.h, int(on)), "shk_timing_enable")

    def timing(self):
        t = ShkTiming()
        self._check(self.L.shk_timing_get(self.h, C.byref(t)), "shk_timing_get")
        return {f: getattr(t, f) for f, _ in ShkTiming._fields_}


def placements_from_raw(raw):
    """(n, 2, 3) uint32 words {pos, support, strand} of shk_placement -> (n, 2, 3) int64 (strand, pos, support)"""
    raw = np.asarray(raw, dtype=np.uint32).reshape(-1, 2, 3)
    out = np.empty(raw.shape, dtype=np.int64)
    out[:, :, 0] = raw[:, :, 2]
    out[:, :, 1] = raw[:, :, 0].view(np.int32)
    out[:, :, 2] = raw[:, :, 1]
    return out


def placements_from_device(n_assoc, ptr):
    """read the records of a resident batch back: (n_assoc, 2, 3) int64 (strand, pos, support)"""
    raw = np.zeros((n_assoc, 2, 3), dtype=np.uint32)
    if n_assoc:
        hip_memcpy_dtoh(raw, ptr, raw.nbytes)
    return placements_from_raw(raw)


def segments_from_raw(raw):
    """(n, 2, m, 5) uint32 words {pos, support, strand, first, last} of shk_segment -> int64 (strand, pos, support, first, last)"""
    raw = np.asarray(raw, dtype=np.uint32)
    out = np.empty(raw.shape, dtype=np.int64)
    out[..., 0] = raw[..., 2]
    out[..., 1] = raw[..., 0].view(np.int32)
    out[..., 2] = raw[..., 1]
    out[..., 3] = raw[..., 3]
    out[..., 4] = raw[..., 4]
    return out


def segments_from_device(n_assoc, m, keys_ptr, entries_ptr):
    """read the records of a resident batch back: ((n_assoc, 2) uint32, (n_assoc, 2, m, 5) int64) as segments_last gives them"""
    keys = np.zeros((n_assoc, 2), dtype=np.uint32)
    raw = np.zeros((n_assoc, 2, m, 5), dtype=np.uint32)
    if n_assoc:
        hip_memcpy_dtoh(keys, keys_ptr, keys.nbytes)
        hip_memcpy_dtoh(raw, entries_ptr, raw.nbytes)
    return keys, segments_from_raw(raw)


def alignments_from_raw(raw):
    """(n, 2, 16) uint32 words of shk_mate_alignment -> (n, 2) records of ALIGNMENT_DTYPE"""
    raw = np.ascontiguousarray(raw, dtype=np.uint32).reshape(-1, 2, 16)
    return raw.view(ALIGNMENT_DTYPE).reshape(-1, 2)


def alignments_from_device(n_assoc, ptr):
    """read the records of a resident batch back: (n_assoc, 2) records of ALIGNMENT_DTYPE as alignments_last gives them"""
    raw = np.zeros((n_assoc, 2, 16), dtype=np.uint32)
    if n_assoc:
        hip_memcpy_dtoh(raw, ptr, raw.nbytes)
    return alignments_from_raw(raw)


def pairs_from_device(n_assoc, ptr):
    """read the records of a resident batch back: (n_assoc,) records of PAIR_DTYPE as pairs_last gives them"""
    raw = np.zeros((n_assoc, 8), dtype=np.uint32)
    if n_assoc:
        hip_memcpy_dtoh(raw, ptr, raw.nbytes)
    return raw.view(PAIR_DTYPE).reshape(-1)


def rescues_from_device(n_assoc, ptr):
    """read the records of a resident batch back: (n_assoc,) records of RESCUE_DTYPE as rescue_last gives them"""
    raw = np.zeros((n_assoc, 4), dtype=np.uint32)
    if n_assoc:
        hip_memcpy_dtoh(raw, ptr, raw.nbytes)
    return raw.view(RESCUE_DTYPE).reshape(-1)


def cigar(rec, L, min_intron=SAM_DEFAULT_MIN_INTRON):
    """(CIGAR string, NM) of one ALIGNMENT_DTYPE record of a mate of L bytes: shk_alignment_cigar, the single definition of the text form
    (a host function: no context, no device).  Raises ValueError for a record that is inconsistent with L"""
    lib = load()
    one = np.zeros(1, dtype=ALIGNMENT_DTYPE)
    one[0] = rec
    buf = C.create_string_buffer(256)
    nm = C.c_uint32()
    rc = lib.shk_alignment_cigar(_ptr(one), int(L), int(min_intron), buf, len(buf), C.byref(nm))
    if rc != 0:
        raise ValueError("shk_alignment_cigar: %s" % lib.shk_strerror(rc).decode())
    return buf.value.decode(), int(nm.value)


def segment_span(seg, L, k):
    """the record span [lo, hi) of one segment (strand, pos, support, first, last) of a mate of L bytes (include/shark_hip.h)"""
    strand, pos, _, first, last = (int(v) for v in seg)
    if strand == 0:
        return pos + first, pos + last + k
    return pos + L - k - last, pos + L - first


def junctions(segments, L, k, s_min=8):
    """the junctions of ONE mate of L bytes from its reported segments (rows (strand, pos, support, first, last), rank order), as
    include/shark_hip.h defines them: [(donor, acceptor, intron, overlap)] in record order"""
    segs = [tuple(int(v) for v in sg) for sg in segments]
    segs = [sg for sg in segs if sg[2] >= 1]
    if not segs:
        return []
    strand0 = segs[0][0]
    kept = sorted((segment_span(sg, L, k) + (sg[1],) for sg in segs if sg[2] >= s_min and sg[0] == strand0), key=lambda t: (t[0], t[1]))
    out = []
    for (lo_a, hi_a, pos_a), (lo_b, hi_b, pos_b) in zip(kept, kept[1:]):
        if pos_b > pos_a:
            intron = pos_b - pos_a
            out.append((hi_a, lo_b, intron, hi_a + intron - lo_b))
    return out


def kept_spans(segments, L, k, s_min):
    """the kept spans of ONE mate of L bytes (include/shark_hip.h, "spliced depth and the junction table"): of its first
    SHK_MAX_SEGMENTS reported segments (rows (strand, pos, support, first, last), rank order) those with support >= s_min on
    rank 0's strand, as [(lo, hi, pos)] sorted by (lo, hi)"""
    segs = [tuple(int(v) for v in sg) for sg in segments][:SHK_MAX_SEGMENTS]
    segs = [sg for sg in segs if sg[2] >= 1]
    if not segs:
        return []
    strand0 = segs[0][0]
    return sorted((segment_span(sg, L, k) + (sg[1],) for sg in segs if sg[2] >= s_min and sg[0] == strand0), key=lambda t: (t[0], t[1]))


def span_union(spans, len_g):
    """the union of spans (rows whose first two fields are lo, hi) clipped to [0, len_g): disjoint [(lo, hi)] in ascending order,
    touching and overlapping spans merged -- the bases spliced depth counts for one mate"""
    out = []
    for lo, hi in sorted((max(int(sp[0]), 0), min(int(sp[1]), int(len_g))) for sp in spans):
        if hi <= lo:
            continue
        if out and lo <= out[-1][1]:
            out[-1] = (out[-1][0], max(out[-1][1], hi))
        else:
            out.append((lo, hi))
    return out


_hip = None


def hip_memcpy_dtoh(dst, src_ptr, nbytes):
    """copy nbytes from a device pointer into a numpy array (bench/test plumbing)"""
    global _hip
    if _hip is None:
        _hip = C.CDLL("libamdhip64.so")
        _hip.hipMemcpy.restype = C.c_int
        _hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    rc = _hip.hipMemcpy(dst.ctypes.data_as(C.c_void_p), C.c_void_p(src_ptr), nbytes, 2)  # hipMemcpyDeviceToHost
    if rc != 0:
        raise SharkHipError("hipMemcpy D2H failed: %d" % rc)
