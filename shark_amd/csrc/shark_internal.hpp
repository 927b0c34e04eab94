// shark_internal.hpp -- context layout and kernel launch entry points shared
// by the translation units of libsharkhip.  Not part of the public ABI.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <string>
#include <vector>

#include "../../include/shark_hip.h"
#include "lds_table.hpp"   // LTAB_*: the LDS-resident exact table of a tiny index
#include "kmer_table.hpp"  // KXTAB_*: the same for a one-gene index, keyed by the canonical k-mer itself
#include "indel_host.hpp"  // indel_key and the host-only parts of indels mode

namespace shk {

// ---- device-resident index (immutable after shk_ref_finalize) -------------
// HBM layout:
//   bf64     : the Bloom filter, sdsl::bit_vector layout (LSB-first 64-bit
//              words), zero-padded to a multiple of 512 bits.
//   rank_w   : uint32 ones-before-word directory, one entry per 64-bit word
//              (+1 sentinel = n_set): rank(pos) = rank_w[pos>>6] +
//              popcount(word & below(pos)) -- the probed word is all it needs.
//   ent      : one 8-byte entry per set bit r (r = rank): {start, len, first
//              gene} of its gene list; ids[start .. start+len) is the list.
//              (+1 sentinel {tot_idx,0,0}).  Explicit form of
//              _bv/_select_bv/_index_kmer (bloomfilter.h:142-167).
//   ids      : uint16 gene indices, ascending and unique inside a list.
//   sum32    : optional summary level: bit j = OR of filter bits
//              [j<<sum_shift, (j+1)<<sum_shift).  A clear summary bit proves
//              the filter bit clear, so the result of every probe is
//              unchanged; sized to stay in L2 (sparse filters) or in the
//              Infinity Cache.  Only for power-of-two filter sizes.
//   tab      : optional POSITION TABLE (power-of-two filter sizes): an exact
//              sparse encoding of the filter's set bits -- bit `pos` is set iff
//              `pos` is a key of the table -- with the list entry inline, so a
//              probe answers "is the bit set" AND "which list" with one
//              16-byte load instead of filter word + rank word + entry.
//              Buckets of two 8-byte slots, linear probing over buckets, home
//              bucket = pos & (n_buckets-1) (pos is already a hash).  Slot:
//                high word: [31:8] tag = pos >> tab_lg   [7] valid   [5:0] displacement (buckets from home)
//                low word : [31] multi   [30:0] gene (single-gene list) or rank r (multi: ent[r])
//              The filter itself stays in HBM as the ground truth (it defines
//              rank, is exported, and is what the tests compare bit for bit).
constexpr uint32_t LDS_SUM_LOG2 = 18;                 // 2^18 bits = 32 KiB of LDS per workgroup
constexpr uint32_t LDS_SUM_BITS = 1u << LDS_SUM_LOG2;

struct ListEntry {
  uint32_t start;
  uint16_t len;     // clipped at 0xFFFF: then the true end is the next entry's start
  uint16_t gene0;   // first gene of the list
};

struct DeviceIndex {
  uint64_t *bf64 = nullptr;
  uint64_t bf_bits = 0;
  uint64_t bf_words64 = 0;   // padded to whole 512-bit blocks
  bool pow2 = false;
  uint32_t *rank_w = nullptr;
  ListEntry *ent = nullptr;
  uint16_t *ids = nullptr;
  uint32_t *sum32 = nullptr;
  uint32_t sum_shift = 0;    // 0 = no summary level
  uint64_t sum_bits = 0;
  uint32_t *lsum32 = nullptr; // 2^18-bit summary staged into LDS by the table kernel (small indices only)
  uint32_t lsum_shift = 0;    // 0 = not used
  uint32_t *lbig32 = nullptr; // 2^20-bit summary (128 KiB of LDS, one 1024-thread workgroup per CU): classify_uni_kernel on
  uint32_t lbig_shift = 0;    //   indices too dense for the 2^18-bit one; 0 = not built
  double lbig_pass = 0.0;     //   the share of random k-mers that pass it
  uint32_t *ltab = nullptr;   // LDS-resident EXACT table of a tiny index (LTAB_BYTES image: T[2^15] then D[2^13]; lds_table.hpp)
  uint32_t ltab_mul = 0;      //   the multiplier its slots were computed with
  uint32_t ltab_gene = 0xFFFFFFFFu;   //   the ONE gene every key of that table answers with (a one-gene index), else 0xFFFFFFFF
  bool ltab_sparse = false;           //   the sparse first rounds are allowed on it (not SHK_NO_SPARSE=1 at build time)
  // the exact table of a ONE-gene index a second time, keyed by the canonical k-mer itself (kmer_table.hpp; k <= 17): its keys are every
  // canonical k-mer whose filter position is a set bit -- the gene's own and the ones that collide with them --, enumerated on the device
  // when the index is built (kmer_enum_kernel), so a probe needs no XXH64.  nullptr = not built (switched off, several genes, too many
  // keys, the builder gave up): the hashed table serves, results are the same
  uint8_t *kxtab = nullptr;           // LTAB_BYTES as allocated (the image is KXTAB_BYTES, the rest zero)
  uint64_t *kxkeys = nullptr;         // the keys, sorted (kx_nkeys of them)
  uint64_t kx_nkeys = 0;
  uint32_t kx_m1 = 0, kx_m2 = 0;      // the image's multipliers
  uint64_t kx_enum_us = 0, kx_build_us = 0;   // what the enumeration on the device and the construction on the host took
  uint64_t *tab = nullptr;   // 2 slots per bucket
  uint32_t tab_lg = 0;       // log2(number of buckets); 0 = no table
  bool tab_with_summary = false;
  uint64_t n_set = 0;
  uint64_t tot_idx = 0;
  uint64_t ent_len = 0, ids_len = 0;   // entries of `ent` / `ids` as allocated (padding and the per-position copies included)
  bool wrap = false;        // more than 65 536 genes: lists sorted by 16-bit id WITH duplicates (index_build.hip), WRAP kernels
  // ---- the reference itself, for the anchored extension of the table kernels (classify_uni.hpp) ----
  //   ref2   : all records back to back as 2-bit codes, base p in bits [2 (p & 15), +2) of dword p >> 4 (LSB first, invalid
  //            characters as 0), padded by four dwords
  //   refpay : per base position x the low word of the position-table slot of the k-mer STARTING at x (multi | payload; what a
  //            probe of that k-mer returns), REFPAY_NONE where no valid k-mer starts (record end, invalid character)
  //   atab   : the position table a second time with, in place of a slot's low word (its list), one occurrence of its key in the
  //            reference: x | strand << 31, strand = 1 when the k-mer at x is stored reverse-complemented (its canonical form is the
  //            reverse complement); 0xFFFFFFFF = unset.  Same buckets, same high words: the anchored extension's sample probes THIS
  //            table, and the bucket that says "the k-mer is in the index" says where in the reference in the same memory round trip
  //            (round 3 kept the occurrences in an array of their own, indexed by the slot that had matched: a dependent load)
  //   refext : per base position x where a valid k-mer starts: g | left << 16 | right << 24 -- the gene of x's record and how many
  //            positions directly in front of / behind x start a valid k-mer too (clipped at REFEXT_CLIP; such a run stays inside its
  //            record); REFEXT_NONE elsewhere.  refmul: one bit per position, 1 = the list under its k-mer is not a single-gene
  //            list.  What anchor_verdict_kernel reads instead of a payload per slot (anchor_verdict.hip)
  uint32_t *ref2 = nullptr, *refpay = nullptr, *refext = nullptr, *refmul = nullptr;
  uint64_t *atab = nullptr;
  uint32_t ref_total = 0;    // bases in ref2 / entries in refpay; 0 = not built
  // ---- the index a third time, keyed by the K-MER and bucketed by its MINIMISER (k = 15 ... 17, tables beyond the caches) ----
  //   ktab : 2^ktab_lg buckets of two 8-byte slots; eight consecutive buckets are one 128-byte LINE.  Keys: every canonical k-mer
  //          whose filter bit is set -- the reference's k-mers AND the filter's false positives, enumerated over all 4^k / 2
  //          canonical k-mers when the index is built --, so "is the key there" is exactly "is the bit set" (bloomfilter.h:87-89).
  //          line = hash of the k-mer's minimiser (the smallest hash among its k - w + 1 canonical w-mers), bucket within the
  //          line = the key's low three bits: consecutive k-mers of a read share their minimiser, hence their line -- one memory-side
  //          request serves several probes.  slot: low word as in `tab` (what a probe of the position returns), high word
  //          (key >> 3) << 1 | 1; a key that does not fit its bucket goes to the same bucket of the next line (so the bucket a slot
  //          sits in always names the key's low bits), marked as in `tab`.
  uint64_t *ktab = nullptr;
  uint32_t ktab_lg = 0;      // log2(buckets); 0 = not built
  uint32_t ktab_w = 0;       // w (the minimiser's length)
  uint64_t ktab_keys = 0;    // keys it holds (reference k-mers + false positives of the filter)
  // ---- placement mode (shk_ref_keep_positions; placement_build.hip): (gene, canonical k-mer) -> its one window in the gene's record ----
  //   ptab : one uint4 per DISTINCT (gene, canonical k-mer) of the reference, sorted by the 32-bit hash of the pair (pl_hash32), then
  //          by the smallest global position of the pair: {k-mer low, k-mer high, x | orientation << 31, gene}; x = the offset of the
  //          pair's only valid window in its record, orientation = 1 when that window's k-mer is its own canonical form;
  //          PTAB_AMBIGUOUS (placement_common.hpp) in place of x | orientation when the pair has two or more windows.  Windows that are their own reverse
  //          complement are left out.
  //   pdir : pdir[b] = the first entry whose hash >> (32 - ptab_lg) is >= b, for b = 0 .. 2^ptab_lg (one more entry = ptab_n)
  uint4 *ptab = nullptr;
  uint32_t *pdir = nullptr;
  uint32_t ptab_lg = 0;      // log2(buckets of pdir); 0 = not built
  uint64_t ptab_n = 0;       // entries
  // ---- depth mode (depth.hip): gene_start[g] = bases of the records numbered below g, g = 0 .. nidx (nidx + 1 entries); built
  //      with ptab for an index of at most 65 536 records (where the mode can be switched on), nullptr otherwise ----
  uint64_t *gene_start = nullptr;
  // ---- variants mode (shk_ref_keep_bases; variants.hip): recbase[gene_start[g] + x] = to_int[byte] - 1 of base x of gene g's record
  //      (0 .. 3, every other byte 4), in gene_start's order; recbase_bytes = gene_start[nidx] rounded up to a dword plus one dword, the padding 4:
  //      a lane may load an aligned dword behind the end.  nullptr / 0 = not built ----
  uint8_t *recbase = nullptr;
  uint64_t recbase_bytes = 0;
};
// Test-only read-back of the arrays above (tests/index_audit.py audits them entry by entry):
//   extern "C" int shk_debug_index_array(const shk_ctx *, const char *name, void *dst, uint64_t dst_bytes, uint64_t *bytes_needed)
// copies the named device array to the host exactly as allocated, padding included.  Names: rank_w, ent, ids, sum32, lsum32,
// lbig32, tab, atab, ltab, ref2, refpay, refext, refmul, recbase.  dst == NULL only reports the size; the size is 0 when this index does
// not carry the array.  "meta" gives SHK_DEBUG_META_WORDS uint64_t scalars in this order: tab_lg, sum_shift, lsum_shift,
// lbig_shift, ltab_mul, ref_total, n_set, tot_idx, pow2, wrap, ent_len, ids_len, bf_bits, bf_words64, sum_bits, ktab_lg.
// The k-mer keyed table: "kxmeta" = SHK_DEBUG_KXMETA_WORDS uint64_t scalars on every index, in this order: kx_in_use (1 = built: the
// one-gene exact-table kernels probe it), kx_m1, kx_m2, kx_keys, kx_enum_us, kx_build_us (a name of its own, as pmeta: `meta` keeps
// its 16 words); kxtab = its image (LTAB_BYTES as allocated), kxkeys = its sorted keys (uint64_t), both of size 0 when it is not built.
// The placement table (tests/placement_audit.py audits it): ptab = ptab_n + 1 entries of 16 bytes as allocated (the last one is
// spare and never written), pdir = 2^ptab_lg + 2 words, "pmeta" = SHK_DEBUG_PMETA_WORDS uint64_t scalars in this order: ptab_lg,
// ptab_n.  All three have size 0 on an index finalized without shk_ref_keep_positions.  (gene_start: shk_depth_layout.)
// The minimiser-bucketed table (tests/ktab_audit.py audits it): ktab = (16 << line_lg) + 16 uint64_t slots as allocated, line_lg =
// ktab_lg - 3, the eight spare buckets behind the last line included; size 0 when the table is not built.  "ktmeta" =
// SHK_DEBUG_KTMETA_WORDS uint64_t scalars on every index, in this order: ktab_lg, ktab_w, ktab_keys (all 0 without the table; a name
// of its own, as kxmeta and pmeta: `meta` keeps its 16 words).
// Exported from the library but deliberately not declared in include/shark_hip.h; no classify path uses it.
//
// Test-only runs of the two device primitives on caller-supplied data (debug_primitives.hip; tests/test_gpu_primitives.py compares
// them with the exact host models of tests/primitives_model.py).  Both work in any mode of the context, on its device and stream,
// allocate what they need and free it again:
//   extern "C" int shk_debug_scan_u32(shk_ctx *, const uint32_t *in, uint64_t n, uint32_t in_off, uint32_t out_off, int in_place,
//                                     uint32_t *out, uint32_t *in_after, uint64_t *total, uint32_t *guard_changed /* [6] */)
// runs exclusive_scan_u32 over the n host words `in` with a temp of exactly scan_temp_words(n) words.  in_off / out_off (0 .. 3)
// place the device copies of in / out that many words behind a 16-byte aligned address -- (0, 0) takes the vector kernels, anything
// else the item-by-item ones --; in_place != 0 means out == in (the offsets must be equal).  Hands back out[0 .. n), the 64-bit
// total read through the returned pointer, and in[0 .. n) as it stands afterwards.
//   extern "C" int shk_debug_sort_u64(shk_ctx *, const uint64_t *keys, uint64_t n, uint32_t end_bit, uint64_t *out, int *which,
//                                     uint32_t *guard_changed /* [8] */)
// runs radix_sort_u64 with `hist` of exactly radix_sort_hist_words(n) words and `scan_tmp` of exactly scan_temp_words(that) words.
// Hands back the n keys of the buffer the function returned and which one that was (0 = a, 1 = b).
// Guard bands: every device buffer handed down lies inside an allocation of its own between two bands of at least 64 words of a
// fixed pattern (out's payload, b, temp, hist and scan_tmp start as a second pattern).  guard_changed counts, per buffer, the guard
// words in front of it and behind it that lost the pattern: scan {in front, in back, out front, out back, temp front, temp back}
// (in place the out pair repeats the in pair), sort {a, b, hist, scan_tmp} x {front, back}.  All zero unless a kernel wrote outside
// its arrays.  n == 0 works and changes nothing but the scan's total.
// As shk_debug_index_array: exported, not declared in include/shark_hip.h, no classify or build path uses them.
// shk_debug_assemble_one (the same file, the same guard bands) runs exclusive_scan_assemble_one, the tail of a one-record index, over a
// caller's counts; it is declared and described in include/shark_hip.h (tests/test_gpu_one_gene_tail.py).
constexpr uint32_t SHK_DEBUG_META_WORDS = 16;
constexpr uint32_t SHK_DEBUG_KXMETA_WORDS = 6;
constexpr uint32_t SHK_DEBUG_PMETA_WORDS = 2;
constexpr uint32_t SHK_DEBUG_KTMETA_WORDS = 3;
constexpr uint32_t REFEXT_NONE = 0xFFFFFFFFu, REFEXT_CLIP = 254u;   // (an extent never reads 255: no entry looks like REFEXT_NONE)
constexpr uint32_t REFPAY_NONE = 0xFFFFFFFFu;   // (multi with payload 2^30-1: not a rank, n_set <= 2^30-1 entries have ranks below that)

// per-wave staging area of a read for a slot capacity S (layout: classify.hip)
__host__ __device__ constexpr uint32_t stage_cap_bases(uint32_t S) { return S + 96; }                  // S = slot capacity, multiple of 64
__host__ __device__ constexpr uint32_t code_dwords_for(uint32_t S) { return stage_cap_bases(S) / 16 + 2; }   // one stream (even)
__host__ __device__ constexpr uint32_t vbit_words_for(uint32_t S) { return stage_cap_bases(S) / 64 + 2; }
__host__ __device__ constexpr uint32_t stage_words_for(uint32_t S) { return code_dwords_for(S) + vbit_words_for(S); }   // 64-bit words: fw + rv + validity

// result / queue pointers of a classify launch.  They live in device memory behind ONE pointer so
// that the hot loop does not pin ~14 SGPRs for values it needs once per read (the fast kernel is at
// the 106-SGPR limit and spills wave-uniform values into VGPRs otherwise).
struct ClassifyOut {
  uint32_t *count;           // n : number of genes kept (exact)
  uint16_t *inl;             // n * SHK_INLINE_IDS : first genes
  uint32_t *counters;        // see CTR_*
  uint32_t *long_queue;      // read indices that did not fit the fast kernel
  uint32_t *tie_queue;       // 3 words per entry: read index, best cov, best nk
  shk_read_evidence *evid;   // n : {best cov, best nk, valid length} per read -- written by the evidence instantiations only (nullptr otherwise)
  // candidates mode (written by the candidates instantiations only; nullptr, nullptr, 0 otherwise)
  shk_read_candidates *cand_reads;   // n : {valid length, genes with a hit}
  shk_candidate *cand_entries;       // n * cand_m : read i's best cand_m genes in rank order, empty slots last
  uint32_t cand_m;                   // 1 .. SHK_MAX_CANDIDATES: how many of the kernel's SHK_MAX_CANDIDATES entries are stored
};

// ---- classify kernel parameters (passed by value) --------------------------
struct ClassifyParams {
  // index
  const uint64_t *bf64;
  const uint32_t *rank_w;
  const ListEntry *ent;
  const uint16_t *ids;
  const uint32_t *sum32;
  uint32_t sum_shift;
  const uint64_t *tab;
  uint32_t tab_lg;
  uint32_t tab_nt;           // 1 = table far larger than the caches: probe it with non-temporal loads
  // non power-of-two filter sizes: bits = mod_m << mod_shift; mod_fast = the 32-bit direct remainder applies
  uint32_t mod_fast, mod_shift, mod_m;
  uint64_t mod_c;
  const uint32_t *lsum32;    // LDS_SUM_BITS-bit summary (global copy), staged into LDS per workgroup
  uint32_t lsum_shift;
  uint32_t lx_gene;          // exact table in LDS (LSL = 21): the gene of a one-gene index (DeviceIndex::ltab_gene), else 0xFFFFFFFF
  uint32_t tro;              // 1 = the three-pairs kernel by offsets (classify_uni.hpp, TRO) is in the stream: uniform_check_kernel's verdict 3 for a batch of mixed lengths its layout holds
  uint32_t tri;              // 1 = the three-pairs-per-pass instantiation (classify_uni.hpp, TRI) is launched beside the ordinary uniform one: the one whose lengths qualify works
  uint32_t tile_first;       // (with tri, one-gene index) 1 = a round of disjoint k-mers for the three staged pairs together in front of the pairs' own rounds (classify_uni.hpp, TF)
  uint32_t lx_multi;         // exact table in LDS of an index of SEVERAL genes: the sparse first rounds with the early decision's argument (classify_uni.hpp)
  uint32_t kx;               // 1 = lsum32 is the one-gene index's table keyed by the canonical k-mer (kmer_table.hpp; classify_uni.hpp, KX): lsum_shift carries its m1,
  uint32_t kx_m2;            //   this its m2
  uint64_t bf_bits;
  uint64_t bf_mask;
  // options
  uint32_t k;
  uint32_t hasq;     // 0 = no masking (the reference's `char min_quality` is 0, FastqSplitter.hpp:52)
  int32_t mq;        // (signed char)(min_quality + 33), FastqSplitter.hpp:70 -- wraps for -q > 94 exactly as the reference's char does
  int32_t single;
  double c;
  // batch
  uint64_t n;
  const uint8_t *seq1;
  const uint64_t *off1;
  const uint8_t *seq2;
  const uint64_t *off2;
  const uint8_t *qual1;
  const uint8_t *qual2;
  // anchored extension (table modes): DeviceIndex::ref2 / refpay / atab; ref_total = 0: not available
  const uint32_t *ref2;
  const uint32_t *refpay;
  const uint64_t *atab;
  uint32_t ref_total;
  const uint32_t *refext;    // DeviceIndex::refext / refmul; nullptr: no anchor_verdict_kernel
  const uint32_t *refmul;
  uint32_t pre_verdict;      // 1 = anchor_verdict_kernel ran in front of this launch: a read whose count[] is set has its result
  uint32_t av_passes;        // anchor_verdict_kernel: consecutive passes a wave takes (set by its launcher from the batch's size)
  // the k-mer keyed, minimiser-bucketed table (DeviceIndex::ktab; classify_uni_kernel's PM_KTAB instantiations)
  const uint64_t *ktab;
  uint32_t ktab_lg, ktab_w;
  uint32_t ktab_nt;          // 1 = probe it with non-temporal loads
  // batches whose reads all have one length per mate (the usual sequencer output) take classify_uni_kernel's UNI instantiation,
  // the others its ragged one, which stages every read in the layout of the batch's LONGEST mates:
  // uni_flag == nullptr: the host knows (uni_L1, uni_L2) = the one length per mate, or the longest; else {1 = uniform and fits,
  // L1, L2 (the same)} written by uniform_check_kernel
  uint32_t uni_L1, uni_L2;
  const uint32_t *uni_flag;
  // ragged batches (the lengths above are then the LONGEST mates): per-launch table of read plans indexed by (l1, l2), 16 bytes each,
  // cleared by the host and filled by the kernel itself (classify_uni.hpp); nullptr / 0 = every read computes its plan
  uint4 *plan_tab;
  uint32_t plan_cap;               // entries
  // batches taken class by class (uni_flag[0] == 2; classify_uni_kernel's CLS instantiation): the pairs sorted by their two lengths,
  // 2 x uint4 per entry {o1, o2 | read index, "unguarded loads are safe", -, -}; cls_list: the non-empty classes in that order
  // {l1, l2, first entry, entries}; cls_share_first[s]: the class that entry s * ceil(n / CLS_SHARES) belongs to;
  // cls_hist: 2 x cls_cap words (pairs per class | the scatter's cursors)
  uint4 *cls_entries;
  uint4 *cls_list;
  uint32_t *cls_share_first;
  uint32_t *cls_hist;
  uint32_t cls_cap;                // classes the histogram holds: a batch with (L1 + 1) (L2 + 1) beyond that stays ragged
  uint32_t cls_min_fill;           // pairs per non-empty class the batch needs on average
  // per-read results and queues (device copy of ClassifyOut)
  const ClassifyOut *out;
  unsigned long long *gene_counts;  // 65536 (general kernel, EMIT mode)
  // work list for the general kernel (nullptr => all reads 0..n)
  const uint32_t *work;
  uint64_t n_work;
  const uint32_t *work_count;      // non-null: the number of work items is read from the device (tie queue) instead of n_work
  const uint32_t *flags;           // the launch's counters (CTR_OVERFLOW is honoured by the kernels that write gene_ids)
  // general-kernel scratch (per wave)
  uint64_t *scratch;
  uint64_t scratch_stride_words;   // per wave
  uint32_t scratch_slots;          // slot capacity per wave
  // emit mode (general kernel): write every gene whose (cov,nk) equals the
  // recorded best to gene_ids[gene_off[read] + i]
  const uint32_t *gene_off;
  uint16_t *gene_ids;
  // work counters (count_work build only)
  unsigned long long *work_counters;
  // timing-only ablation switches (env SHK_ABLATE; results are wrong when set; never set in tests/bench)
  uint32_t ablate;
  // 1 = a speculated launch (shark_hip.hip, enqueue_classify): uni_L1 / uni_L2 are the lengths the device found in the batch BEFORE this
  // one, and uniform_check_kernel looks at this batch's offsets beside the launch, not in front of it.  The uniform instantiations
  // return from their prologue unless the batch's first and last offsets are those of such a batch (classify_uni.hpp)
  uint32_t spec;
};

enum {
  CTR_LONG = 0,      // entries in long_queue
  CTR_TIE = 1,       // entries in tie_queue
  CTR_OVERFLOW = 2,  // 1 = the batch has more associations than gene_ids holds (finalize_total_kernel; scan_tile_offsets_one_kernel)
  CTR_UNUSED3 = 3,
  CTR_MAX_SLOTS = 4, // max k-mer slots over queued long reads
  CTR_UNUSED5 = 5,
  CTR_VOUCH_BAD = 5, // 1 = the caller of shk_classify_device_submit vouched for read lengths that the batch's offsets do not have (vouch_check_kernel)
  CTR_ASSOC_LO = 6,  // number of associations of the batch (the scan's total), 64 bits
  CTR_ASSOC_HI = 7,
  CTR_VERDICT = 8,   // (host copy only) 1 + uni_flag[0] of a batch the device looked at: 1 ragged, 2 uniform, 3 by classes; 0: the host knew
  CTR_UNI_L1 = 9,    // (host copy only) uni_flag[1], uni_flag[2] of such a batch: the one length per mate, or the longest mates; 0: the host knew
  CTR_UNI_L2 = 10,
  CTR_SPEC_MISS = 11, // 1 = a speculated batch whose offsets are not what the launch assumed (scan_tile_offsets_one_kernel): nothing was counted, the host runs it again
  CTR_WORDS = 12
};

constexpr uint32_t UNI_FLAG_WORDS = 16;
constexpr uint32_t COUNTER_BLOCK_WORDS = 16;   // CTR_WORDS rounded up: Slot::d_uni_flag = d_counters + this
static_assert(CTR_WORDS <= COUNTER_BLOCK_WORDS, "the counters and the uniformity words share one allocation");
constexpr uint32_t CLS_SHARES = 65536;    // equal shares of a sorted batch: sixteen per wave of the exact-table kernels' grid, taken in turns (classify_uni.hpp, DYN)
constexpr uint32_t CLS_MIN_FILL = 16;     // by classes only if a non-empty class holds that many pairs on average

// ---- one batch in flight ---------------------------------------------------------------------
constexpr int PIPE_DEPTH = 3;      // batches shk_classify_submit keeps in flight per context

struct Ctx;
int set_hip_error(Ctx *ctx, hipError_t e, const char *what);

// ---- a buffer that owns its memory: device (hipMalloc) or pinned host (hipHostMalloc); cap counts entries.  Movable, not
// copyable, freed by its destructor: a Slot frees what it owns, `s = Slot{}` included, and so does a Ctx (delete ctx) ----
template <typename T, bool PINNED>
struct Array {
  T *p = nullptr;
  size_t cap = 0;
  Array() = default;
  Array(const Array &) = delete;
  Array &operator=(const Array &) = delete;
  Array(Array &&o) noexcept : p(o.p), cap(o.cap) { o.p = nullptr; o.cap = 0; }
  Array &operator=(Array &&o) noexcept
  {
    if (this != &o) { release(); p = o.p; cap = o.cap; o.p = nullptr; o.cap = 0; }
    return *this;
  }
  ~Array() { release(); }
  hipError_t release()
  {
    const hipError_t e = !p ? hipSuccess : PINNED ? hipHostFree(p) : hipFree(p);
    p = nullptr;
    cap = 0;
    return e;
  }
  // exactly n entries, newly allocated (what it held is gone): the context's states, which are sized by the index or by their caller
  int alloc_exact(Ctx *ctx, size_t n)
  {
    hipError_t e = release();
    if (e != hipSuccess && !PINNED) return set_hip_error(ctx, e, "hipFree");
    e = PINNED ? hipHostMalloc((void **)&p, n * sizeof(T), hipHostMallocDefault) : hipMalloc((void **)&p, n * sizeof(T));
    if (e != hipSuccess) return set_hip_error(ctx, e, PINNED ? "hipHostMalloc" : "hipMalloc");
    cap = n;
    return SHK_OK;
  }
  // at least `need` entries (a quarter more and 64 where it has to grow; what it held is gone then): the buffers that follow the batches
  int reserve(Ctx *ctx, size_t need)
  {
    if (need <= cap && p) return SHK_OK;
    return alloc_exact(ctx, need + need / 4 + 64);
  }
};
template <typename T> using DevArray = Array<T, false>;
template <typename T> using PinArray = Array<T, true>;

// one kind of per-batch record: the device array the kernels write and the pinned mirror a host batch's records are published into
// (launch_publish_records); a batch hands out the one its caller can read
template <typename T>
struct Mirrored {
  DevArray<T> d;
  PinArray<T> h;
  const T *handed(bool host_batch) const { return host_batch ? h.p : d.p; }
};

// associations that segment arrays (two headers and 2 x m entries each) hold at m entries per mate
template <bool PINNED>
uint64_t segments_cap(const Array<uint32_t, PINNED> &keys, const Array<shk_segment, PINNED> &entries, uint32_t m)
{
  if (!m) return 0;
  const uint64_t by_keys = keys.cap / 2, by_entries = entries.cap / (2ull * m);
  return by_keys < by_entries ? by_keys : by_entries;
}

struct Slot {
  // device copies of a host batch (host-buffer entry points only)
  DevArray<uint8_t> d_seq1, d_seq2, d_qual1, d_qual2;
  DevArray<uint64_t> d_off1, d_off2;
  // device results
  DevArray<uint32_t> d_count;
  DevArray<uint16_t> d_inl;
  DevArray<uint32_t> d_gene_off;
  DevArray<uint16_t> d_gene_ids;
  Mirrored<shk_read_evidence> rec_evid;                // evidence mode: one record per read (allocated with the first such batch)
  Mirrored<shk_read_candidates> rec_cand_reads;        // candidates mode: one header per read and cand_m entries
  Mirrored<shk_candidate> rec_cand_entries;            //  (allocated with the first such batch)
  DevArray<uint32_t> d_long_queue, d_tie_queue;
  uint32_t *d_counters = nullptr;
  uint32_t *d_uni_flag = nullptr;  // UNI_FLAG_WORDS words: verdict of uniform_check_kernel / class_plan_kernel (0 ragged, 1 uniform, 2 by classes), lengths, scratch
  DevArray<uint4> d_plan;          // read plans of a ragged batch (ClassifyParams::plan_tab)
  // a batch taken class by class (ClassifyParams::cls_*)
  DevArray<uint4> d_cls_entries, d_cls_list;
  uint32_t *d_cls_share = nullptr;
  DevArray<uint32_t> d_cls_hist;
  DevArray<uint64_t> d_scan_temp;
  ClassifyOut *d_out = nullptr;
  ClassifyOut out_shadow{};        // what *d_out holds (rewritten only when a buffer moved)
  // pinned host: counters, result offsets and ids
  uint32_t *h_counters = nullptr;  // CTR_WORDS
  PinArray<uint32_t> h_gene_off;
  PinArray<uint16_t> h_gene_ids;
  hipEvent_t ev_h2d = nullptr, ev_done = nullptr, ev_d2h = nullptr;
  // the batch
  uint64_t ticket = 0;             // 0 = free
  bool waited = true;              // its results were handed out (the slot may be reused by a later submit)
  uint64_t n = 0;
  ClassifyParams p{};              // launch parameters (kept for the slow paths)
  uint32_t fast_cap = 0, gen_slots = 0;
  bool host_batch = false;
  bool speculated = false;         // the uniform launch was made with the lengths of the batch before, the check beside it (enqueue_classify)
  bool evidence = false;           // submitted in evidence mode: the evidence instantiations ran and rec_evid holds its records
  uint32_t cand_m = 0;             // submitted in candidates mode with this many entries per read (0: not): the candidates instantiations ran
  bool long_speculative = false;   // (device-resident submit) the caller's length bound was taken on trust: checked in wait
  // placement mode: one record per association, as many as d_gene_ids holds (allocated with the first such batch)
  bool placement = false;          // submitted in placement mode: placement_kernel ran behind the assembly and rec_place holds its records
  Mirrored<shk_placement> rec_place;
  // depth mode: submitted with this min_support (0: not): placement_kernel ran (rec_place.d holds its records) and depth_accumulate_kernel behind it
  uint32_t depth = 0;
  // segments mode: submitted with this many entries per mate (0: not): segments_kernel ran behind the assembly; per association two headers
  // (rec_seg_keys) and 2 x seg_m entries (rec_seg_entries), allocated with the first such batch for as many associations as d_gene_ids holds
  uint32_t seg_m = 0;
  Mirrored<uint32_t> rec_seg_keys;
  Mirrored<shk_segment> rec_seg_entries;
  // spliced depth and the junction table (spliced.hip): submitted with these floors (0: not).  They read segments_kernel's records at
  // m = SHK_MAX_SEGMENTS: segments mode's own when it runs at that m, else arrays of their own (allocated with the first such batch,
  // never handed out) that a second launch of segments_kernel fills
  uint32_t sp_depth = 0, sp_junc = 0;
  DevArray<uint32_t> d_sp_keys;
  DevArray<shk_segment> d_sp_entries;
  // pileup mode (pileup.hip): submitted with this floor (0: not).  The third reader of those records at m = SHK_MAX_SEGMENTS, from the same
  // arrays: segments mode's own at that m, else d_sp_*, which are filled when ANY of spliced depth, the junction table and pileup is on
  uint32_t pileup = 0;
  // alignments mode (align.hip): submitted with this floor (0: not).  The fourth reader of those records, and the one whose result is per
  // association: two 64-byte records each (rec_align, allocated with the first such batch for as many associations as d_gene_ids holds;
  // its capacities count mates' records)
  uint32_t align = 0;
  Mirrored<shk_mate_alignment> rec_align;
  // end extension (shk_alignments_extend) as submitted: mismatch penalty (0: off) and end bonus; aligned pileup (shk_pileup_enable_aligned):
  // submitted with this floor (0: not) -- align_kernel's accumulating instantiation adds the batch to Ctx::pileup, pileup_kernel does not run
  uint32_t ext_p = 0, ext_b = 0;
  uint32_t pileup_al = 0;
  // spliced ends (shk_alignments_splice) as submitted: min_overhang (0: off), max_cost, min_gap; the site list is the context's
  uint32_t spl_h = 0, spl_cost = 0, spl_gap = 0;
  // pairs mode (pairs.hip): submitted with this n_bins (0: not; only with `align`): pair_kernel ran behind the storing align_kernel, one
  // 32-byte record per association (rec_pairs, allocated with the first such batch for as many associations as d_gene_ids holds);
  // pairs_count: the batch is added to Ctx::frag (not a shk_count_work batch)
  uint32_t pairs = 0, pairs_min_intron = 0, pairs_max_frag = 0;
  bool pairs_count = false;
  Mirrored<shk_pair> rec_pairs;
  // rescue mode (rescue.hip): submitted with this max_frag (0: not; only with `align`): rescue_scan_kernel and rescue_kernel ran behind the
  // storing align_kernel and in front of pair_kernel, one 16-byte record per association (rec_rescue) and a queue of the attempted
  // associations (d_rescue_queue: 16 bytes that hold the count, then (read, association) pairs), both allocated with the first such batch
  uint32_t rescue = 0, rescue_min_intron = 0, rescue_max_cost = 0, rescue_min_gap = 0;
  Mirrored<shk_rescue> rec_rescue;
  DevArray<uint2> d_rescue_queue;
  // indels mode (indels.hip): submitted with this floor (0: not) and min_intron.  It reads align_kernel's records at that floor: alignments
  // mode's own where it runs at the same floor, else an array of its own (allocated with the first such batch, never handed out) that the
  // storing align_kernel fills once more
  uint32_t indels = 0, indels_min_intron = 0;
  DevArray<shk_mate_alignment> d_indel_align;
};


// SpliceSites::d: the word at which the site arrays start behind the n_genes + 1 offsets (even: the pairs are 8-byte aligned)
__host__ __device__ inline uint32_t splice_sites_word(uint32_t n_genes) { return (n_genes + 2u) & ~1u; }

// one entry of the junction table (spliced.hip): key = (gene_start[g] + donor) << 32 | (gene_start[g] + acceptor)
struct JunctionEntry {
  unsigned long long key;   // JUNCTION_EMPTY: free
  uint32_t mates;           // observations since the last reset
  uint32_t intron;          // the smallest seen (all ones in a free entry)
};
static_assert(sizeof(JunctionEntry) == 16, "16-byte entries");
constexpr unsigned long long JUNCTION_EMPTY = ~0ull;   // (no key: its acceptor half would be base 2^32 - 1 of a reference of fewer than 2^32 bases)

// ---- the context's accumulated states: what the batches' tails add to and the read-outs read.  Each owns its device memory, sized exactly
// (Array::alloc_exact) by the enable that finds it missing, and outlives its mode's being switched off; all of one state's arrays are
// allocated or none is ----
// uint32 counters along the reference with the mates counted into them: the depth state and the pileup state
struct CounterState {
  uint32_t floor = 0;                          // min_support for the batches submitted from now on (0: off)
  bool kind = false;                           // the kind `floor` stands for, one per state: depth plain intervals (false) or the unions of kept spans (true, shk_depth_enable_spliced);
                                               //  pileup owned pieces (false, pileup.hip) or the alignment's final blocks (true, align.hip)
  bool dirty = false;                          // a batch of either kind was submitted since the first enable / the last reset
  // depth: gene_start[nidx] + 1 entries: +1 at a counted mate's first base, -1 behind its last
  // pileup: gene_start[nidx] x 4 counters, [x * 4 + b]: the observations of base b at x
  DevArray<uint32_t> counts;
  DevArray<unsigned long long> mates;          // counted mates since the last reset (not null: the mode was enabled once)
};
// depth mode (shk_depth_enable; depth.hip): its counters are a difference array, so its read-outs go through a scan
struct DepthState : CounterState {
  DevArray<uint32_t> scan;                     // read-out: exclusive scan of `counts` over all its entries; depth of base x at [1 + x] (allocated by the first read-out)
  DevArray<uint64_t> scan_temp;
  bool scan_current = false;                   // `scan` holds the scan of the state as it stands (cleared by every launch that adds to it and by reset)
  DevArray<shk_gene_depth> summary;            // nidx records (allocated by the first shk_depth_summary)
};
// junction table (shk_junctions_enable; spliced.hip)
struct JunctionState {
  uint32_t floor = 0;                          // min_support for the batches submitted from now on (0: off)
  bool dirty = false;                          // a junction batch was submitted since the first enable / the last reset
  DevArray<JunctionEntry> tab;                 // tab.cap entries, a power of two >= 64 (null: never enabled)
  DevArray<unsigned long long> dropped;        // observations that found the table full since the last reset (allocated in front of the first table, kept across a new capacity)
};
// one entry of the indel table (indels.hip): key = (gene_start[g] + x) << 32 | kind << 31 | the event (indel_key, indel_host.hpp)
struct IndelEntry {
  unsigned long long key;   // INDEL_EMPTY: free
  uint32_t fwd, rev;        // observations since the last reset from mates whose record has strand 0 / 1
};
static_assert(sizeof(IndelEntry) == 16, "16-byte entries");
constexpr unsigned long long INDEL_EMPTY = ~0ull;   // (no key: its position would be base 2^32 - 1 of a reference of fewer than 2^32 - 1 bases)
constexpr uint32_t INDEL_STATS = 7;                  // shk_indel_stats' counters, in its order
// indels mode's parameters and the indel table (shk_indels_enable; indels.hip)
struct IndelState {
  uint32_t floor = 0;                          // min_support for the batches submitted from now on (0: off)
  uint32_t min_intron = 0;                     // the table's (set by the enable that found it clean)
  bool dirty = false;                          // an indels batch was submitted or entries were added since the first enable / the last reset
  DevArray<IndelEntry> tab;                    // tab.cap entries, a power of two >= 64 (null: never enabled)
  DevArray<unsigned long long> stats;          // INDEL_STATS counters since the last reset (allocated in front of the first table, kept across a new capacity)
};
// pairs mode's parameters and the fragments state (shk_pairs_enable; pairs.hip)
struct FragmentState {
  uint32_t n_bins = 0;                         // n_bins for the batches submitted from now on (0: off)
  uint32_t min_intron = 0, max_frag = 0;
  bool dirty = false;                          // a pairs batch was submitted since the first enable / the last reset
  DevArray<unsigned long long> hist;           // hist[bins()], classes[6] (null: never enabled)
  uint32_t bins() const { return hist.p ? (uint32_t)(hist.cap - 6) : 0u; }   // the state's n_bins
};
// variants mode's scratch (shk_variants_get / _summary; variants.hip): read-outs of the pileup state; it only grows
struct VariantScratch {
  DevArray<uint32_t> waves;                    // sites per wavefront of 256 positions, then their exclusive scan
  DevArray<uint64_t> temp;                     // exclusive_scan_u32's temp over `waves` (allocated with it)
  DevArray<shk_variant> out;                   // records
  DevArray<shk_gene_variants> summary;         // nidx records
};
// spliced ends (shk_splice_sites_set, shk_alignments_splice): the list as it was given (sorted by (gene, donor, acceptor)), on the device a
// per-gene offset array and the sites as {donor, acceptor} in that order and as {acceptor, donor} in (acceptor, donor) order per gene
struct SpliceSites {
  std::vector<shk_splice_site> sites;
  DevArray<uint32_t> d;                        // one allocation: n_genes + 1 offsets, then from word splice_sites_word(n_genes) on the two site arrays
  uint32_t h = 0, cost = 0, gap = 0;           // shk_alignments_splice: min_overhang (0: off), max_cost, min_gap for the batches submitted from now on
};

// index_build.hip
int build_index(Ctx *ctx);
// placement_build.hip: DeviceIndex::ptab / pdir from the uploaded reference (called by build_index while its buffers live; keys_a, keys_b:
// `total` words each, free for use)
int build_placement_table(Ctx *ctx, const uint8_t *d_bytes, uint64_t total, const uint64_t *d_rec_off, uint32_t n_rec, const uint32_t *d_rec_nidx,
                          uint64_t *keys_a, uint64_t *keys_b);
// placement.hip: per association of the batch in `s` the best diagonal per mate, behind the kernels that wrote gene_off / gene_ids
int launch_placement(Ctx *ctx, const Slot &s, hipStream_t stream);
// segments.hip: per association of the batch in `s` and per mate its best s.seg_m diagonals with their first and last voting slot
int launch_segments(Ctx *ctx, const Slot &s, hipStream_t stream);
// the same kernel at m entries per mate into other arrays (cap_assoc: associations they hold): what spliced.hip reads when segments mode is off or narrower
int launch_segments_into(Ctx *ctx, const Slot &s, uint32_t m, uint32_t *d_keys, shk_segment *d_entries, uint64_t cap_assoc, hipStream_t stream);
// depth.hip: the batch in `s` (its placements in s.rec_place.d) into the context's difference array, behind launch_placement; skip_if_long: as launch_gene_hist
int launch_depth_accumulate(Ctx *ctx, const Slot &s, bool skip_if_long, hipStream_t stream);
// spliced.hip: the batch in `s` from its segments at m = SHK_MAX_SEGMENTS (`entries`, cap_assoc associations) into the depth state (s.sp_depth)
// and / or the junction table (s.sp_junc), behind segments_kernel; skip_if_long: as launch_gene_hist
int launch_spliced_accumulate(Ctx *ctx, const Slot &s, const shk_segment *entries, uint64_t cap_assoc, bool skip_if_long, hipStream_t stream);
// pileup.hip: the batch in `s` from the same records into Ctx::pileup at floor s.pileup, behind segments_kernel; skip_if_long: as launch_gene_hist
int launch_pileup(Ctx *ctx, const Slot &s, const shk_segment *entries, uint64_t cap_assoc, bool skip_if_long, hipStream_t stream);
// align.hip: per association of the batch in `s` and per mate its blocks on the gene's record with their match and mismatch counts, from the
// same records and DeviceIndex::recbase into s.rec_align.d at floor s.align, behind segments_kernel; skip_if_long: as launch_gene_hist
// store: the records go to s.rec_align.d at floor s.align; accumulate: the final blocks' bases go to Ctx::pileup at floor s.pileup_al (one launch
// does both where the floors are equal).  With s.ext_p == 0 and no accumulation the kernel launched is the one this mode always launched
int launch_alignments(Ctx *ctx, const Slot &s, const shk_segment *entries, uint64_t cap_assoc, bool skip_if_long, bool store, bool accumulate, hipStream_t stream);
// pairs.hip: per association of the batch in `s` its pair record from the two mates' records in s.rec_align.d (cap_assoc: launch_alignments') into
// s.rec_pairs.d and, where s.pairs_count, the batch into Ctx::frag; directly behind the storing launch_alignments; skip_if_long: as launch_gene_hist
int launch_pairs(Ctx *ctx, const Slot &s, uint64_t cap_assoc, bool skip_if_long, hipStream_t stream);
// rescue.hip: per association of the batch in `s` its rescue record into s.rec_rescue.d and, where a mate is rescued, that mate's record in
// s.rec_align.d; directly behind the storing launch_alignments and in front of launch_pairs (cap_assoc, skip_if_long: launch_pairs')
int launch_rescue(Ctx *ctx, const Slot &s, uint64_t cap_assoc, bool skip_if_long, hipStream_t stream);
// variants.hip: pileup.counts[i] += d_add[i] over n_entries counters (d_add 16-byte aligned: SHK_ERR_ARG otherwise), *pileup.mates += mates, on ctx->stream
int launch_pileup_add(Ctx *ctx, const uint32_t *d_add, uint64_t n_entries, uint64_t mates);
// variants.hip: the sites of the pileup state against DeviceIndex::recbase: their number into *n_sites (host; the stream is drained) and, with
// out != nullptr, the records in (gene, x) order into out[0 .. *n_sites) (host; SHK_ERR_ARG if cap is smaller, *n_sites set all the same)
int variants_call(Ctx *ctx, const shk_variant_params &prm, shk_variant *out, uint64_t cap, uint64_t *n_sites);
// variants.hip: per gene {observed, mismatches, covered, sites} into Ctx::var.summary (nidx records), on ctx->stream
int launch_variants_summary(Ctx *ctx, const shk_variant_params &prm);
// align.hip: the storing launch at floor s_min into `out` (out_cap mates' records) instead of s.rec_align.d: what indels mode reads when
// alignments mode is off or at another floor; extension and spliced ends as submitted
int launch_alignments_into(Ctx *ctx, const Slot &s, const shk_segment *entries, uint64_t cap_assoc, bool skip_if_long, uint32_t s_min, shk_mate_alignment *out,
                           uint64_t out_cap, hipStream_t stream);
// indels.hip: the gaps between the blocks of the batch's records in `records` (cap_assoc associations; align_kernel's at floor s.indels) into
// Ctx::indel, directly behind the align_kernel that stored them; skip_if_long: as launch_gene_hist
int launch_indels(Ctx *ctx, const Slot &s, const shk_mate_alignment *records, uint64_t cap_assoc, bool skip_if_long, hipStream_t stream);
int launch_indel_clear(Ctx *ctx);      // every entry of Ctx::indel.tab empty, its counters 0, on ctx->stream
// indels.hip: n validated entries {key, fwd, rev} (device memory) into the table and, with d_stats, INDEL_STATS counters onto its counters, on ctx->stream
int launch_indel_add(Ctx *ctx, const IndelEntry *d_in, uint64_t n, const unsigned long long *d_stats);
int launch_junction_clear(Ctx *ctx);   // every entry of Ctx::junc.tab empty, its `dropped` 0, on ctx->stream
// the read-out: Ctx::depth.scan[1 + x] = depth of base x of the full array (inclusive prefix sum of the difference array), on ctx->stream
int depth_scan(Ctx *ctx);
// per gene {len, covered, max, sum} of the scanned array into Ctx::depth.summary (nidx records), on ctx->stream behind depth_scan
int launch_depth_summary(Ctx *ctx);

// classify.hip
int launch_classify_fast(Ctx *ctx, const ClassifyParams &p, uint32_t max_slots, hipStream_t stream, bool evidence = false, bool candidates = false);   // candidates: serves evidence too
const char *probe_mode_name(const Ctx *ctx);
int launch_classify_general(Ctx *ctx, const ClassifyParams &p, bool emit, unsigned n_waves, hipStream_t stream, bool evidence = false, bool candidates = false);   // evidence, candidates: the non-EMIT pass only
int launch_gather_inline(const uint32_t *count, const uint16_t *inl, const uint32_t *gene_off, uint16_t *gene_ids, uint64_t n,
                         const uint32_t *counters, hipStream_t stream);
int launch_finalize_total(const uint64_t *total, uint32_t *counters, uint64_t gene_ids_cap, hipStream_t stream);
int launch_gene_hist(const uint16_t *gene_ids, const uint32_t *counters, bool skip_if_long, unsigned long long *gene_counts, uint64_t n_reads, uint64_t n_genes,
                     hipStream_t stream);
int launch_fill_offsets(uint64_t *off, uint64_t n_plus_1, uint64_t stride, hipStream_t stream);
int launch_vouch_check(const ClassifyParams &p, uint32_t L1, uint32_t L2, uint32_t *counters, hipStream_t stream);
int launch_publish_results(const uint32_t *counters, uint32_t *h_counters, const uint32_t *gene_off, uint32_t *h_gene_off, uint64_t n_off,
                           const uint16_t *gene_ids, uint16_t *h_gene_ids, uint64_t h_ids_cap, const uint32_t *uni_flag, hipStream_t stream);
// a host batch's records of one kind -> pinned host memory: `units` records of words_per_unit 32-bit words each from src (16-byte aligned, as
// h_dst).  With `counters`: units = min(the batch's associations, limit), none for a batch that overflowed; nullptr: units = limit
int launch_publish_records(const uint32_t *counters, const void *src, void *h_dst, uint64_t limit, uint32_t words_per_unit, hipStream_t stream);
int launch_classify_uni(Ctx *ctx, const ClassifyParams &p, uint32_t max_slots, int rmode, hipStream_t stream);   // 0 ragged, 1 uniform, 2 by classes (CLS)
int launch_class_prepass(const ClassifyParams &p, uint32_t slot_cap, uint32_t *flag, hipStream_t stream);   // behind launch_uniform_check: histogram, plan, scatter
bool class_kernel_available(const Ctx *ctx, uint32_t max_slots);
bool offsets_kernel_available(const Ctx *ctx, uint32_t max_slots, bool hasq);
bool offsets_kernel_fits(const Ctx *ctx, uint32_t max_slots, uint32_t L1, uint32_t L2);
int launch_uniform_check(const ClassifyParams &p, uint32_t slot_cap, uint32_t *flag, hipStream_t stream, bool beside = false);   // beside: while a classify kernel holds the CUs
bool uni_kernel_available(const Ctx *ctx);
// anchor_verdict.hip
bool anchor_verdict_applies(const ClassifyParams &p);
int launch_anchor_verdict(const ClassifyParams &p, bool pow2, bool ragged, hipStream_t stream);
uint32_t fast_kernel_max_slots();
uint32_t fast_kernel_unroll(uint32_t max_slots);  // U of the specialisation chosen for max_slots (0 = unknown)
uint32_t uni_kernel_max_groups(uint32_t max_slots);   // staging groups per pair classify_uni_kernel can take at that specialisation

// the records of the batch whose result was handed out last, per kind (shk_*_last).  valid = false: that batch had none of the kind, or it
// was refused, or it was a measurement (shk_count_work).  Pointers into the batch's Slot: pinned host memory for a host batch, else device
struct LastRecords {
  uint64_t n = 0, n_assoc = 0;      // the batch's reads (evidence, candidates) and associations (every other kind)
  bool evid_valid = false;
  const shk_read_evidence *evid = nullptr;
  bool cand_valid = false;
  uint32_t cand_m = 0;
  const shk_read_candidates *cand_reads = nullptr;
  const shk_candidate *cand_entries = nullptr;
  bool place_valid = false;
  const shk_placement *place = nullptr;
  bool seg_valid = false;
  uint32_t seg_m = 0;
  const uint32_t *seg_keys = nullptr;
  const shk_segment *seg_entries = nullptr;
  bool align_valid = false;
  const shk_mate_alignment *align = nullptr;
  bool pairs_valid = false;
  const shk_pair *pairs = nullptr;
  bool rescue_valid = false;
  const shk_rescue *rescue = nullptr;
};

struct Ctx {
  shk_params prm{};
  int mode = 0;  // 0 = accepting references, 2 = frozen (bloomfilter.h:104-110)
  hipStream_t stream = nullptr;
  std::string last_error;

  // buffered reference records (host)
  std::vector<char> ref_bytes;
  std::vector<uint64_t> ref_off{0};

  DeviceIndex idx;
  uint64_t n_records = 0, nidx = 0, n_ref_kmers = 0;

  // classify workspace: one Slot per batch in flight (PIPE_DEPTH for shk_classify_submit/_wait plus one for
  // shk_classify_device); the general kernel's scratch is shared (kernels of one context run on one stream)
  Slot slots[PIPE_DEPTH + 1];
  uint64_t next_ticket = 1;
  hipStream_t h2d_stream = nullptr, d2h_stream = nullptr;
  DevArray<uint64_t> scratch;
  unsigned long long *d_gene_counts = nullptr;
  unsigned long long *d_gene_totals = nullptr;   // result of the all-reduce (the per-GPU counters stay local)
  unsigned long long *d_work_counters = nullptr;
  int8_t q8 = 0;                                  // min_quality as the reference's `char` (argument_parser.hpp:59,:144)
  // RCCL communicators, created once: one-process-per-GPU (shk_dist_init) and one-process-many-GPUs (allreduce over contexts)
  void *dist_comm = nullptr;
  int dist_rank = 0, dist_world = 1;
  void *group_comm = nullptr;
  std::vector<int> group_devs;

  // test / A-B switches of the environment, read ONCE when the context is created (never per launch):
  //   SHK_FORCE_GENERIC=1  every batch through classify_fast_kernel (the tests run both code paths)
  //   SHK_BIG_LDS_ALWAYS=1 panels of 60-150 genes stay on the 128 KiB LDS summary whatever the previous batch said
  int env_tile_first = 0;           // SHK_TILE_FIRST=1: the tiles' round for every batch it can serve (tests); =0: never; unset: by the last batch's assigned fraction
  bool env_no_tro = false;          // SHK_NO_TRO=1: trimmed batches never through the three-pairs kernel by offsets (the class-by-class path instead; tests, A/B timing)
  bool env_force_tro = false;      // SHK_FORCE_TRO=1: batches of one length through the offsets kernel as well (diagnostic: what the offsets cost)
  bool env_no_tri = false;          // SHK_NO_TRI=1: no three-pairs-per-pass instantiation (A/B timing, tests)
  bool env_plain_tail = false;      // SHK_PLAIN_TAIL=1: a one-record index's results through gather, EMIT pass and histogram as every other index's (A/B timing, tests)
  bool env_no_pre_verdict = false;  // SHK_NO_PRE_VERDICT=1: no anchor_verdict_kernel in front of the table kernels (A/B timing, tests)
  bool env_anchor_always = false;   // SHK_ANCHOR_ALWAYS=1: the anchored extension for every batch of an index that has the reference arrays (tests, A/B timing)
  bool env_ktab_always = false;     // SHK_KTAB=1: the minimiser table for every batch of an index that has it (tests)
  bool env_ktab_nt = false, env_ktab_plain = false;   // SHK_KTAB_NT=1 / 0: the minimiser table probed with / without non-temporal loads whatever its size (A/B timing, tests)
  bool env_force_generic = false, env_big_lds_always = false, env_cls_always = false;   // SHK_CLS_MIN_FILL given: no adapting to the stream
  uint32_t last_verdict = 0;        // CTR_VERDICT of the last batch finished
  // speculation (shark_hip.hip, enqueue_classify): what shk_classify_device's last batch was like when the device judged it uniform
  struct SpecPrev {
    bool valid = false;             // the batch finished last came through shk_classify_device and the device's verdict was "uniform"
    bool paired = false, quals = false;
    uint32_t max_slots = 0, L1 = 0, L2 = 0;
  } spec_prev;
  bool env_no_speculate = false;    // SHK_NO_SPECULATE=1: the check always in front of the classify launches (A/B timing, tests)
  bool env_spec_in_front = false;   // SHK_SPECULATE_IN_FRONT=1: a speculated batch's check in front of its classify launch on the one stream (A/B timing)
  int last_speculation = 0;         // shk_debug_last_speculation: 0 not speculated, 1 speculated and held, 2 speculated and redone
  hipStream_t chk_stream = nullptr; // a speculated batch's uniform_check_kernel runs here, beside the classify kernel
  hipEvent_t ev_chk_go = nullptr, ev_chk_done = nullptr;
  uint32_t env_cls_min_fill = CLS_MIN_FILL;   // SHK_CLS_MIN_FILL: pairs per non-empty class a batch needs to go class by class (0: never; tests: 1)
  // which classify kernel the last batch's main launch was (shk_last_kernel): the choice can depend on the batch before it
  char last_kernel[160] = "";
  // what finalize builds beside the filter
  bool keep_positions = false;      // DeviceIndex::ptab (shk_ref_keep_positions)
  bool kmer_table = true;           // DeviceIndex::kxtab where it applies (shk_ref_kmer_table; SHK_NO_KMER_TABLE=1: never)
  // the per-batch record modes: what the batches submitted from now on run with (0 / false: off).  Their records are handed out with the
  // batch's result: last_rec
  bool evidence = false;            // shk_evidence_enable: the evidence instantiations
  uint32_t cand_m = 0;              // shk_candidates_enable: entries per read
  bool placement = false;           // shk_placement_enable (an index built with shk_ref_keep_positions)
  uint32_t seg_m = 0;               // shk_segments_enable (segments.hip): entries per mate
  LastRecords last_rec;
  // the accumulated states (above), which outlive their modes' being switched off, and the list of splice sites
  std::vector<uint64_t> gene_start;            // host copy of DeviceIndex::gene_start (empty: the index carries none)
  DepthState depth;
  JunctionState junc;
  CounterState pileup;
  FragmentState frag;
  IndelState indel;
  bool keep_bases = false;                     // finalize builds DeviceIndex::recbase (shk_ref_keep_bases)
  VariantScratch var;
  SpliceSites splice;
  // alignments mode (shk_alignments_enable; align.hip), as segments mode: the floor for the batches submitted from now on (0: off)
  uint32_t align = 0;
  uint32_t ext_p = 0, ext_b = 0;               // shk_alignments_extend: mismatch penalty (0: off) and end bonus for the batches submitted from now on
  bool env_pairs_global = false;               // SHK_PAIRS_GLOBAL_ATOMICS=1: the histogram by one global atomic per pair (A/B timing only)
  // rescue mode (shk_rescue_enable; rescue.hip): per-batch records as pairs mode's; no state of its own
  uint32_t rescue_max_frag = 0;                // for the batches submitted from now on (0: off)
  uint32_t rescue_min_intron = 0, rescue_max_cost = 0, rescue_min_gap = 0;

  // timing
  bool timing = false;
  std::vector<hipEvent_t> ev_start, ev_stop, ev_pre;   // per launch: in front of the classify launches, behind them, in front of the passes over the offsets
  size_t ev_used = 0;
  shk_timing last{};
};

// error helper
#define SHK_HIP(ctx, call)                                            \
  do {                                                                \
    hipError_t e__ = (call);                                          \
    if (e__ != hipSuccess) return shk::set_hip_error(ctx, e__, #call); \
  } while (0)

}  // namespace shk

// the opaque context of the C ABI
struct shk_ctx : public shk::Ctx {};
