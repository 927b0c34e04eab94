// shark_hip.hip -- the C ABI of libsharkhip (include/shark_hip.h): context,
// device memory, and the orchestration around the HIP kernels.  No CPU
// implementation of any hot-path step lives here: without a device every
// computing entry point fails.
#include <hip/hip_runtime.h>
#include <chrono>
#include <mutex>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <dlfcn.h>
#include <unistd.h>
#include <cstring>
#include <new>
#include <tuple>

#include "device_scan.hpp"
#include "shark_internal.hpp"

namespace shk {

int set_hip_error(Ctx *ctx, hipError_t e, const char *what)
{
  if (ctx) {
    ctx->last_error = std::string(what) + ": " + hipGetErrorString(e);
  }
  return e == hipErrorOutOfMemory ? SHK_ERR_NOMEM : SHK_ERR_HIP;
}

static void free_index(DeviceIndex &ix)
{
  hipFree(ix.bf64); hipFree(ix.rank_w); hipFree(ix.ent); hipFree(ix.ids); hipFree(ix.sum32); hipFree(ix.tab); hipFree(ix.lsum32); hipFree(ix.lbig32); hipFree(ix.ltab); hipFree(ix.kxtab); hipFree(ix.kxkeys); hipFree(ix.ref2); hipFree(ix.refpay); hipFree(ix.refext); hipFree(ix.refmul); hipFree(ix.atab); hipFree(ix.ktab);
  hipFree(ix.ptab); hipFree(ix.pdir); hipFree(ix.gene_start); hipFree(ix.recbase);
  ix = DeviceIndex{};
}

// ---- tracing hook: roctx ranges around the library's phases, so that a rocprofv3 --marker-trace /
// --sys-trace timeline shows index build, submit and wait next to the kernels.  Off unless SHK_ROCTX=1; libroctx64 is
// loaded on first use, nothing is linked.
namespace {
struct Roctx {
  int (*push)(const char *) = nullptr;
  int (*pop)() = nullptr;
  bool tried = false;
};
Roctx &roctx()
{
  static Roctx r;
  if (!r.tried) {
    r.tried = true;
    const char *e = getenv("SHK_ROCTX");
    if (e && e[0] == '1') {
      void *lib = dlopen("libroctx64.so.4", RTLD_NOW | RTLD_LOCAL);
      if (!lib) lib = dlopen("libroctx64.so", RTLD_NOW | RTLD_LOCAL);
      if (lib) {
        r.push = (int (*)(const char *))dlsym(lib, "roctxRangePushA");
        r.pop = (int (*)())dlsym(lib, "roctxRangePop");
      }
    }
  }
  return r;
}
}  // namespace
struct TraceRange {
  explicit TraceRange(const char *name) { if (roctx().push) { (void)roctx().push(name); on = true; } }
  ~TraceRange() { if (on && roctx().pop) (void)roctx().pop(); }
  bool on = false;
};

// slot positions of a read (pair) whose mates are `len` long: classify.hip packs mate 2 at the next
// multiple of 8 after mate 1 and uses packed positions as k-mer slots
static uint32_t slots_for_len(uint32_t len, uint32_t k, bool paired)
{
  const uint32_t per = len >= k ? len - k + 1 : 0;
  return (paired && per) ? ((len + 7u) & ~7u) + per : per;
}

// exact slot count of one read (pair): the `ns` of classify.hip's process_read
static uint32_t slots_of_read(uint64_t L1, uint64_t L2, uint32_t k)
{
  const uint64_t nk1 = L1 >= k ? L1 - k + 1 : 0, nk2 = L2 >= k ? L2 - k + 1 : 0;
  const uint64_t ns = nk2 ? ((L1 + 7u) & ~7ull) + nk2 : nk1;
  return ns > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)ns;
}

static int slot_init(Ctx *ctx, Slot &s)
{
  // (the batch's counters and, behind them, the words of the uniformity check: one allocation, cleared by one memset per batch)
  SHK_HIP(ctx, hipMalloc((void **)&s.d_counters, (COUNTER_BLOCK_WORDS + UNI_FLAG_WORDS) * sizeof(uint32_t)));
  s.d_uni_flag = s.d_counters + COUNTER_BLOCK_WORDS;
  SHK_HIP(ctx, hipMalloc((void **)&s.d_out, sizeof(ClassifyOut)));
  SHK_HIP(ctx, hipHostMalloc((void **)&s.h_counters, CTR_WORDS * sizeof(uint32_t), hipHostMallocDefault));
  SHK_HIP(ctx, hipEventCreateWithFlags(&s.ev_h2d, hipEventDisableTiming));
  SHK_HIP(ctx, hipEventCreateWithFlags(&s.ev_done, hipEventDisableTiming));
  SHK_HIP(ctx, hipEventCreateWithFlags(&s.ev_d2h, hipEventDisableTiming));
  return SHK_OK;
}

static void slot_free(Slot &s)
{
  hipFree(s.d_counters); hipFree(s.d_out); hipFree(s.d_cls_share);
  if (s.h_counters) (void)hipHostFree(s.h_counters);
  if (s.ev_h2d) (void)hipEventDestroy(s.ev_h2d);
  if (s.ev_done) (void)hipEventDestroy(s.ev_done);
  if (s.ev_d2h) (void)hipEventDestroy(s.ev_d2h);
  s = Slot{};   // (every growable buffer frees itself)
}

// result buffers of a batch of n reads; *d_out is rewritten only when one of them moved (a blocking
// copy: never on the steady-state path of the pipeline)
static int slot_reserve(Ctx *ctx, Slot &s, uint64_t n)
{
  int rc;
  if ((rc = s.d_count.reserve(ctx, n + 1))) return rc;
  if ((rc = s.d_inl.reserve(ctx, n * SHK_INLINE_IDS + 8))) return rc;
  if ((rc = s.d_gene_off.reserve(ctx, n + 1))) return rc;
  if ((rc = s.d_long_queue.reserve(ctx, n + 1))) return rc;
  if ((rc = s.d_tie_queue.reserve(ctx, 3 * n + 3))) return rc;
  if ((rc = s.d_scan_temp.reserve(ctx, scan_temp_words(n + 1)))) return rc;
  // associations: two per read to start with; a batch that needs more is finished by the overflow path
  if ((rc = s.d_gene_ids.reserve(ctx, 2 * n + 4096))) return rc;
  // (evidence mode only: 12 bytes per read that no other batch pays for)
  if (s.evidence && (rc = s.rec_evid.d.reserve(ctx, n + 1))) return rc;
  // (candidates mode only: 8 + 12 m bytes per read; the spare records keep publish_records_kernel's 16-byte copies inside)
  if (s.cand_m && (rc = s.rec_cand_reads.d.reserve(ctx, n + 2))) return rc;
  if (s.cand_m && (rc = s.rec_cand_entries.d.reserve(ctx, n * s.cand_m + 2))) return rc;
  ClassifyOut ho{};
  ho.evid = s.evidence ? s.rec_evid.d.p : nullptr;
  ho.cand_reads = s.cand_m ? s.rec_cand_reads.d.p : nullptr;
  ho.cand_entries = s.cand_m ? s.rec_cand_entries.d.p : nullptr;
  ho.cand_m = s.cand_m;
  ho.count = s.d_count.p; ho.inl = s.d_inl.p; ho.counters = s.d_counters; ho.long_queue = s.d_long_queue.p; ho.tie_queue = s.d_tie_queue.p;
  if (memcmp(&ho, &s.out_shadow, sizeof(ho)) != 0) {
    SHK_HIP(ctx, hipMemcpy(s.d_out, &ho, sizeof(ho), hipMemcpyHostToDevice));
    s.out_shadow = ho;
  }
  return SHK_OK;
}

static void fill_params(Ctx *ctx, Slot &s, const shk_batch *b)
{
  ClassifyParams p{};
  const DeviceIndex &ix = ctx->idx;
  p.bf64 = ix.bf64; p.rank_w = ix.rank_w; p.ent = ix.ent; p.ids = ix.ids;
  p.sum32 = ix.sum_shift ? ix.sum32 : nullptr; p.sum_shift = ix.sum_shift;
  p.tab = ix.tab_lg ? ix.tab : nullptr; p.tab_lg = ix.tab_lg;
  p.tab_nt = ix.tab_lg && (16ull << ix.tab_lg) > (256ull << 20);   // beyond L2 + Infinity Cache
  p.lsum32 = ix.lsum_shift ? ix.lsum32 : nullptr; p.lsum_shift = ix.lsum_shift;
  p.lx_gene = 0xFFFFFFFFu;   // (launch_classify_uni sets it when it chooses the exact LDS table)
  p.ref2 = ix.ref2; p.refpay = ix.refpay; p.atab = ix.atab; p.ref_total = ix.ref_total; p.refext = ix.refext; p.refmul = ix.refmul;
  p.ktab = ix.ktab_lg ? ix.ktab : nullptr; p.ktab_lg = ix.ktab_lg; p.ktab_w = ix.ktab_w;
  // (far beyond the caches: streaming loads -- 17.8 / 18.1 -> 16.7 / 17.3 ms per 10 M pairs at 0 / 50 % on-target on the 60 000-gene index)
  p.ktab_nt = (ix.ktab_lg && (16ull << ix.ktab_lg) > (256ull << 20) && !ctx->env_ktab_plain) || ctx->env_ktab_nt ? 1u : 0u;
  p.bf_bits = ix.bf_bits;
  p.bf_mask = ix.pow2 ? ix.bf_bits - 1 : ~0ull;   // (non power-of-two: positions are reduced explicitly, the masks become no-ops)
  if (!ix.pow2) {
    const uint32_t sh = (uint32_t)__builtin_ctzll(ix.bf_bits);
    const uint64_t m = ix.bf_bits >> sh;
    p.mod_shift = sh;
    p.mod_fast = sh >= 32 && m < (1ull << 32);
    p.mod_m = p.mod_fast ? (uint32_t)m : 0;
    p.mod_c = p.mod_fast ? 0xFFFFFFFFFFFFFFFFull / m + 1 : 0;
  }
  p.k = ctx->prm.k; p.c = ctx->prm.c; p.single = ctx->prm.single;
  // FastqSplitter.hpp:52,:70 with the reference's `char min_quality` (argument_parser.hpp:59,:144): no masking when the
  // char is 0; otherwise the threshold is (char)(min_quality + 33), which wraps for -q > 94 just as it does there
  p.hasq = ctx->q8 != 0;
  p.mq = (int32_t)(int8_t)(uint8_t)((int)ctx->q8 + 33);
  p.n = b->n;
  p.seq1 = (const uint8_t *)b->seq1; p.off1 = b->off1;
  p.seq2 = (const uint8_t *)b->seq2; p.off2 = b->off2;
  p.qual1 = (const uint8_t *)b->qual1; p.qual2 = (const uint8_t *)b->qual2;
  p.out = s.d_out;
  p.flags = s.d_counters;
#ifdef SHK_ABLATION
  p.ablate = getenv("SHK_ABLATE") ? (uint32_t)atoi(getenv("SHK_ABLATE")) : 0u;
#endif
  s.p = p;
}

// scratch of the general kernel for `n_items` work items of at most `slots` k-mer slots
static int size_scratch(Ctx *ctx, ClassifyParams &p, uint32_t slots, uint64_t n_items, unsigned *n_waves)
{
  const uint32_t S = ((slots + 63) / 64) * 64;
  const uint64_t stride = (uint64_t)stage_words_for(S) + (3ull * S) / 2 + 2;   // staging area + 3 u32 slot records
  uint64_t waves = std::min<uint64_t>(std::max<uint64_t>(n_items, 1), 4096);
  const uint64_t budget_words = (1ull << 31) / 8;  // at most 2 GiB of scratch
  if (waves * stride > budget_words) waves = std::max<uint64_t>(1, budget_words / stride);
  waves = ((waves + 3) / 4) * 4;
  int r = ctx->scratch.reserve(ctx, waves * stride);
  if (r) return r;
  p.scratch = ctx->scratch.p;
  p.scratch_stride_words = stride;
  p.scratch_slots = S;
  *n_waves = (unsigned)waves;
  return SHK_OK;
}

// reads queued for the general kernel because they exceed the fast kernel's slot capacity
static int run_long_reads(Ctx *ctx, Slot &s, uint32_t n_long)
{
  if (!n_long) return SHK_OK;
  ClassifyParams p = s.p;
  unsigned n_waves = 0;
  int rc;
  if ((rc = size_scratch(ctx, p, s.gen_slots, n_long, &n_waves))) return rc;
  p.work = s.d_long_queue.p;
  p.n_work = n_long;
  p.work_count = nullptr;
  return launch_classify_general(ctx, p, false, n_waves, ctx->stream, s.evidence, s.cand_m != 0);
}

// a host batch's records of one kind into their pinned mirror, which is reserved for `need` records first.  Per association, `per_assoc`
// records each: as many associations as the device array and the mirror both hold, and at most `bound` (what the kernel that wrote them held)
template <typename T>
static int publish_assoc(Ctx *ctx, const Slot &s, Mirrored<T> &rec, size_t need, uint32_t per_assoc, uint64_t bound)
{
  if (const int rc = rec.h.reserve(ctx, need)) return rc;
  const uint64_t limit = std::min<uint64_t>(std::min<uint64_t>(rec.h.cap, rec.d.cap) / per_assoc, bound);
  return launch_publish_records(s.d_counters, rec.d.p, rec.h.p, limit, per_assoc * (uint32_t)(sizeof(T) / 4), ctx->stream);
}
// ... and per read, `per_read` records each (the spare records in `need` keep the 16-byte copies inside)
template <typename T>
static int publish_reads(Ctx *ctx, const Slot &s, Mirrored<T> &rec, size_t need, uint32_t per_read)
{
  if (const int rc = rec.h.reserve(ctx, need)) return rc;
  return launch_publish_records(nullptr, rec.d.p, rec.h.p, s.n, per_read * (uint32_t)(sizeof(T) / 4), ctx->stream);
}

// The record modes of the batch in `s`, behind its assembled result (gene_off / gene_ids as they now stand: a redone batch comes through
// here again).  Each mode: reserve its device array for as many associations as d_gene_ids holds, launch, and for a host batch publish into
// the pinned mirror (per read: evidence and candidates, whose records the classify kernels wrote).  The modes that add to a state of the
// context do so under gene_hist_kernel's rule for a batch that comes through here again (skip_if_long)
static int enqueue_record_modes(Ctx *ctx, Slot &s, bool skip_if_long)
{
  hipStream_t st = ctx->stream;
  const uint64_t n = s.n;
  const size_t ids = s.d_gene_ids.cap;
  const bool host = s.host_batch;
  int rc;
  if (s.evidence && host && (rc = publish_reads(ctx, s, s.rec_evid, n + 1, 1))) return rc;
  if (s.cand_m && host) {
    if ((rc = s.rec_cand_entries.h.reserve(ctx, n * s.cand_m + 2))) return rc;   // (both mirrors in front of both launches)
    if ((rc = publish_reads(ctx, s, s.rec_cand_reads, n + 2, 1))) return rc;
    if ((rc = publish_reads(ctx, s, s.rec_cand_entries, n * s.cand_m + 2, s.cand_m))) return rc;
  }
  // (depth mode needs placement's records as well: the kernel runs for either mode, only placement mode hands its records out)
  if (s.placement || s.depth) {
    if ((rc = s.rec_place.d.reserve(ctx, ids))) return rc;
    if ((rc = launch_placement(ctx, s, st))) return rc;
    if (s.depth && (rc = launch_depth_accumulate(ctx, s, skip_if_long, st))) return rc;
    if (s.placement && host && (rc = publish_assoc(ctx, s, s.rec_place, ids, 1, ~0ull))) return rc;
  }
  if (s.seg_m) {
    if ((rc = s.rec_seg_keys.d.reserve(ctx, 2 * ids))) return rc;
    if ((rc = s.rec_seg_entries.d.reserve(ctx, 2 * ids * s.seg_m))) return rc;
    if ((rc = launch_segments(ctx, s, st))) return rc;
    if (host) {
      if ((rc = s.rec_seg_keys.h.reserve(ctx, 2 * ids))) return rc;
      if ((rc = s.rec_seg_entries.h.reserve(ctx, 2 * ids * s.seg_m))) return rc;
      // (the two arrays hold associations together: one bound for both)
      const uint64_t both = std::min(segments_cap(s.rec_seg_keys.h, s.rec_seg_entries.h, s.seg_m), segments_cap(s.rec_seg_keys.d, s.rec_seg_entries.d, s.seg_m));
      if ((rc = launch_publish_records(s.d_counters, s.rec_seg_keys.d.p, s.rec_seg_keys.h.p, both, 2, st))) return rc;
      if ((rc = launch_publish_records(s.d_counters, s.rec_seg_entries.d.p, s.rec_seg_entries.h.p, both, 2 * s.seg_m * (uint32_t)(sizeof(shk_segment) / 4), st))) return rc;
    }
  }
  // the readers of segments_kernel's records at m = SHK_MAX_SEGMENTS -- segments mode's own where it runs at that m, else a launch of that
  // kernel into arrays nobody else sees --: spliced depth and the junction table; pileup; aligned pileup (align_kernel's accumulating
  // instantiation in pileup_kernel's stead: the same launch as alignments mode's where the two floors are equal, else one of its own);
  // alignments mode, the one with records of its own per association
  if (!(s.sp_depth || s.sp_junc || s.pileup || s.align || s.pileup_al || s.indels)) return SHK_OK;
  const shk_segment *entries = s.rec_seg_entries.d.p;
  uint64_t cap_assoc = segments_cap(s.rec_seg_keys.d, s.rec_seg_entries.d, s.seg_m);
  if (s.seg_m != SHK_MAX_SEGMENTS) {
    if ((rc = s.d_sp_keys.reserve(ctx, 2 * ids))) return rc;
    if ((rc = s.d_sp_entries.reserve(ctx, 2 * ids * SHK_MAX_SEGMENTS))) return rc;
    entries = s.d_sp_entries.p;
    cap_assoc = segments_cap(s.d_sp_keys, s.d_sp_entries, SHK_MAX_SEGMENTS);
    if ((rc = launch_segments_into(ctx, s, SHK_MAX_SEGMENTS, s.d_sp_keys.p, s.d_sp_entries.p, cap_assoc, st))) return rc;
  }
  if ((s.sp_depth || s.sp_junc) && (rc = launch_spliced_accumulate(ctx, s, entries, cap_assoc, skip_if_long, st))) return rc;
  if (s.pileup && (rc = launch_pileup(ctx, s, entries, cap_assoc, skip_if_long, st))) return rc;
  const bool acc_with_records = s.pileup_al && s.pileup_al == s.align;
  if (s.pileup_al && !acc_with_records && (rc = launch_alignments(ctx, s, entries, cap_assoc, skip_if_long, false, true, st))) return rc;
  // (indels mode reads align_kernel's records at its own floor: alignments mode's where the floors are equal, else those of one more storing
  //  launch into an array nobody else sees; indel_kernel directly behind the launch that stored them)
  const bool indels_with_records = s.indels && s.indels == s.align;
  if (s.indels && !indels_with_records) {
    if ((rc = s.d_indel_align.reserve(ctx, 2 * ids))) return rc;
    if ((rc = launch_alignments_into(ctx, s, entries, cap_assoc, skip_if_long, s.indels, s.d_indel_align.p, s.d_indel_align.cap, st))) return rc;
    if ((rc = launch_indels(ctx, s, s.d_indel_align.p, std::min<uint64_t>(cap_assoc, s.d_indel_align.cap / 2), skip_if_long, st))) return rc;
  }
  if (!s.align) return SHK_OK;
  if ((rc = s.rec_align.d.reserve(ctx, 2 * ids))) return rc;
  if ((rc = launch_alignments(ctx, s, entries, cap_assoc, skip_if_long, true, acc_with_records, st))) return rc;
  if (indels_with_records && (rc = launch_indels(ctx, s, s.rec_align.d.p, std::min<uint64_t>(cap_assoc, s.rec_align.d.cap / 2), skip_if_long, st))) return rc;
  // (rescue mode: a mate without a block placed beside its partner, in front of everything that reads the alignment records)
  if (s.rescue) {
    if ((rc = s.rec_rescue.d.reserve(ctx, ids))) return rc;
    if ((rc = s.d_rescue_queue.reserve(ctx, ids + 2))) return rc;
    if ((rc = launch_rescue(ctx, s, cap_assoc, skip_if_long, st))) return rc;
    if (host && (rc = publish_assoc(ctx, s, s.rec_rescue, ids, 1, cap_assoc))) return rc;
  }
  // (pairs mode: the two mates' records of an association read together, directly behind the kernels that stored them)
  if (s.pairs) {
    if ((rc = s.rec_pairs.d.reserve(ctx, ids))) return rc;
    if ((rc = launch_pairs(ctx, s, cap_assoc, skip_if_long, st))) return rc;
    if (host && (rc = publish_assoc(ctx, s, s.rec_pairs, ids, 1, cap_assoc))) return rc;
  }
  if (host && (rc = publish_assoc(ctx, s, s.rec_align, 2 * ids, 2, cap_assoc))) return rc;
  return SHK_OK;
}

// Everything behind the classify kernels, WITHOUT a host round trip: per-read counts -> offsets (scan), inline ids ->
// CSR (gather), reads with more than SHK_INLINE_IDS genes (EMIT pass of the general kernel over the tie queue, whose
// length stays on the device), per-gene histogram, counters -> pinned host memory, the record modes, event.
static int enqueue_tail(Ctx *ctx, Slot &s, bool skip_hist_if_long, bool count_genes)
{
  hipStream_t st = ctx->stream;
  const uint64_t n = s.n;
  int rc;
  // An index of one record without wrap: a read's list is {} or {0}, whichever kernel classified it, so gene_ids is `total` copies of id 0,
  // gene 0 was assigned `total` reads and the tie queue is empty by construction -- the scan assembles all of it in its own three
  // launches (device_scan.hpp, OneRecordResult): no finalize, gather, EMIT or histogram launch.  SHK_PLAIN_TAIL=1: the sequence below
  const bool one_record = ctx->n_records == 1 && !ctx->idx.wrap && !ctx->env_plain_tail;
  if (one_record) {
    // (a speculated batch: the scan's epilogue compares the check's words with what the classify launch assumed -- enqueue_classify)
    const OneRecordResult r{s.d_gene_ids.p, s.d_gene_ids.cap, s.d_counters, ctx->d_gene_counts, count_genes, skip_hist_if_long,
                            s.speculated ? s.d_uni_flag : nullptr, s.p.uni_L1, s.p.uni_L2};
    (void)exclusive_scan_assemble_one(s.d_count.p, s.d_gene_off.p, n + 1, s.d_scan_temp.p, r, st);
    SHK_HIP(ctx, hipGetLastError());
  } else {
    const uint64_t *d_total = exclusive_scan_u32(s.d_count.p, s.d_gene_off.p, n + 1, s.d_scan_temp.p, st);
    SHK_HIP(ctx, hipGetLastError());
    if ((rc = launch_finalize_total(d_total, s.d_counters, s.d_gene_ids.cap, st))) return rc;
    if ((rc = launch_gather_inline(s.d_count.p, s.d_inl.p, s.d_gene_off.p, s.d_gene_ids.p, n, s.d_counters, st))) return rc;
    ClassifyParams p = s.p;
    unsigned n_waves = 0;
    if ((rc = size_scratch(ctx, p, s.gen_slots, std::min<uint64_t>(n, 1024), &n_waves))) return rc;
    p.work = s.d_tie_queue.p;
    p.n_work = 0;
    p.work_count = s.d_counters + CTR_TIE;
    p.gene_off = s.d_gene_off.p;
    p.gene_ids = s.d_gene_ids.p;
    if ((rc = launch_classify_general(ctx, p, true, n_waves, st))) return rc;
    if (count_genes && (rc = launch_gene_hist(s.d_gene_ids.p, s.d_counters, skip_hist_if_long, ctx->d_gene_counts, n, ctx->n_records, st))) return rc;
  }
  // counters (and, for host batches, the associations) are stored into pinned host memory by a kernel: no copy-engine
  // command ever sits in this stream waiting for kernels (see publish_results_kernel)
  if (s.host_batch) {
    if ((rc = s.h_gene_off.reserve(ctx, n + 1))) return rc;
    if ((rc = s.h_gene_ids.reserve(ctx, s.d_gene_ids.cap))) return rc;
  }
  if ((rc = launch_publish_results(s.d_counters, s.h_counters, s.d_gene_off.p, s.host_batch ? s.h_gene_off.p : nullptr, n + 1, s.d_gene_ids.p,
                                   s.h_gene_ids.p, s.h_gene_ids.cap, s.p.uni_flag, st)))
    return rc;
  if ((rc = enqueue_record_modes(ctx, s, skip_hist_if_long))) return rc;
  SHK_HIP(ctx, hipEventRecord(s.ev_done, st));
  return SHK_OK;
}

enum LongMode {
  LONG_NONE_EXPECTED = 0,   // the caller's length bound says every read fits the fast kernel; checked after the fact
  LONG_KNOWN = 1,           // the host has counted the reads that do not fit (host batches)
  LONG_UNKNOWN = 2          // no bound: one host round trip behind the fast kernel
};

// what the device said about the batch just finished (0: the host knew); shk_last_kernel() carries it
static void note_verdict(Ctx *ctx, uint32_t v)
{
  ctx->last_verdict = v;
  ctx->spec_prev.valid = false;   // (classify_resident says so again behind a batch of its own)
  ctx->last_speculation = 0;
  if (char *e = strstr(ctx->last_kernel, " verdict=")) *e = 0;
  if (v) {
    const size_t l = strlen(ctx->last_kernel);
    snprintf(ctx->last_kernel + l, sizeof(ctx->last_kernel) - l, " verdict=%s", v == 1u ? "ragged" : (v == 2u ? "uniform" : (v == 3u ? "classes" : "offsets")));
  }
}

// all kernels of one batch whose inputs are (or will be, in stream order) resident in HBM; batch pointers are device
// pointers.  Returns with the work enqueued on ctx->stream; finish_classify() completes the rare slow paths.
enum UniMode {
  UNI_ASK_DEVICE = 0,  // lengths unknown on the host: the device decides (uniform / ragged / by classes), every candidate kernel is launched, all but one return at once
  UNI_YES = 1,         // the host has seen the offsets: one length per mate (uni_L1, uni_L2), and such a read fits
  UNI_NO = 2
};

static int enqueue_classify(Ctx *ctx, Slot &s, const shk_batch *b, uint32_t max_slots, int long_mode, uint32_t n_long_host,
                            uint32_t long_slots_host, bool count_genes, int uni_mode = UNI_ASK_DEVICE, uint32_t uni_L1 = 0, uint32_t uni_L2 = 0,
                            bool groups_fit = true, bool may_speculate = false)
{
  hipStream_t st = ctx->stream;
  const uint64_t n = b->n;
  int rc;
  s.evidence = ctx->evidence;
  s.cand_m = ctx->cand_m;
  s.placement = ctx->placement;
  s.seg_m = ctx->seg_m;
  s.depth = count_genes && !ctx->depth.kind ? ctx->depth.floor : 0u;   // (shk_count_work is a measurement: its batch is not counted)
  s.sp_depth = count_genes && ctx->depth.kind ? ctx->depth.floor : 0u;
  s.sp_junc = count_genes ? ctx->junc.floor : 0u;
  s.pileup = count_genes && !ctx->pileup.kind ? ctx->pileup.floor : 0u;
  s.pileup_al = count_genes && ctx->pileup.kind ? ctx->pileup.floor : 0u;
  s.align = ctx->align;
  s.ext_p = ctx->ext_p;
  s.ext_b = ctx->ext_b;
  s.spl_h = ctx->splice.h;
  s.spl_cost = ctx->splice.cost;
  s.spl_gap = ctx->splice.gap;
  s.pairs = s.align ? ctx->frag.n_bins : 0u;      // (pair records only behind alignment records)
  s.pairs_min_intron = ctx->frag.min_intron;
  s.pairs_max_frag = ctx->frag.max_frag;
  s.pairs_count = s.pairs && count_genes;
  s.rescue = s.align ? ctx->rescue_max_frag : 0u;   // (rescue only behind alignment records)
  s.rescue_min_intron = ctx->rescue_min_intron;
  s.rescue_max_cost = ctx->rescue_max_cost;
  s.rescue_min_gap = ctx->rescue_min_gap;
  if (s.pairs_count) ctx->frag.dirty = true;
  if (s.pileup || s.pileup_al) ctx->pileup.dirty = true;
  if (s.depth || s.sp_depth) ctx->depth.dirty = true;
  if (s.sp_junc) ctx->junc.dirty = true;
  s.indels = count_genes ? ctx->indel.floor : 0u;
  s.indels_min_intron = ctx->indel.min_intron;
  if (s.indels) ctx->indel.dirty = true;
  if ((rc = slot_reserve(ctx, s, n))) return rc;
  s.n = n;
  fill_params(ctx, s, b);
  SHK_HIP(ctx, hipMemsetAsync(s.d_counters, 0, (COUNTER_BLOCK_WORDS + UNI_FLAG_WORDS) * sizeof(uint32_t), st));
  if (max_slots > fast_kernel_max_slots()) max_slots = fast_kernel_max_slots();
  s.fast_cap = 64 * fast_kernel_unroll(max_slots);
  s.gen_slots = s.fast_cap;
  // an index with a position table: classify_uni_kernel, uniform or not -- unless the batch is known to hold reads of more
  // than 64 staging groups (> 512 bases per pair), which only classify_fast_kernel stages without the general kernel's help
  // (evidence mode: never -- that kernel and anchor_verdict_kernel decide without a read's final coverage and k-mer count; the batch
  //  takes the evidence instantiation of classify_fast_kernel, and none of the passes in front of the table kernels is made;
  //  candidates mode: the same route for the same reason, through the candidates instantiation)
  const bool table_kernel = uni_kernel_available(ctx) && n != 0 && groups_fit && !s.evidence && !s.cand_m;
  // a batch of mixed lengths on an index whose uniform batches take the exact table in LDS: sorted by the pairs' two lengths on
  // the device and classified class by class (classify_uni_kernel's CLS instantiation) -- when the classes are few enough for
  // the histogram (the caller's bound on the read length says) and, the device decides, full enough; also when the host knows
  // the batch is ragged: it has not counted
  // ((l1, l2) tables -- the classes' counters, the ragged instantiation's plans -- are sized by the caller's bound on the read length,
  //  2^20 entries at most and when there is no bound or a loose one; the device checks the batch's longest mates against them)
  const uint64_t hint_classes = uni_L1 ? ((uint64_t)uni_L1 + 1) * ((uint64_t)(b->seq2 ? uni_L2 : 0) + 1) : 0;
  const uint64_t classes = table_kernel ? std::min<uint64_t>(hint_classes ? hint_classes : (1ull << 20), 1ull << 20) : 0;
  // (a batch only the device can judge, in a stream whose last batch was uniform -- a sequencer's output --: the four launches of
  //  this path are left out, 2 % of such a batch; should it be ragged after all, the ragged instantiation takes it, and the next one
  //  comes here again)
  const bool stream_is_uniform = uni_mode == UNI_ASK_DEVICE && ctx->last_verdict == 2u && !ctx->env_cls_always;
  bool by_classes = table_kernel && uni_mode != UNI_YES && class_kernel_available(ctx, max_slots) && n < (1ull << 31) && ctx->env_cls_min_fill != 0 &&
                    !stream_is_uniform;
  // read plans of a ragged batch, indexed by (l1, l2) up to the longest mates (uni_L1 / uni_L2: known, or the caller's bound for
  // a resident batch; no bound, or a loose one: 2^20 entries, of which the batch's own longest mates decide how many are used).
  // Cleared per launch, filled by the kernel.
  // ... or, where it exists and the longest mates fit its layout, through the three-pairs kernel by offsets (TRO): no sorting.  A host
  // batch known to be ragged (UNI_NO: uni_L1 / uni_L2 are its longest mates) takes it instead of the ragged instantiation; for a batch
  // only the device can judge it is launched beside the others and uniform_check_kernel's verdict 3 picks it
  const bool tro_avail = table_kernel && uni_mode != UNI_YES && offsets_kernel_available(ctx, max_slots, ctx->q8 != 0) && n < (1ull << 31);
  const bool tro_host = tro_avail && uni_mode == UNI_NO && offsets_kernel_fits(ctx, max_slots, uni_L1, b->seq2 ? uni_L2 : 0u);
  const bool tro_ask = tro_avail && uni_mode == UNI_ASK_DEVICE;
  if (tro_host) by_classes = false;
  const bool with_plans = table_kernel && uni_mode != UNI_YES;
  // Speculation.  A sequencer's stream has one length per mate, batch after batch: behind a batch that the device judged uniform with
  // lengths (L1, L2), shk_classify_device launches the uniform kernel for THOSE lengths at once, as if the host knew them, and
  // uniform_check_kernel looks at this batch's offsets beside it on a stream of its own: nothing the kernel computes depends on the
  // check when the lengths are what they were.  No offsets form, no ragged form, no plan-table fill.  The launch is marked
  // (ClassifyParams::spec): the kernel returns at once unless the batch's first and last offsets are those of such a batch, so it reads
  // nothing that the batch's own offsets do not claim.  The tail waits for the check; the scan's epilogue compares the check's words
  // with the lengths assumed and, where they differ, counts nothing and raises CTR_SPEC_MISS: classify_resident runs the batch again.
  // Only where all of this holds: shk_classify_device with a length bound that fits (no host round trip in this function), lengths for
  // the device to judge, an index of one record without wrap whose uniform batches take the exact table in LDS and whose tail is the
  // scan's own, no record mode and no accumulating state, a batch before of the same pairedness, presence of qualities and
  // specialisation.  SHK_NO_SPECULATE=1: never
  const Ctx::SpecPrev &sp = ctx->spec_prev;
  const bool modes_on = s.evidence || s.cand_m || s.placement || s.seg_m || s.depth || s.sp_depth || s.sp_junc || s.pileup || s.pileup_al || s.align || s.indels;
  const bool spec = may_speculate && !ctx->env_no_speculate && stream_is_uniform && sp.valid && long_mode == LONG_NONE_EXPECTED && table_kernel &&
                    ctx->n_records == 1 && !ctx->idx.wrap && !ctx->env_plain_tail && class_kernel_available(ctx, max_slots) && !modes_on &&
                    sp.paired == (b->seq2 != nullptr) && sp.quals == (b->qual1 != nullptr) && sp.max_slots == max_slots;
  s.speculated = spec;
  if (by_classes) {
    // (32 bytes per pair of extra HBM: a device too full for them classifies the batch with the ragged instantiation instead)
    if (s.d_cls_entries.reserve(ctx, (size_t)(2 * n)) != SHK_OK ||
        s.d_cls_list.reserve(ctx, (size_t)classes) != SHK_OK ||
        s.d_cls_hist.reserve(ctx, (size_t)(2 * classes)) != SHK_OK ||
        (!s.d_cls_share && hipMalloc((void **)&s.d_cls_share, CLS_SHARES * sizeof(uint32_t)) != hipSuccess)) {
      (void)hipGetLastError();
      ctx->last_error.clear();
      by_classes = false;
    }
  }
  if (by_classes) {
    s.p.cls_entries = s.d_cls_entries.p;
    s.p.cls_list = s.d_cls_list.p;
    s.p.cls_share_first = s.d_cls_share;
    s.p.cls_hist = s.d_cls_hist.p;
    s.p.cls_cap = (uint32_t)classes;
    s.p.cls_min_fill = ctx->env_cls_min_fill;
  }
  if (with_plans) {
    if ((rc = s.d_plan.reserve(ctx, (size_t)classes))) return rc;
    s.p.plan_tab = s.d_plan.p;
    s.p.plan_cap = (uint32_t)classes;
  }
  if (!table_kernel) {
    uni_mode = UNI_NO;
    SHK_HIP(ctx, hipMemsetAsync(s.d_count.p + n, 0, sizeof(uint32_t), st));
  } else {
    // classify_uni_kernel writes count[] only for reads with associations
    SHK_HIP(ctx, hipMemsetAsync(s.d_count.p, 0, (n + 1) * sizeof(uint32_t), st));
  }
  // timed: the classify launches (shk_timing::total_ms) and, for a batch the device has to look at first, the passes over its
  // offsets in front of them (prepass_ms)
  hipEvent_t e0 = nullptr, e1 = nullptr;
  if (ctx->timing) {
    if (ctx->ev_used == ctx->ev_start.size()) {
      hipEvent_t a, c, d;
      SHK_HIP(ctx, hipEventCreate(&a));
      SHK_HIP(ctx, hipEventCreate(&c));
      SHK_HIP(ctx, hipEventCreate(&d));
      ctx->ev_start.push_back(a);
      ctx->ev_stop.push_back(c);
      ctx->ev_pre.push_back(d);
    }
    e0 = ctx->ev_start[ctx->ev_used];
    e1 = ctx->ev_stop[ctx->ev_used];
    SHK_HIP(ctx, hipEventRecord(ctx->ev_pre[ctx->ev_used], st));
    ctx->ev_used++;
  }
  if (table_kernel) {
    if (by_classes) {
      uni_mode = UNI_ASK_DEVICE;
      SHK_HIP(ctx, hipMemsetAsync(s.d_cls_hist.p, 0, classes * sizeof(uint32_t), st));
    }
    if (spec) {
      // (the check itself is launched with the classify kernel, below)
      s.p.tro = tro_ask ? (ctx->env_force_tro ? 2u : 1u) : 0u;
      // (the lengths as the host's: uni_flag stays nullptr until the launch is made)
      s.p.uni_L1 = sp.L1;
      s.p.uni_L2 = sp.L2;
      s.p.spec = 1u;
    } else if (uni_mode == UNI_ASK_DEVICE) {
      s.p.tro = tro_ask ? (ctx->env_force_tro ? 2u : 1u) : 0u;
      if ((rc = launch_uniform_check(s.p, s.fast_cap, s.d_uni_flag, st))) return rc;
      if (by_classes && (rc = launch_class_prepass(s.p, s.fast_cap, s.d_uni_flag, st))) return rc;
      s.p.uni_flag = s.d_uni_flag;
    } else {
      // the one length per mate (UNI_YES), or the longest mates: the ragged instantiation stages the batch in their layout
      s.p.uni_L1 = uni_L1;
      s.p.uni_L2 = uni_L2;
      // (a resident batch whose caller vouched for the lengths: nobody has looked at its offsets)
      if (uni_mode == UNI_YES && !s.host_batch && n != 0 && (rc = launch_vouch_check(s.p, uni_L1, uni_L2, s.d_counters, st))) return rc;
    }
    // (a speculated batch launches no reader of the plans; should it come through again, classify_resident clears them)
    if (with_plans && !spec) SHK_HIP(ctx, hipMemsetAsync(s.d_plan.p, 0, classes * sizeof(uint4), st));
  }
  if (ctx->timing) SHK_HIP(ctx, hipEventRecord(e0, st));

  // the timed launch is the one that does the work: the uniform kernel when the host knows it applies (or has to ask
  // the device: then the generic kernel is launched behind it and returns at once for a uniform batch)
  if (ctx->idx.wrap) {
    // more than 65 536 genes: lists carry multiplicities, which only the general kernel counts (classify.hip, WRAP); it
    // runs over all reads with the fast kernel's slot capacity and queues what does not fit, as the fast kernel would
    ClassifyParams p = s.p;
    unsigned n_waves = 0;
    if ((rc = size_scratch(ctx, p, s.fast_cap, n, &n_waves))) return rc;
    p.work = nullptr;
    p.n_work = n;
    p.work_count = nullptr;
    if ((rc = launch_classify_general(ctx, p, false, n_waves, st, s.evidence, s.cand_m != 0))) return rc;
    snprintf(ctx->last_kernel, sizeof(ctx->last_kernel), s.cand_m ? "classify_general_kernel<wrap, candidates>"
                                                                   : (s.evidence ? "classify_general_kernel<wrap, evidence>" : "classify_general_kernel<wrap>"));
  }
  if (!ctx->idx.wrap) {
    if (!table_kernel) {
      if ((rc = launch_classify_fast(ctx, s.p, max_slots, st, s.evidence, s.cand_m != 0))) return rc;           // bit-vector probe chains; every index in evidence mode
    } else if (spec) {
      // the check beside the classify kernel, on the context's second stream: behind the fills of the counter / flag words, and nobody
      // waits for it before the tail.  Then the uniform launch alone, exactly the form that applies to the speculated lengths; then the
      // check's words are awaited and the tail reports the device's verdict as ever.  An error on the way: the check may be running
      // -- it reads the caller's offsets and writes the flag words --, so the second stream is drained before the error is returned
      // (SHK_SPECULATE_IN_FRONT=1, A/B timing: the check in front of the launch on the one stream, as without speculation; the launches
      //  that are left out stay out)
      hipError_t e = hipSuccess;
      if (ctx->env_spec_in_front) {
        rc = launch_uniform_check(s.p, s.fast_cap, s.d_uni_flag, st);
        if (!rc) rc = launch_classify_uni(ctx, s.p, max_slots, 1, st);
      } else {
        e = hipEventRecord(ctx->ev_chk_go, st);
        if (e == hipSuccess) e = hipStreamWaitEvent(ctx->chk_stream, ctx->ev_chk_go, 0);
        rc = e == hipSuccess ? launch_uniform_check(s.p, s.fast_cap, s.d_uni_flag, ctx->chk_stream, true) : set_hip_error(ctx, e, "the check's start event");
        if (!rc && (e = hipEventRecord(ctx->ev_chk_done, ctx->chk_stream)) != hipSuccess) rc = set_hip_error(ctx, e, "hipEventRecord(ctx->ev_chk_done, ctx->chk_stream)");
        if (!rc) rc = launch_classify_uni(ctx, s.p, max_slots, 1, st);
        if (!rc && (e = hipStreamWaitEvent(st, ctx->ev_chk_done, 0)) != hipSuccess) rc = set_hip_error(ctx, e, "hipStreamWaitEvent(st, ctx->ev_chk_done, 0)");
      }
      if (rc) {
        (void)hipStreamSynchronize(ctx->chk_stream);
        return rc;
      }
      s.p.uni_flag = s.d_uni_flag;
    } else {
      // what the host knows decides the launch; when only the device knows, both are made and one returns at once
      if (uni_mode != UNI_NO && (rc = launch_classify_uni(ctx, s.p, max_slots, 1, st))) return rc;
      if ((tro_host || tro_ask) && (rc = launch_classify_uni(ctx, s.p, max_slots, 3, st))) return rc;
      if (by_classes && (rc = launch_classify_uni(ctx, s.p, max_slots, 2, st))) return rc;
      if (uni_mode != UNI_YES && !tro_host && (rc = launch_classify_uni(ctx, s.p, max_slots, 0, st))) return rc;
    }
  }
  if (ctx->timing) SHK_HIP(ctx, hipEventRecord(e1, st));

  uint32_t n_long = 0;
  if (long_mode == LONG_UNKNOWN) {
    if ((rc = launch_publish_results(s.d_counters, s.h_counters, nullptr, nullptr, 0, nullptr, nullptr, 0, s.p.uni_flag, st))) return rc;
    SHK_HIP(ctx, hipStreamSynchronize(st));
    n_long = s.h_counters[CTR_LONG];
    s.gen_slots = std::max(s.fast_cap, s.h_counters[CTR_MAX_SLOTS]);
  } else if (long_mode == LONG_KNOWN) {
    n_long = n_long_host;
    s.gen_slots = std::max(s.fast_cap, long_slots_host);
  }
  if ((rc = run_long_reads(ctx, s, n_long))) return rc;
  return enqueue_tail(ctx, s, long_mode == LONG_NONE_EXPECTED, count_genes);
}

// after ev_done: complete what the enqueued work could not (both paths are rare and synchronous)
//  * a length bound that did not hold: reads sit in the long queue -> general kernel, tail again
//  * more associations than gene_ids holds -> grow it, tail again
// The histogram kernel skipped itself in exactly these cases, so no batch is counted twice.
static int finish_classify(Ctx *ctx, Slot &s, bool long_was_speculative, bool count_genes, bool *redone)
{
  hipStream_t st = ctx->stream;
  int rc;
  *redone = false;
  if (long_was_speculative && s.h_counters[CTR_LONG]) {
    s.gen_slots = std::max(s.fast_cap, s.h_counters[CTR_MAX_SLOTS]);
    if ((rc = run_long_reads(ctx, s, s.h_counters[CTR_LONG]))) return rc;
    if ((rc = enqueue_tail(ctx, s, false, count_genes))) return rc;
    SHK_HIP(ctx, hipStreamSynchronize(st));
    *redone = true;
  }
  if (s.h_counters[CTR_OVERFLOW]) {
    const uint64_t n_assoc = ((uint64_t)s.h_counters[CTR_ASSOC_HI] << 32) | s.h_counters[CTR_ASSOC_LO];
    if (n_assoc >= 0xFFFFFFFFull) { ctx->last_error = "more than 2^32-1 associations in one batch"; return SHK_ERR_ARG; }
    SHK_HIP(ctx, hipStreamSynchronize(st));     // gene_ids is about to be replaced
    if ((rc = s.d_gene_ids.reserve(ctx, n_assoc + 8))) return rc;
    if ((rc = enqueue_tail(ctx, s, false, count_genes))) return rc;
    SHK_HIP(ctx, hipStreamSynchronize(st));
    *redone = true;
  }
  return SHK_OK;
}

// The records of the batch in `s`, whose result is being handed out, become the context's last records (shk_*_last).  host: the pinned
// mirrors (a host batch), else the device arrays; measurement: no kind is valid.  A host batch with more associations than a kind's mirror
// holds was not published whole: the kinds in front of that one are valid, it and all behind it are not
static int hand_out_records(Ctx *ctx, const Slot &s, bool host, bool measurement, uint64_t n_assoc)
{
  LastRecords &l = ctx->last_rec;
  const bool on = !measurement;
  l.n = s.n;
  l.n_assoc = n_assoc;
  l.evid_valid = s.evidence && on;
  l.evid = s.rec_evid.handed(host);
  l.cand_valid = s.cand_m != 0 && on;
  l.cand_m = s.cand_m;
  l.cand_reads = s.rec_cand_reads.handed(host);
  l.cand_entries = s.rec_cand_entries.handed(host);
  if (s.placement && host && n_assoc > s.rec_place.h.cap) { ctx->last_error = "placement publication failed"; return SHK_ERR_HIP; }
  l.place_valid = s.placement && on;
  l.place = s.rec_place.handed(host);
  if (s.seg_m && host && n_assoc > segments_cap(s.rec_seg_keys.h, s.rec_seg_entries.h, s.seg_m)) { ctx->last_error = "segments publication failed"; return SHK_ERR_HIP; }
  l.seg_valid = s.seg_m != 0 && on;
  l.seg_m = s.seg_m;
  l.seg_keys = s.rec_seg_keys.handed(host);
  l.seg_entries = s.rec_seg_entries.handed(host);
  if (s.align && host && n_assoc > s.rec_align.h.cap / 2) { ctx->last_error = "alignments publication failed"; return SHK_ERR_HIP; }
  l.align_valid = s.align != 0 && on;
  l.align = s.rec_align.handed(host);
  if (s.pairs && host && n_assoc > s.rec_pairs.h.cap) { ctx->last_error = "pairs publication failed"; return SHK_ERR_HIP; }
  l.pairs_valid = s.pairs != 0 && on;
  l.pairs = s.rec_pairs.handed(host);
  if (s.rescue && host && n_assoc > s.rec_rescue.h.cap) { ctx->last_error = "rescue publication failed"; return SHK_ERR_HIP; }
  l.rescue_valid = s.rescue != 0 && on;
  l.rescue = s.rec_rescue.handed(host);
  return SHK_OK;
}

// A speculated batch whose offsets were not what its classify launch assumed (CTR_SPEC_MISS; enqueue_classify): the launch returned from
// its prologue or classified reads cut at the wrong places, and the scan counted nothing.  The batch comes through again: the counters and
// count[] cleared, the plans cleared, then exactly the launches the path without speculation makes behind the check -- whose verdict is
// where it was, and which is not repeated --, the tail, a synchronisation.  The result is that of the kernels that path would have run,
// and the batch is counted here, once; finish_classify's slow paths follow as behind any batch
static int redo_speculated(Ctx *ctx, Slot &s, uint32_t max_slots, bool count_genes)
{
  hipStream_t st = ctx->stream;
  int rc;
  s.speculated = false;
  s.p.spec = 0u;
  s.p.uni_L1 = s.p.uni_L2 = 0u;
  s.p.uni_flag = s.d_uni_flag;
  SHK_HIP(ctx, hipMemsetAsync(s.d_counters, 0, COUNTER_BLOCK_WORDS * sizeof(uint32_t), st));   // (the check's words behind them stay)
  SHK_HIP(ctx, hipMemsetAsync(s.d_count.p, 0, (s.n + 1) * sizeof(uint32_t), st));
  if (s.p.plan_tab) SHK_HIP(ctx, hipMemsetAsync(s.p.plan_tab, 0, (size_t)s.p.plan_cap * sizeof(uint4), st));
  if ((rc = launch_classify_uni(ctx, s.p, max_slots, 1, st))) return rc;
  if (s.p.tro && (rc = launch_classify_uni(ctx, s.p, max_slots, 3, st))) return rc;
  if ((rc = launch_classify_uni(ctx, s.p, max_slots, 0, st))) return rc;
  if ((rc = enqueue_tail(ctx, s, true, count_genes))) return rc;
  SHK_HIP(ctx, hipStreamSynchronize(st));
  return SHK_OK;
}

// a batch resident in HBM, start to finish (shk_classify_device, shk_count_work)
static int classify_resident(Ctx *ctx, const shk_batch *b, uint32_t max_read_len, shk_result *res, shk_work_counters *wc = nullptr)
{
  hipStream_t st = ctx->stream;
  Slot &s = ctx->slots[PIPE_DEPTH];
  const uint64_t n = b->n;
  ctx->last_rec = LastRecords{};   // (until this batch's result is handed out)
  if (n >= 0xFFFFFFFFull) { ctx->last_error = "batch too large (n must be < 2^32-1)"; return SHK_ERR_ARG; }
  const bool paired = b->seq2 != nullptr;
  const uint32_t max_slots = max_read_len ? slots_for_len(max_read_len, ctx->prm.k, paired) : 0;
  const int long_mode = (max_read_len && max_slots <= fast_kernel_max_slots()) ? LONG_NONE_EXPECTED : LONG_UNKNOWN;
  int rc;
  const uint64_t hint_groups = (((uint64_t)max_read_len + 7) >> 3) * (paired ? 2 : 1);   // (no bound given: the table kernel queues what it cannot stage)
  // (UNI_ASK_DEVICE: the lengths passed here only size the plan table of a batch that turns out ragged: the caller's bound per mate)
  if ((rc = enqueue_classify(ctx, s, b, max_slots, long_mode, 0, 0, wc == nullptr, UNI_ASK_DEVICE, max_read_len, paired ? max_read_len : 0,
                             hint_groups <= uni_kernel_max_groups(max_slots), wc == nullptr)))
    return rc;
  SHK_HIP(ctx, hipStreamSynchronize(st));
  int speculation = s.speculated ? 1 : 0;
  if (s.speculated && s.h_counters[CTR_SPEC_MISS]) {
    if ((rc = redo_speculated(ctx, s, max_slots, wc == nullptr))) return rc;
    speculation = 2;
  }
  bool redone = false;
  // (behind a batch that was run again too.  Of the two slow paths only the long reads' can follow a missed speculation today: speculation
  //  needs an index of one record, where a read has at most one association and gene_ids holds 2 n + 4 096 -- CTR_OVERFLOW is never
  //  raised there, so "missed, then overflow" is a sequence no test can drive; tests/test_gpu_speculative_uniform.py drives "missed,
  //  then long reads")
  if ((rc = finish_classify(ctx, s, long_mode == LONG_NONE_EXPECTED, wc == nullptr, &redone))) return rc;
  const uint64_t n_assoc = ((uint64_t)s.h_counters[CTR_ASSOC_HI] << 32) | s.h_counters[CTR_ASSOC_LO];

  if (wc) {
    // measurement only: re-run every read through the general kernel with the
    // exact work counters switched on (results are rewritten with equal values)
    ClassifyParams p = s.p;
    unsigned n_waves = 0;
    if ((rc = size_scratch(ctx, p, s.gen_slots, n, &n_waves))) return rc;
    SHK_HIP(ctx, hipMemsetAsync(s.d_counters, 0, CTR_WORDS * sizeof(uint32_t), st));
    SHK_HIP(ctx, hipMemsetAsync(ctx->d_work_counters, 0, 4 * sizeof(unsigned long long), st));
    p.work = nullptr;
    p.n_work = n;
    p.work_count = nullptr;
    p.work_counters = ctx->d_work_counters;
    if ((rc = launch_classify_general(ctx, p, false, n_waves, st))) return rc;
    unsigned long long h[4] = {0, 0, 0, 0};
    SHK_HIP(ctx, hipMemcpyAsync(h, ctx->d_work_counters, sizeof(h), hipMemcpyDeviceToHost, st));
    SHK_HIP(ctx, hipStreamSynchronize(st));
    wc->n_kmers = h[0]; wc->n_hits = h[1]; wc->n_list_ids = h[2]; wc->n_bases = h[3];
  }

  ctx->last.last_n_reads = n;
  ctx->last.last_n_long = s.h_counters[CTR_LONG];
  ctx->last.last_n_tie = s.h_counters[CTR_TIE];
  note_verdict(ctx, s.h_counters[CTR_VERDICT]);
  // (what the next batch of shk_classify_device may speculate on: the device's own "uniform", with the lengths it found)
  if (!wc && s.h_counters[CTR_VERDICT] == 2u)
    ctx->spec_prev = Ctx::SpecPrev{true, paired, b->qual1 != nullptr, max_slots, s.h_counters[CTR_UNI_L1], s.h_counters[CTR_UNI_L2]};
  ctx->last_speculation = speculation;
#ifdef SHK_ANCH_STATS   // (experiments: reads the anchored extension settled early / settled after probing its open slots)
  ctx->last.last_n_long = s.h_counters[CTR_UNUSED3];
  ctx->last.last_n_tie = s.h_counters[CTR_UNUSED5];
#endif
  ctx->last.last_n_assoc = n_assoc;
  res->n = n;
  res->gene_off = s.d_gene_off.p;
  res->gene_ids = s.d_gene_ids.p;
  res->n_assoc = n_assoc;
  // (shk_count_work is a measurement, not one of the calls that hand out records: none is left behind it)
  return hand_out_records(ctx, s, false, wc != nullptr, n_assoc);
}

}  // namespace shk

// ---- RCCL, loaded on first use so that single-GPU users never pay for (or conflict over) it ----
namespace shk {
typedef void *rccl_comm_t;
struct rccl_uid { char internal[128]; };   // ncclUniqueId
struct RcclApi {
  void *lib = nullptr;
  int (*CommInitAll)(rccl_comm_t *, int, const int *) = nullptr;
  int (*CommInitRank)(rccl_comm_t *, int, rccl_uid, int) = nullptr;
  int (*GetUniqueId)(rccl_uid *) = nullptr;
  int (*CommDestroy)(rccl_comm_t) = nullptr;
  int (*CommCount)(rccl_comm_t, int *) = nullptr;
  int (*CommUserRank)(rccl_comm_t, int *) = nullptr;
  int (*AllReduce)(const void *, void *, size_t, int, int, rccl_comm_t, hipStream_t) = nullptr;
  int (*GroupStart)() = nullptr;
  int (*GroupEnd)() = nullptr;
  bool ok = false;
};
static RcclApi &rccl()
{
  static RcclApi api;
  if (!api.lib) {
    api.lib = dlopen("librccl.so.1", RTLD_NOW | RTLD_LOCAL);
    if (!api.lib) api.lib = dlopen("librccl.so", RTLD_NOW | RTLD_LOCAL);
    if (api.lib) {
      api.CommInitAll = (int (*)(rccl_comm_t *, int, const int *))dlsym(api.lib, "ncclCommInitAll");
      api.CommInitRank = (int (*)(rccl_comm_t *, int, rccl_uid, int))dlsym(api.lib, "ncclCommInitRank");
      api.GetUniqueId = (int (*)(rccl_uid *))dlsym(api.lib, "ncclGetUniqueId");
      api.CommDestroy = (int (*)(rccl_comm_t))dlsym(api.lib, "ncclCommDestroy");
      api.CommCount = (int (*)(rccl_comm_t, int *))dlsym(api.lib, "ncclCommCount");
      api.CommUserRank = (int (*)(rccl_comm_t, int *))dlsym(api.lib, "ncclCommUserRank");
      api.AllReduce = (int (*)(const void *, void *, size_t, int, int, rccl_comm_t, hipStream_t))dlsym(api.lib, "ncclAllReduce");
      api.GroupStart = (int (*)())dlsym(api.lib, "ncclGroupStart");
      api.GroupEnd = (int (*)())dlsym(api.lib, "ncclGroupEnd");
      api.ok = api.CommInitAll && api.CommInitRank && api.GetUniqueId && api.CommDestroy && api.CommCount && api.CommUserRank && api.AllReduce &&
               api.GroupStart && api.GroupEnd;
    }
  }
  return api;
}

// RCCL may print a version banner on stdout when it initialises; stdout is the ssv stream of the CLI
// (ReadOutput.hpp:43), so anything RCCL prints during init is sent to stderr instead
template <typename F>
static int with_stdout_on_stderr(F f)
{
  fflush(stdout);
  const int saved_stdout = dup(1);
  if (saved_stdout >= 0) (void)dup2(2, 1);
  const int rc = f();
  if (saved_stdout >= 0) {
    fflush(stdout);
    (void)dup2(saved_stdout, 1);
    close(saved_stdout);
  }
  return rc;
}

static void dist_release(Ctx *ctx)
{
  if (ctx->dist_comm) { (void)rccl().CommDestroy(ctx->dist_comm); ctx->dist_comm = nullptr; }
  if (ctx->group_comm) { (void)rccl().CommDestroy(ctx->group_comm); ctx->group_comm = nullptr; }
}
}  // namespace shk

using namespace shk;

// a state whose shape its caller chooses (the junction table's capacity, the fragments state's n_bins), asked for at `entries` entries.  Missing:
// allocated and cleared.  Of another shape: refused while dirty, otherwise released behind the drained stream, then allocated and cleared
template <typename T, typename Clear>
static int state_shape(shk_ctx *ctx, DevArray<T> &arr, size_t entries, bool &dirty, const char *refusal, Clear clear)
{
  if (arr.p && arr.cap != entries) {
    if (dirty) { ctx->last_error = refusal; return SHK_ERR_ARG; }
    SHK_HIP(ctx, hipSetDevice(ctx->prm.device));
    SHK_HIP(ctx, hipStreamSynchronize(ctx->stream));
    (void)arr.release();
  }
  if (arr.p) return SHK_OK;
  SHK_HIP(ctx, hipSetDevice(ctx->prm.device));
  if (const int rc = arr.alloc_exact(ctx, entries)) return rc;
  dirty = false;
  return clear();
}

extern "C" {

const char *shk_version(void) { return "sharkhip 0.1 (gfx950)"; }

const char *shk_strerror(int code)
{
  switch (code) {
  case SHK_OK: return "ok";
  case SHK_ERR_ARG: return "invalid argument";
  case SHK_ERR_STATE: return "call not allowed in the current mode";
  case SHK_ERR_HIP: return "HIP runtime error";
  case SHK_ERR_NOMEM: return "out of memory";
  case SHK_ERR_TOO_MANY_GENES: return "more than 65536 reference sequences";
  case SHK_ERR_INDEX_TOO_LARGE: return "index exceeds the reference's 2^31 limits";
  case SHK_ERR_NO_DEVICE: return "no HIP device";
  default: return "unknown error";
  }
}

const char *shk_last_error(const shk_ctx *ctx) { return ctx ? ctx->last_error.c_str() : ""; }

int shk_create(const shk_params *prm, shk_ctx **out)
{
  if (!prm || !out) return SHK_ERR_ARG;
  *out = nullptr;
  if (prm->k == 0 || prm->k > 31) return SHK_ERR_ARG;                  // argument_parser.hpp:115
  if (!(prm->c >= 0.0 && prm->c <= 1.0)) return SHK_ERR_ARG;           // :124
  if (prm->min_quality < 0) return SHK_ERR_ARG;                        // :138
  if (prm->bf_bits == 0) return SHK_ERR_ARG;
  int n_dev = 0;
  {
    // the first HIP call of a process brings the runtime up (tens of milliseconds).  N workers created on N threads (shark --gpus N) all
    // arrive here at once: behind one mutex the first of them initialises the runtime and the others sleep -- racing into the runtime's
    // own initialisation they took three times as long together (measured: "contexts created" 0.22 s for two workers against 0.10 s)
    static std::mutex init_m;
    std::lock_guard<std::mutex> l(init_m);
    if (hipGetDeviceCount(&n_dev) != hipSuccess || n_dev <= 0) return SHK_ERR_NO_DEVICE;
  }
  if (prm->device < 0 || prm->device >= n_dev) return SHK_ERR_ARG;
  shk_ctx *ctx = new (std::nothrow) shk_ctx();
  if (!ctx) return SHK_ERR_NOMEM;
  ctx->prm = *prm;
  ctx->prm.single = prm->single ? 1 : 0;
  ctx->q8 = (int8_t)(uint8_t)(prm->min_quality & 0xFF);                // static_cast<char>(mq), argument_parser.hpp:144
  {
    const char *e = getenv("SHK_FORCE_GENERIC");
    ctx->env_force_generic = e && e[0] == '1';
    ctx->env_big_lds_always = getenv("SHK_BIG_LDS_ALWAYS") != nullptr;
    { const char *nt = getenv("SHK_KTAB_NT"); ctx->env_ktab_nt = nt && nt[0] == '1'; ctx->env_ktab_plain = nt && nt[0] == '0'; }
    ctx->env_ktab_always = getenv("SHK_KTAB") != nullptr;
    ctx->env_anchor_always = getenv("SHK_ANCHOR_ALWAYS") != nullptr;
    ctx->env_no_pre_verdict = getenv("SHK_NO_PRE_VERDICT") != nullptr;
    ctx->env_no_tri = getenv("SHK_NO_TRI") != nullptr;
    { const char *pt = getenv("SHK_PLAIN_TAIL"); ctx->env_plain_tail = pt && pt[0] == '1'; }
    { const char *ns = getenv("SHK_NO_SPECULATE"); ctx->env_no_speculate = ns && ns[0] == '1'; }
    { const char *sf = getenv("SHK_SPECULATE_IN_FRONT"); ctx->env_spec_in_front = sf && sf[0] == '1'; }
    ctx->env_pairs_global = getenv("SHK_PAIRS_GLOBAL_ATOMICS") != nullptr;
    ctx->env_no_tro = getenv("SHK_NO_TRO") != nullptr;
    ctx->env_force_tro = getenv("SHK_FORCE_TRO") != nullptr;
    ctx->env_tile_first = getenv("SHK_TILE_FIRST") ? (getenv("SHK_TILE_FIRST")[0] == '0' ? -1 : 1) : 0;
    if (const char *f = getenv("SHK_CLS_MIN_FILL")) { ctx->env_cls_min_fill = (uint32_t)strtoul(f, nullptr, 10); ctx->env_cls_always = true; }
  }
  auto fail = [&](int rc) { shk_destroy(ctx); return rc; };
  // (SHK_TRACE_CREATE=1: where the time of this call goes, on stderr -- tools/workers_start.py)
  const bool trace = getenv("SHK_TRACE_CREATE") != nullptr;
  const auto t_start = std::chrono::steady_clock::now();
  auto stamp = [&](const char *what) {
    if (trace) fprintf(stderr, "[shk/create dev %d ctx %p] %-28s %8.3f ms\n", prm->device, (void *)ctx, what,
                       std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_start).count());
  };
  stamp("device count");
#define CR_HIP(call) do { hipError_t e__ = (call); if (e__ != hipSuccess) return fail(e__ == hipErrorOutOfMemory ? SHK_ERR_NOMEM : SHK_ERR_HIP); } while (0)
  CR_HIP(hipSetDevice(prm->device));
  stamp("hipSetDevice");
  CR_HIP(hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking));
  CR_HIP(hipStreamCreateWithFlags(&ctx->h2d_stream, hipStreamNonBlocking));
  CR_HIP(hipStreamCreateWithFlags(&ctx->d2h_stream, hipStreamNonBlocking));
  // (and the one a speculated batch's check runs on, beside the classify kernel: enqueue_classify)
  CR_HIP(hipStreamCreateWithFlags(&ctx->chk_stream, hipStreamNonBlocking));
  CR_HIP(hipEventCreateWithFlags(&ctx->ev_chk_go, hipEventDisableTiming));
  CR_HIP(hipEventCreateWithFlags(&ctx->ev_chk_done, hipEventDisableTiming));
  stamp("three streams");
  DeviceIndex &ix = ctx->idx;
  ix.bf_bits = prm->bf_bits;
  ix.pow2 = (prm->bf_bits & (prm->bf_bits - 1)) == 0;
  ix.bf_words64 = ((prm->bf_bits + 511) / 512) * 8;
  // BF::BF(size): size zero bits (bloomfilter.h:48-53)
  CR_HIP(hipMalloc((void **)&ix.bf64, ix.bf_words64 * sizeof(uint64_t)));
  stamp("filter allocated");
  CR_HIP(hipMemsetAsync(ix.bf64, 0, ix.bf_words64 * sizeof(uint64_t), ctx->stream));
  stamp("filter clear enqueued");
  for (Slot &sl : ctx->slots)
    if (slot_init(ctx, sl) != SHK_OK) return fail(SHK_ERR_HIP);
  stamp("slots");
  CR_HIP(hipMalloc((void **)&ctx->d_gene_counts, 65536 * sizeof(unsigned long long)));
  CR_HIP(hipMemsetAsync(ctx->d_gene_counts, 0, 65536 * sizeof(unsigned long long), ctx->stream));
  CR_HIP(hipMalloc((void **)&ctx->d_gene_totals, 65536 * sizeof(unsigned long long)));
  CR_HIP(hipMalloc((void **)&ctx->d_work_counters, 4 * sizeof(unsigned long long)));
  stamp("counters");
  CR_HIP(hipStreamSynchronize(ctx->stream));
  stamp("synchronised");
#undef CR_HIP
  *out = ctx;
  return SHK_OK;
}

void shk_destroy(shk_ctx *ctx)
{
  if (!ctx) return;
  (void)hipSetDevice(ctx->prm.device);
  // tickets that were submitted and never waited for (a caller bailing out) may still have copies in flight on the copy
  // streams -- into slot buffers that are about to be freed, out of caller memory that may be released right after this call
  if (ctx->h2d_stream) (void)hipStreamSynchronize(ctx->h2d_stream);
  if (ctx->d2h_stream) (void)hipStreamSynchronize(ctx->d2h_stream);
  if (ctx->stream) (void)hipStreamSynchronize(ctx->stream);
  if (ctx->chk_stream) (void)hipStreamSynchronize(ctx->chk_stream);
  free_index(ctx->idx);
  for (Slot &sl : ctx->slots) slot_free(sl);
  hipFree(ctx->d_gene_counts); hipFree(ctx->d_gene_totals); hipFree(ctx->d_work_counters);
  dist_release(ctx);
  for (auto e : ctx->ev_start) (void)hipEventDestroy(e);
  for (auto e : ctx->ev_stop) (void)hipEventDestroy(e);
  for (auto e : ctx->ev_pre) (void)hipEventDestroy(e);
  if (ctx->h2d_stream) (void)hipStreamDestroy(ctx->h2d_stream);
  if (ctx->d2h_stream) (void)hipStreamDestroy(ctx->d2h_stream);
  if (ctx->stream) (void)hipStreamDestroy(ctx->stream);
  if (ctx->ev_chk_go) (void)hipEventDestroy(ctx->ev_chk_go);
  if (ctx->ev_chk_done) (void)hipEventDestroy(ctx->ev_chk_done);
  if (ctx->chk_stream) (void)hipStreamDestroy(ctx->chk_stream);
  delete ctx;   // (the general kernel's scratch and the accumulated states free themselves here: the device is current, the streams were drained)
}

int shk_ref_add(shk_ctx *ctx, const char *seq, uint64_t len)
{
  if (!ctx || (!seq && len)) return SHK_ERR_ARG;
  if (ctx->mode != 0) return SHK_ERR_STATE;
  if (ctx->n_records >= 0x7FFFFFFFull) return SHK_ERR_TOO_MANY_GENES;
  try {
    ctx->ref_bytes.insert(ctx->ref_bytes.end(), seq, seq + len);
    ctx->ref_off.push_back(ctx->ref_bytes.size());
  } catch (...) {
    return SHK_ERR_NOMEM;
  }
  ctx->n_records++;
  return SHK_OK;
}

int shk_ref_finalize(shk_ctx *ctx)
{
  if (!ctx) return SHK_ERR_ARG;
  if (ctx->mode != 0) return SHK_ERR_STATE;
  SHK_HIP(ctx, hipSetDevice(ctx->prm.device));
  TraceRange tr("shk_ref_finalize: index build");
  const int rc = build_index(ctx);
  if (rc != SHK_OK) return rc;
  ctx->mode = 2;
  std::vector<char>().swap(ctx->ref_bytes);
  return SHK_OK;
}

int shk_index_info_get(const shk_ctx *ctx, shk_index_info *info)
{
  if (!ctx || !info) return SHK_ERR_ARG;
  info->n_records = ctx->n_records;
  info->nidx = ctx->nidx;
  info->bf_bits = ctx->idx.bf_bits;
  info->n_set_bits = ctx->idx.n_set;
  info->tot_idx = ctx->idx.tot_idx;
  info->n_ref_kmers = ctx->n_ref_kmers;
  return SHK_OK;
}

const char *shk_probe_mode(const shk_ctx *ctx)
{
  if (!ctx || ctx->mode != 2) return "";
  return probe_mode_name(ctx);
}

const char *shk_last_kernel(const shk_ctx *ctx) { return ctx ? ctx->last_kernel : ""; }
int shk_debug_last_speculation(const shk_ctx *ctx) { return ctx ? ctx->last_speculation : 0; }

int shk_index_copy_bf(const shk_ctx *cctx, uint64_t *words, uint64_t n_words)
{
  shk_ctx *ctx = const_cast<shk_ctx *>(cctx);
  if (!ctx || !words) return SHK_ERR_ARG;
  if (ctx->mode != 2) return SHK_ERR_STATE;
  const uint64_t have = (ctx->idx.bf_bits + 63) / 64;
  if (n_words > have) return SHK_ERR_ARG;
  SHK_HIP(ctx, hipSetDevice(ctx->prm.device));
  SHK_HIP(ctx, hipMemcpy(words, ctx->idx.bf64, n_words * sizeof(uint64_t), hipMemcpyDeviceToHost));
  return SHK_OK;
}

int shk_index_copy_lists(const shk_ctx *cctx, uint32_t *offsets, uint16_t *ids)
{
  shk_ctx *ctx = const_cast<shk_ctx *>(cctx);
  if (!ctx || !offsets) return SHK_ERR_ARG;
  if (ctx->mode != 2) return SHK_ERR_STATE;
  SHK_HIP(ctx, hipSetDevice(ctx->prm.device));
  std::vector<ListEntry> ent;
  try { ent.resize(ctx->idx.n_set + 1); } catch (...) { return SHK_ERR_NOMEM; }
  SHK_HIP(ctx, hipMemcpy(ent.data(), ctx->idx.ent, ent.size() * sizeof(ListEntry), hipMemcpyDeviceToHost));
  for (size_t r = 0; r < ent.size(); ++r) offsets[r] = ent[r].start;
  if (ctx->idx.tot_idx && ids)
    SHK_HIP(ctx, hipMemcpy(ids, ctx->idx.ids, ctx->idx.tot_idx * sizeof(uint16_t), hipMemcpyDeviceToHost));
  return SHK_OK;
}

// Test-only read-back of the derived index arrays (shark_internal.hpp, next to DeviceIndex); not declared in shark_hip.h.
int shk_debug_index_array(const shk_ctx *cctx, const char *name, void *dst, uint64_t dst_bytes, uint64_t *bytes_needed)
{
  shk_ctx *ctx = const_cast<shk_ctx *>(cctx);
  if (!ctx || !name || !bytes_needed) return SHK_ERR_ARG;
  if (ctx->mode != 2) return SHK_ERR_STATE;
  const DeviceIndex &ix = ctx->idx;
  const std::string what(name);
  const uint64_t slots = ix.tab_lg ? (2ull << ix.tab_lg) : 0;
  const uint64_t total = ix.ref_total;
  if (what == "meta") {
    const uint64_t meta[SHK_DEBUG_META_WORDS] = {ix.tab_lg, ix.sum_shift, ix.lsum_shift, ix.lbig_shift, ix.ltab ? ix.ltab_mul : 0, total, ix.n_set, ix.tot_idx,
                                                 ix.pow2 ? 1u : 0u, ix.wrap ? 1u : 0u, ix.ent_len, ix.ids_len, ix.bf_bits, ix.bf_words64, ix.sum_bits, ix.ktab_lg};
    *bytes_needed = sizeof(meta);
    if (!dst) return SHK_OK;
    if (dst_bytes < sizeof(meta)) return SHK_ERR_ARG;
    memcpy(dst, meta, sizeof(meta));
    return SHK_OK;
  }
  if (what == "kxmeta") {   // (the k-mer keyed table's scalars, on every index; a name of its own: `meta` keeps its 16 words)
    const uint64_t kxmeta[SHK_DEBUG_KXMETA_WORDS] = {ix.kxtab ? 1u : 0u, ix.kx_m1, ix.kx_m2, ix.kx_nkeys, ix.kx_enum_us, ix.kx_build_us};
    *bytes_needed = sizeof(kxmeta);
    if (!dst) return SHK_OK;
    if (dst_bytes < sizeof(kxmeta)) return SHK_ERR_ARG;
    memcpy(dst, kxmeta, sizeof(kxmeta));
    return SHK_OK;
  }
  if (what == "pmeta") {   // (a name of its own: `meta` keeps its 16 words)
    const uint64_t pmeta[SHK_DEBUG_PMETA_WORDS] = {ix.ptab_lg, ix.ptab_n};
    *bytes_needed = ix.ptab_lg ? sizeof(pmeta) : 0;
    if (!dst || !ix.ptab_lg) return SHK_OK;
    if (dst_bytes < sizeof(pmeta)) return SHK_ERR_ARG;
    memcpy(dst, pmeta, sizeof(pmeta));
    return SHK_OK;
  }
  if (what == "ktmeta") {   // (the minimiser-bucketed table's scalars, on every index; a name of its own: `meta` keeps its 16 words)
    const bool kt = ix.ktab && ix.ktab_lg;
    const uint64_t ktmeta[SHK_DEBUG_KTMETA_WORDS] = {kt ? ix.ktab_lg : 0u, kt ? ix.ktab_w : 0u, kt ? ix.ktab_keys : 0ull};
    *bytes_needed = sizeof(ktmeta);
    if (!dst) return SHK_OK;
    if (dst_bytes < sizeof(ktmeta)) return SHK_ERR_ARG;
    memcpy(dst, ktmeta, sizeof(ktmeta));
    return SHK_OK;
  }
  const void *src = nullptr;
  uint64_t bytes = 0;
  if (what == "rank_w") { src = ix.rank_w; bytes = (ix.bf_words64 + 2) * sizeof(uint32_t); }
  else if (what == "ent") { src = ix.ent; bytes = ix.ent_len * sizeof(ListEntry); }
  else if (what == "ids") { src = ix.ids; bytes = ix.ids_len * sizeof(uint16_t); }
  else if (what == "sum32") { src = ix.sum_shift ? ix.sum32 : nullptr; bytes = ((ix.sum_bits + 31) / 32 + 2) * sizeof(uint32_t); }
  else if (what == "lsum32") { src = ix.lsum_shift ? ix.lsum32 : nullptr; bytes = (LDS_SUM_BITS / 32 + 2) * sizeof(uint32_t); }
  else if (what == "lbig32") { src = ix.lbig_shift ? ix.lbig32 : nullptr; bytes = ((1u << 20) / 32 + 2) * sizeof(uint32_t); }
  else if (what == "tab") { src = slots ? ix.tab : nullptr; bytes = (slots + 2) * sizeof(uint64_t); }
  else if (what == "atab") { src = slots && total ? ix.atab : nullptr; bytes = (slots + 2) * sizeof(uint64_t); }
  else if (what == "ltab") { src = ix.ltab; bytes = LTAB_BYTES; }
  else if (what == "kxtab") { src = ix.kxtab; bytes = LTAB_BYTES; }
  else if (what == "kxkeys") { src = ix.kxtab ? ix.kxkeys : nullptr; bytes = ix.kx_nkeys * sizeof(uint64_t); }
  else if (what == "ktab") { src = ix.ktab_lg >= 3 ? ix.ktab : nullptr; bytes = src ? ((2ull << ix.ktab_lg) + 16) * sizeof(uint64_t) : 0; }   // (as allocated: the eight spare buckets included)
  else if (what == "ref2") { src = total ? ix.ref2 : nullptr; bytes = ((total + 15) / 16 + 4) * sizeof(uint32_t); }
  else if (what == "refpay") { src = total ? ix.refpay : nullptr; bytes = (total + 8) * sizeof(uint32_t); }
  else if (what == "refext") { src = total ? ix.refext : nullptr; bytes = (total + 8) * sizeof(uint32_t); }
  else if (what == "recbase") { src = ix.recbase; bytes = ix.recbase_bytes; }
  else if (what == "refmul") { src = total ? ix.refmul : nullptr; bytes = ((total + 31) / 32 + 2) * sizeof(uint32_t); }
  else if (what == "ptab") { src = ix.ptab_lg ? ix.ptab : nullptr; bytes = (ix.ptab_n + 1) * sizeof(uint4); }
  else if (what == "pdir") { src = ix.ptab_lg ? ix.pdir : nullptr; bytes = ((1ull << ix.ptab_lg) + 2) * sizeof(uint32_t); }
  else return SHK_ERR_ARG;
  if (!src) bytes = 0;
  *bytes_needed = bytes;
  if (!dst || bytes == 0) return SHK_OK;
  if (dst_bytes < bytes) return SHK_ERR_ARG;
  SHK_HIP(ctx, hipSetDevice(ctx->prm.device));
  SHK_HIP(ctx, hipMemcpy(dst, src, bytes, hipMemcpyDeviceToHost));
  return SHK_OK;
}

static int check_batch(const shk_ctx *ctx, const shk_batch *b)
{
  if (!b) return SHK_ERR_ARG;
  if (b->n == 0) return SHK_OK;
  if (!b->seq1 || !b->off1) return SHK_ERR_ARG;
  if ((b->seq2 == nullptr) != (b->off2 == nullptr)) return SHK_ERR_ARG;
  if (ctx->q8 != 0 && (!b->qual1 || (b->seq2 && !b->qual2))) return SHK_ERR_ARG;
  return SHK_OK;
}

int shk_classify_device(shk_ctx *ctx, const shk_batch *batch, uint32_t max_read_len, shk_result *result)
{
  if (!ctx || !result) return SHK_ERR_ARG;
  if (ctx->mode != 2) return SHK_ERR_STATE;
  int rc = check_batch(ctx, batch);
  if (rc) return rc;
  SHK_HIP(ctx, hipSetDevice(ctx->prm.device));
  TraceRange tr("shk_classify_device");
  return classify_resident(ctx, batch, max_read_len, result);
}

// ---- host batches: a pipeline of PIPE_DEPTH batches per context ---------------------------------
// submit(i): host scan of the offsets, H2D on the copy stream, every kernel on the compute stream behind an event,
//            no host round trip.  wait(i): the batch's event, then D2H of exactly its results into the slot's pinned
//            buffers.  While the host waits for batch i, the H2D of batch i+1 and i+2 overlaps the kernels of batch i
//            (the reference overlaps split / analyze / output across its worker threads, main.cpp:66-77).
int shk_classify_submit(shk_ctx *ctx, const shk_batch *b, uint64_t *ticket)
{
  if (!ctx || !ticket) return SHK_ERR_ARG;
  if (ctx->mode != 2) return SHK_ERR_STATE;
  int rc = check_batch(ctx, b);
  if (rc) return rc;
  SHK_HIP(ctx, hipSetDevice(ctx->prm.device));
  TraceRange tr("shk_classify_submit");
  Slot &s = ctx->slots[(ctx->next_ticket - 1) % PIPE_DEPTH];
  if (s.ticket != 0 && !s.waited) {
    ctx->last_error = "pipeline full: shk_classify_wait the oldest ticket before submitting another batch";
    return SHK_ERR_STATE;
  }
  const uint64_t n = b->n;
  if (n >= 0xFFFFFFFFull) { ctx->last_error = "batch too large (n must be < 2^32-1)"; return SHK_ERR_ARG; }
  const bool paired = b->seq2 != nullptr;
  const uint32_t k = ctx->prm.k;
  // one pass over the offsets: validation, the longest mate (selects the kernel specialisation), and whether every
  // read has the same length (then the offsets are generated on the device instead of crossing PCIe)
  uint64_t max1 = 0, max2 = 0, bad = 0;
  const uint64_t f1 = n ? b->off1[1] - b->off1[0] : 0, f2 = (n && paired) ? b->off2[1] - b->off2[0] : 0;
  uint64_t nonuni = n ? (b->off1[0] | (paired ? b->off2[0] : 0)) : 0;
  for (uint64_t i = 0; i < n; ++i) {
    const uint64_t a = b->off1[i], e = b->off1[i + 1];
    bad |= (uint64_t)(e < a);
    const uint64_t l = e - a;
    max1 = l > max1 ? l : max1;
    nonuni |= l ^ f1;
  }
  if (paired)
    for (uint64_t i = 0; i < n; ++i) {
      const uint64_t a = b->off2[i], e = b->off2[i + 1];
      bad |= (uint64_t)(e < a);
      const uint64_t l = e - a;
      max2 = l > max2 ? l : max2;
      nonuni |= l ^ f2;
    }
  if (bad) return SHK_ERR_ARG;
  const bool uniform = n && !nonuni;
  const uint64_t bytes1 = n ? b->off1[n] : 0;
  const uint64_t bytes2 = (n && paired) ? b->off2[n] : 0;
  // slot count of the longest read decides the specialisation; only when even the largest one is too small do reads
  // go to the general kernel, and then the host counts them here (so the device never has to be asked)
  uint32_t max_slots = slots_of_read(max1, max2, k);   // an upper bound for every read: the slot count is monotone in both lengths
  // Reads with more slots than the largest specialisation go to the general kernel; the host counts them here with the
  // kernels' own criterion (classify.hip), so the device never has to be asked.  Only when the bound says there are any.
  uint32_t n_long = 0, long_slots = 0;
  const uint64_t groups_bound = ((max1 + 7) >> 3) + ((max2 + 7) >> 3);
  const bool groups_fit = groups_bound <= uni_kernel_max_groups(max_slots);   // else the batch runs on classify_fast_kernel, which stages any number of groups
  if (max_slots > fast_kernel_max_slots()) {
    const uint32_t cap = 64 * fast_kernel_unroll(std::min(max_slots, fast_kernel_max_slots()));
    for (uint64_t i = 0; i < n; ++i) {
      const uint64_t l1 = b->off1[i + 1] - b->off1[i], l2 = paired ? b->off2[i + 1] - b->off2[i] : 0;
      const uint32_t ns = slots_of_read(l1, l2, k);
      if (ns > cap) {
        long_slots = std::max(long_slots, ns);
        ++n_long;
      }
    }
    if (max_slots > fast_kernel_max_slots()) max_slots = fast_kernel_max_slots();
  }

  hipStream_t up = ctx->h2d_stream, st = ctx->stream;
  shk_batch d{};
  d.n = n;
  if ((rc = s.d_seq1.reserve(ctx, bytes1 + 16))) return rc;
  if ((rc = s.d_off1.reserve(ctx, n + 1))) return rc;
  if (paired) {
    if ((rc = s.d_seq2.reserve(ctx, bytes2 + 16))) return rc;
    if ((rc = s.d_off2.reserve(ctx, n + 1))) return rc;
  }
  const bool hasq = ctx->q8 != 0;
  if (hasq) {
    if ((rc = s.d_qual1.reserve(ctx, bytes1 + 16))) return rc;
    if (paired && (rc = s.d_qual2.reserve(ctx, bytes2 + 16))) return rc;
  }
  if (n) {
    SHK_HIP(ctx, hipMemcpyAsync(s.d_seq1.p, b->seq1, bytes1, hipMemcpyHostToDevice, up));
    if (paired) SHK_HIP(ctx, hipMemcpyAsync(s.d_seq2.p, b->seq2, bytes2, hipMemcpyHostToDevice, up));
    if (hasq) {
      SHK_HIP(ctx, hipMemcpyAsync(s.d_qual1.p, b->qual1, bytes1, hipMemcpyHostToDevice, up));
      if (paired) SHK_HIP(ctx, hipMemcpyAsync(s.d_qual2.p, b->qual2, bytes2, hipMemcpyHostToDevice, up));
    }
    if (uniform) {
      if ((rc = launch_fill_offsets(s.d_off1.p, n + 1, f1, st))) return rc;
      if (paired && (rc = launch_fill_offsets(s.d_off2.p, n + 1, f2, st))) return rc;
    } else {
      SHK_HIP(ctx, hipMemcpyAsync(s.d_off1.p, b->off1, (n + 1) * sizeof(uint64_t), hipMemcpyHostToDevice, up));
      if (paired) SHK_HIP(ctx, hipMemcpyAsync(s.d_off2.p, b->off2, (n + 1) * sizeof(uint64_t), hipMemcpyHostToDevice, up));
    }
  }
  SHK_HIP(ctx, hipEventRecord(s.ev_h2d, up));
  SHK_HIP(ctx, hipStreamWaitEvent(st, s.ev_h2d, 0));
  d.seq1 = (const char *)s.d_seq1.p; d.off1 = s.d_off1.p;
  if (paired) { d.seq2 = (const char *)s.d_seq2.p; d.off2 = s.d_off2.p; }
  if (hasq) { d.qual1 = (const char *)s.d_qual1.p; if (paired) d.qual2 = (const char *)s.d_qual2.p; }
  s.host_batch = true;
  s.long_speculative = false;
  const bool uni_fits = uniform && n_long == 0 && groups_fit;
  if ((rc = enqueue_classify(ctx, s, &d, max_slots, LONG_KNOWN, n_long, long_slots, true, uni_fits ? UNI_YES : UNI_NO, (uint32_t)max1, (uint32_t)max2,
                             groups_fit)))
    return rc;
  s.ticket = ctx->next_ticket++;
  s.waited = false;
  *ticket = s.ticket;
  return SHK_OK;
}

// the device-resident entry point as a pipeline (no host synchronisation): see the header
int shk_classify_device_submit(shk_ctx *ctx, const shk_batch *b, uint32_t max_read_len, uint32_t uniform_len1, uint32_t uniform_len2, uint64_t *ticket)
{
  if (!ctx || !ticket || max_read_len == 0) return SHK_ERR_ARG;
  if (ctx->mode != 2) return SHK_ERR_STATE;
  int rc = check_batch(ctx, b);
  if (rc) return rc;
  SHK_HIP(ctx, hipSetDevice(ctx->prm.device));
  TraceRange tr("shk_classify_device_submit");
  Slot &s = ctx->slots[(ctx->next_ticket - 1) % PIPE_DEPTH];
  if (s.ticket != 0 && !s.waited) {
    ctx->last_error = "pipeline full: shk_classify_wait the oldest ticket before submitting another batch";
    return SHK_ERR_STATE;
  }
  const uint64_t n = b->n;
  if (n >= 0xFFFFFFFFull) { ctx->last_error = "batch too large (n must be < 2^32-1)"; return SHK_ERR_ARG; }
  const bool paired = b->seq2 != nullptr;
  if (uniform_len1 > max_read_len || uniform_len2 > max_read_len || (!paired && uniform_len2)) {
    ctx->last_error = "uniform_len1 / uniform_len2 exceed max_read_len, or uniform_len2 given for a single-end batch";
    return SHK_ERR_ARG;
  }
  uint32_t max_slots = slots_for_len(max_read_len, ctx->prm.k, paired);
  // a bound beyond the largest specialisation: the device would have to be asked how many reads do not fit
  if (max_slots > fast_kernel_max_slots()) { ctx->last_error = "max_read_len beyond the kernels' specialisations: use shk_classify_device"; return SHK_ERR_ARG; }
  const uint64_t hint_groups = (((uint64_t)max_read_len + 7) >> 3) * (paired ? 2 : 1);
  const bool groups_fit = hint_groups <= uni_kernel_max_groups(max_slots);
  const bool vouched = n != 0 && uniform_len1 != 0 && (paired ? uniform_len2 != 0 : true) && groups_fit;
  s.host_batch = false;
  s.long_speculative = true;
  if ((rc = enqueue_classify(ctx, s, b, max_slots, LONG_NONE_EXPECTED, 0, 0, true, vouched ? UNI_YES : UNI_ASK_DEVICE,
                             vouched ? uniform_len1 : max_read_len, vouched ? uniform_len2 : (paired ? max_read_len : 0), groups_fit)))
    return rc;
  s.ticket = ctx->next_ticket++;
  s.waited = false;
  *ticket = s.ticket;
  return SHK_OK;
}

int shk_classify_wait(shk_ctx *ctx, uint64_t ticket, shk_result *result)
{
  if (!ctx || !result || ticket == 0) return SHK_ERR_ARG;
  SHK_HIP(ctx, hipSetDevice(ctx->prm.device));
  TraceRange tr("shk_classify_wait");
  Slot &s = ctx->slots[(ticket - 1) % PIPE_DEPTH];
  if (s.ticket != ticket || s.waited) { ctx->last_error = "unknown or already waited ticket"; return SHK_ERR_STATE; }
  ctx->last_rec = LastRecords{};   // (a batch that is refused below hands out no records either, and leaves none of an earlier batch behind)
  SHK_HIP(ctx, hipEventSynchronize(s.ev_done));
  bool redone = false;
  int rc = finish_classify(ctx, s, s.long_speculative, true, &redone);
  if (rc) { s.waited = true; return rc; }
  if (!s.host_batch && s.h_counters[CTR_VOUCH_BAD]) {
    ctx->last_error = "uniform_len1 / uniform_len2 do not describe the batch: its offsets are not r * length (shk_classify_device_submit)";
    s.waited = true;
    return SHK_ERR_ARG;
  }
  // (finish_classify re-ran the tail when it had to, and the tail publishes the results again)
  const uint64_t n = s.n;
  const uint64_t n_assoc = ((uint64_t)s.h_counters[CTR_ASSOC_HI] << 32) | s.h_counters[CTR_ASSOC_LO];
  if (s.h_counters[CTR_OVERFLOW] || (s.host_batch && n_assoc > s.h_gene_ids.cap)) { ctx->last_error = "result publication failed"; s.waited = true; return SHK_ERR_HIP; }
  s.waited = true;
  ctx->last.last_n_reads = n;
  ctx->last.last_n_long = s.h_counters[CTR_LONG];
  ctx->last.last_n_tie = s.h_counters[CTR_TIE];
  note_verdict(ctx, s.h_counters[CTR_VERDICT]);
  ctx->last.last_n_assoc = n_assoc;
  result->n = n;
  result->gene_off = s.host_batch ? s.h_gene_off.p : s.d_gene_off.p;     // (a device-resident ticket: device pointers)
  result->gene_ids = s.host_batch ? s.h_gene_ids.p : s.d_gene_ids.p;
  result->n_assoc = n_assoc;
  return hand_out_records(ctx, s, s.host_batch, false, n_assoc);
}

// what every enable, read-out and reset of a mode or state refuses: a change while a submitted batch was not waited for
static int refuse_tickets(shk_ctx *ctx, const char *who)
{
  for (int i = 0; i < PIPE_DEPTH; ++i)
    if (ctx->slots[i].ticket != 0 && !ctx->slots[i].waited) {
      ctx->last_error = std::string(who) + ": tickets are outstanding (wait for them first)";
      return SHK_ERR_STATE;
    }
  return SHK_OK;
}

// what a mode that reads the placement table asks of the index, in this order: finalized, built with shk_ref_keep_positions, at most
// 65 536 records (NEED_GENE_START: and the genes' starts, which such an index carries) and, NEED_BASES, built with shk_ref_keep_bases
enum { NEED_GENE_START = 1, NEED_BASES = 2 };
static int check_mode_index(shk_ctx *ctx, const char *who, unsigned need)
{
  const std::string w(who);
  if (ctx->mode != 2) { ctx->last_error = w + ": the index is not finalized"; return SHK_ERR_STATE; }
  if (!ctx->idx.ptab_lg) { ctx->last_error = w + ": the index was finalized without shk_ref_keep_positions"; return SHK_ERR_STATE; }
  if (ctx->n_records > 65536 || ctx->idx.wrap || ((need & NEED_GENE_START) && !ctx->idx.gene_start)) {
    ctx->last_error = w + ": more than 65 536 records (gene ids wrap)";
    return SHK_ERR_STATE;
  }
  if ((need & NEED_BASES) && !ctx->idx.recbase) { ctx->last_error = w + ": the index was finalized without shk_ref_keep_bases"; return SHK_ERR_STATE; }
  return SHK_OK;
}

int shk_evidence_enable(shk_ctx *ctx, int enable)
{
  if (!ctx) return SHK_ERR_ARG;
  if (const int rc = refuse_tickets(ctx, "shk_evidence_enable")) return rc;
  ctx->evidence = enable != 0;
  return SHK_OK;
}

int shk_evidence_last(const shk_ctx *ctx, shk_evidence *out)
{
  if (!ctx || !out) return SHK_ERR_ARG;
  if (!ctx->last_rec.evid_valid) return SHK_ERR_STATE;
  out->n = ctx->last_rec.n;
  out->reads = ctx->last_rec.evid;
  return SHK_OK;
}

int shk_candidates_enable(shk_ctx *ctx, uint32_t m)
{
  if (!ctx) return SHK_ERR_ARG;
  if (m > SHK_MAX_CANDIDATES) { ctx->last_error = "shk_candidates_enable: m must be at most SHK_MAX_CANDIDATES"; return SHK_ERR_ARG; }
  if (const int rc = refuse_tickets(ctx, "shk_candidates_enable")) return rc;
  ctx->cand_m = m;
  return SHK_OK;
}

int shk_candidates_last(const shk_ctx *ctx, shk_candidates *out)
{
  if (!ctx || !out) return SHK_ERR_ARG;
  if (!ctx->last_rec.cand_valid) return SHK_ERR_STATE;
  out->n = ctx->last_rec.n;   // (the batch whose result was handed out last: one n for both kinds of record)
  out->m = ctx->last_rec.cand_m;
  out->reads = ctx->last_rec.cand_reads;
  out->entries = ctx->last_rec.cand_entries;
  return SHK_OK;
}

int shk_ref_keep_positions(shk_ctx *ctx)
{
  if (!ctx) return SHK_ERR_ARG;
  if (ctx->mode != 0) { ctx->last_error = "shk_ref_keep_positions: the index is finalized already"; return SHK_ERR_STATE; }
  ctx->keep_positions = true;
  return SHK_OK;
}

int shk_ref_kmer_table(shk_ctx *ctx, int on)
{
  if (!ctx) return SHK_ERR_ARG;
  if (ctx->mode != 0) { ctx->last_error = "shk_ref_kmer_table: the index is finalized already"; return SHK_ERR_STATE; }
  ctx->kmer_table = on != 0;
  return SHK_OK;
}

int shk_ref_keep_bases(shk_ctx *ctx)
{
  if (!ctx) return SHK_ERR_ARG;
  if (ctx->mode != 0) { ctx->last_error = "shk_ref_keep_bases: the index is finalized already"; return SHK_ERR_STATE; }
  ctx->keep_positions = true;   // (the bases lie in gene_start's order, which the placement table's build provides)
  ctx->keep_bases = true;
  return SHK_OK;
}

int shk_placement_enable(shk_ctx *ctx, int enable)
{
  if (!ctx) return SHK_ERR_ARG;
  if (const int rc = refuse_tickets(ctx, "shk_placement_enable")) return rc;
  if (enable) {
    if (const int rc = check_mode_index(ctx, "shk_placement_enable", 0)) return rc;
  }
  ctx->placement = enable != 0;
  return SHK_OK;
}

int shk_placement_last(const shk_ctx *ctx, shk_placements *out)
{
  if (!ctx || !out) return SHK_ERR_ARG;
  if (!ctx->last_rec.place_valid) return SHK_ERR_STATE;
  out->n_assoc = ctx->last_rec.n_assoc;
  out->entries = ctx->last_rec.place;
  return SHK_OK;
}

int shk_segments_enable(shk_ctx *ctx, uint32_t m)
{
  if (!ctx) return SHK_ERR_ARG;
  if (m > SHK_MAX_SEGMENTS) { ctx->last_error = "shk_segments_enable: m must be at most SHK_MAX_SEGMENTS"; return SHK_ERR_ARG; }
  if (const int rc = refuse_tickets(ctx, "shk_segments_enable")) return rc;
  if (m) {
    if (const int rc = check_mode_index(ctx, "shk_segments_enable", 0)) return rc;
  }
  ctx->seg_m = m;
  return SHK_OK;
}

int shk_segments_last(const shk_ctx *ctx, shk_segments *out)
{
  if (!ctx || !out) return SHK_ERR_ARG;
  if (!ctx->last_rec.seg_valid) return SHK_ERR_STATE;
  out->n_assoc = ctx->last_rec.n_assoc;
  out->m = ctx->last_rec.seg_m;
  out->n_keys = ctx->last_rec.seg_keys;
  out->entries = ctx->last_rec.seg_entries;
  return SHK_OK;
}

// ---- the accumulated states (shark_internal.hpp): they live in the context, the batches' tails add to them ----
// what every read-out and reset of a state starts with, in this order: the state was enabled once (`what`: how the refusal names it), no
// ticket is outstanding, the context's device is current
static int state_ready(shk_ctx *ctx, const char *who, bool enabled, const char *what)
{
  if (!enabled) { ctx->last_error = std::string(who) + ": " + what + " was never enabled on this context"; return SHK_ERR_STATE; }
  if (const int rc = refuse_tickets(ctx, who)) return rc;
  SHK_HIP(ctx, hipSetDevice(ctx->prm.device));
  return SHK_OK;
}

// ---- depth mode (depth.hip) and pileup mode (pileup.hip, align.hip): two states of one type (CounterState), each of two kinds -- depth: plain
// intervals / the unions of kept spans, pileup: owned pieces / the alignment's final blocks.  What tells the two states apart: ----
struct CounterRules {
  CounterState &(*state)(shk_ctx *);
  const char *what;                    // state_ready's
  size_t (*entries)(uint64_t bases);   // counters over a reference of that many bases
  uint32_t per_base;                   // counters per base that a read-out hands back
  bool scanned;                        // a read-out hands back the scan of the counters (depth_scan), not the counters themselves
  const char *other_kind;              // the refusal of the other kind on a dirty state
  uint64_t max_mates;                  // what the 32-bit counters hold, and the read-outs' refusal beyond
  const char *too_many;
};
static const CounterRules DEPTH_RULES = {
  [](shk_ctx *c) -> CounterState & { return c->depth; }, "depth mode", [](uint64_t bases) { return (size_t)bases + 1; }, 1, true,
  ": the state holds depth of the other kind (plain / spliced): shk_depth_reset first",
  0x7FFFFFFFull, ": more than 2^31-1 mates counted since the last reset (32-bit depth counters)"};
// (four counters per record base, and at least one allocation's worth for an index without a base)
static const CounterRules PILEUP_RULES = {
  [](shk_ctx *c) -> CounterState & { return c->pileup; }, "pileup mode", [](uint64_t bases) { return std::max<size_t>((size_t)bases * 4, 4); }, 4, false,
  ": the state holds pileup of the other kind (owned / aligned): shk_pileup_reset first",
  0xFFFFFFFFull, ": more than 2^32-1 pileup mates since the last reset (32-bit counters)"};

static int counters_enable(shk_ctx *ctx, const CounterRules &R, uint32_t min_support, bool kind, unsigned need, const char *who)
{
  if (!ctx) return SHK_ERR_ARG;
  if (const int rc = refuse_tickets(ctx, who)) return rc;
  CounterState &S = R.state(ctx);
  if (min_support) {
    if (const int rc = check_mode_index(ctx, who, need)) return rc;
    if (S.mates.p && S.dirty && kind != S.kind) { ctx->last_error = std::string(who) + R.other_kind; return SHK_ERR_STATE; }
    if (!S.mates.p) {
      SHK_HIP(ctx, hipSetDevice(ctx->prm.device));
      // (out of memory: SHK_ERR_NOMEM, the mode stays off and the state never enabled -- both arrays or none)
      const size_t n = R.entries(ctx->gene_start.back());
      DevArray<uint32_t> counts;
      DevArray<unsigned long long> mates;
      int rc;
      if ((rc = counts.alloc_exact(ctx, n)) || (rc = mates.alloc_exact(ctx, 1))) return rc;
      S.counts = std::move(counts);
      S.mates = std::move(mates);
      SHK_HIP(ctx, hipMemsetAsync(S.counts.p, 0, n * sizeof(uint32_t), ctx->stream));
      SHK_HIP(ctx, hipMemsetAsync(S.mates.p, 0, sizeof(unsigned long long), ctx->stream));
    }
    S.kind = kind;
  }
  S.floor = min_support;
  return SHK_OK;
}

// what every read-out starts with: the state rules, the stream drained behind everything enqueued so far, the mate counter and its guard
static int counters_read_mates(shk_ctx *ctx, const CounterRules &R, const char *who, uint64_t *n_mates)
{
  CounterState &S = R.state(ctx);
  if (const int rc = state_ready(ctx, who, S.mates.p != nullptr, R.what)) return rc;
  unsigned long long m = 0;
  SHK_HIP(ctx, hipMemcpyAsync(&m, S.mates.p, sizeof(m), hipMemcpyDeviceToHost, ctx->stream));
  SHK_HIP(ctx, hipStreamSynchronize(ctx->stream));
  if (n_mates) *n_mates = m;
  if (m > R.max_mates) { ctx->last_error = std::string(who) + R.too_many; return SHK_ERR_INDEX_TOO_LARGE; }
  return SHK_OK;
}

// the counters of one gene, or with gene < 0 of all of them (only then may dst be device memory), as the state stands
static int counters_get(shk_ctx *ctx, const CounterRules &R, const char *who, int64_t gene, uint32_t *dst, uint64_t cap, int device)
{
  if (!ctx) return SHK_ERR_ARG;
  int rc = counters_read_mates(ctx, R, who, nullptr);
  if (rc) return rc;
  const std::vector<uint64_t> &gs = ctx->gene_start;
  if (gene >= 0 && (uint64_t)gene + 1 >= gs.size()) return SHK_ERR_ARG;
  const uint64_t a = gene < 0 ? 0 : R.per_base * gs[gene], len = R.per_base * (gene < 0 ? gs.back() : gs[gene + 1]) - a;
  if (cap < len || (!dst && len)) return SHK_ERR_ARG;
  if (len == 0) return SHK_OK;
  // (pileup: the counters are the answer: no scan, one copy)
  if (R.scanned && (rc = depth_scan(ctx))) return rc;
  const uint32_t *src = R.scanned ? ctx->depth.scan.p + 1 : R.state(ctx).counts.p;
  SHK_HIP(ctx, hipMemcpyAsync(dst, src + a, len * sizeof(uint32_t), device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, ctx->stream));
  SHK_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return SHK_OK;
}

static int counters_reset(shk_ctx *ctx, const CounterRules &R, const char *who)
{
  if (!ctx) return SHK_ERR_ARG;
  CounterState &S = R.state(ctx);
  if (const int rc = state_ready(ctx, who, S.mates.p != nullptr, R.what)) return rc;
  SHK_HIP(ctx, hipMemsetAsync(S.counts.p, 0, S.counts.cap * sizeof(uint32_t), ctx->stream));
  SHK_HIP(ctx, hipMemsetAsync(S.mates.p, 0, sizeof(unsigned long long), ctx->stream));
  if (R.scanned) ctx->depth.scan_current = false;
  S.dirty = false;
  SHK_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return SHK_OK;
}

int shk_depth_enable(shk_ctx *ctx, uint32_t min_support) { return counters_enable(ctx, DEPTH_RULES, min_support, false, NEED_GENE_START, "shk_depth_enable"); }
int shk_depth_enable_spliced(shk_ctx *ctx, uint32_t min_support) { return counters_enable(ctx, DEPTH_RULES, min_support, true, NEED_GENE_START, "shk_depth_enable_spliced"); }

int shk_depth_layout(const shk_ctx *ctx, uint64_t *gene_start, uint32_t n_genes)
{
  if (!ctx || !gene_start) return SHK_ERR_ARG;
  if (ctx->mode != 2 || ctx->gene_start.empty()) return SHK_ERR_STATE;
  if ((uint64_t)n_genes + 1 > ctx->gene_start.size()) return SHK_ERR_ARG;
  memcpy(gene_start, ctx->gene_start.data(), ((size_t)n_genes + 1) * sizeof(uint64_t));
  return SHK_OK;
}

int shk_depth_mates(const shk_ctx *cctx, uint64_t *n_mates)
{
  if (!cctx || !n_mates) return SHK_ERR_ARG;
  return counters_read_mates(const_cast<shk_ctx *>(cctx), DEPTH_RULES, "shk_depth_mates", n_mates);
}

int shk_depth_get_all(shk_ctx *ctx, uint32_t *depth, uint64_t cap, int device) { return counters_get(ctx, DEPTH_RULES, "shk_depth_get_all", -1, depth, cap, device); }
int shk_depth_get(shk_ctx *ctx, uint32_t gene, uint32_t *depth, uint64_t cap) { return counters_get(ctx, DEPTH_RULES, "shk_depth_get", gene, depth, cap, 0); }

int shk_depth_summary(shk_ctx *ctx, shk_gene_depth *out, uint32_t n_genes)
{
  if (!ctx || (!out && n_genes)) return SHK_ERR_ARG;
  int rc = counters_read_mates(ctx, DEPTH_RULES, "shk_depth_summary", nullptr);
  if (rc) return rc;
  if ((uint64_t)n_genes + 1 > ctx->gene_start.size()) return SHK_ERR_ARG;
  if (n_genes == 0) return SHK_OK;
  if ((rc = depth_scan(ctx))) return rc;
  if ((rc = launch_depth_summary(ctx))) return rc;
  SHK_HIP(ctx, hipMemcpyAsync(out, ctx->depth.summary.p, (size_t)n_genes * sizeof(shk_gene_depth), hipMemcpyDeviceToHost, ctx->stream));
  SHK_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return SHK_OK;
}

int shk_depth_reset(shk_ctx *ctx) { return counters_reset(ctx, DEPTH_RULES, "shk_depth_reset"); }

int shk_pileup_enable(shk_ctx *ctx, uint32_t min_support) { return counters_enable(ctx, PILEUP_RULES, min_support, false, NEED_GENE_START, "shk_pileup_enable"); }
int shk_pileup_enable_aligned(shk_ctx *ctx, uint32_t min_support) { return counters_enable(ctx, PILEUP_RULES, min_support, true, NEED_GENE_START | NEED_BASES, "shk_pileup_enable_aligned"); }

int shk_pileup_mates(const shk_ctx *cctx, uint64_t *n)
{
  if (!cctx || !n) return SHK_ERR_ARG;
  return counters_read_mates(const_cast<shk_ctx *>(cctx), PILEUP_RULES, "shk_pileup_mates", n);
}

int shk_pileup_get_all(shk_ctx *ctx, uint32_t *counts, uint64_t cap, int device) { return counters_get(ctx, PILEUP_RULES, "shk_pileup_get_all", -1, counts, cap, device); }
int shk_pileup_get(shk_ctx *ctx, uint32_t gene, uint32_t *counts, uint64_t cap) { return counters_get(ctx, PILEUP_RULES, "shk_pileup_get", gene, counts, cap, 0); }
int shk_pileup_reset(shk_ctx *ctx) { return counters_reset(ctx, PILEUP_RULES, "shk_pileup_reset"); }

// ---- the junction table (spliced.hip) ----
int shk_junctions_enable(shk_ctx *ctx, uint32_t min_support, uint64_t capacity)
{
  if (!ctx) return SHK_ERR_ARG;
  if (const int rc = refuse_tickets(ctx, "shk_junctions_enable")) return rc;
  JunctionState &J = ctx->junc;
  if (min_support) {
    int rc;
    if ((rc = check_mode_index(ctx, "shk_junctions_enable", NEED_GENE_START))) return rc;
    if (capacity > (1ull << 40)) { ctx->last_error = "shk_junctions_enable: capacity beyond 2^40 entries"; return SHK_ERR_ARG; }
    uint64_t cap = 64;
    while (cap < capacity) cap <<= 1;
    if (!J.dropped.p) {
      SHK_HIP(ctx, hipSetDevice(ctx->prm.device));
      if ((rc = J.dropped.alloc_exact(ctx, 1))) return rc;
    }
    if ((rc = state_shape(ctx, J.tab, (size_t)cap, J.dirty, "shk_junctions_enable: another capacity than the table's (shk_junctions_reset first)",
                          [&] { return launch_junction_clear(ctx); })))
      return rc;
  }
  J.floor = min_support;
  return SHK_OK;
}

int shk_junctions_get(shk_ctx *ctx, shk_junction *out, uint64_t cap, uint64_t *n)
{
  if (!ctx || !n) return SHK_ERR_ARG;
  const JunctionState &J = ctx->junc;
  if (const int rc = state_ready(ctx, "shk_junctions_get", J.tab.p != nullptr, "the junction table")) return rc;
  // once per sample: the whole table to the host, the occupied entries ordered there.  Key order IS (gene, donor, acceptor) order: the
  // genes' bases are numbered gene after gene and a donor is at least k, so within the reference donors ascend with (gene, donor)
  std::vector<JunctionEntry> tab(J.tab.cap);
  unsigned long long dropped = 0;
  SHK_HIP(ctx, hipMemcpyAsync(&dropped, J.dropped.p, sizeof(dropped), hipMemcpyDeviceToHost, ctx->stream));
  SHK_HIP(ctx, hipMemcpyAsync(tab.data(), J.tab.p, tab.size() * sizeof(JunctionEntry), hipMemcpyDeviceToHost, ctx->stream));
  SHK_HIP(ctx, hipStreamSynchronize(ctx->stream));
  if (dropped) {
    ctx->last_error = "shk_junctions_get: the table was full for " + std::to_string(dropped) + " observations (shk_junctions_reset, then a larger capacity)";
    return SHK_ERR_INDEX_TOO_LARGE;
  }
  tab.erase(std::remove_if(tab.begin(), tab.end(), [](const JunctionEntry &e) { return e.key == JUNCTION_EMPTY; }), tab.end());
  *n = tab.size();
  if (!out) return SHK_OK;
  if (cap < tab.size()) return SHK_ERR_ARG;
  std::sort(tab.begin(), tab.end(), [](const JunctionEntry &a, const JunctionEntry &b) { return a.key < b.key; });
  const std::vector<uint64_t> &gs = ctx->gene_start;
  for (size_t i = 0; i < tab.size(); ++i) {
    const uint64_t donor = tab[i].key >> 32, acceptor = tab[i].key & 0xFFFFFFFFull;
    // acceptor < len_g strictly: the last gene that starts at or in front of it (genes without a record have no bases)
    const size_t g = (size_t)(std::upper_bound(gs.begin(), gs.end(), acceptor) - gs.begin()) - 1;
    out[i].gene = (uint32_t)g;
    out[i].donor = (uint32_t)(donor - gs[g]);
    out[i].acceptor = (uint32_t)(acceptor - gs[g]);
    out[i].intron = tab[i].intron;
    out[i].mates = tab[i].mates;
  }
  return SHK_OK;
}

int shk_junctions_reset(shk_ctx *ctx)
{
  if (!ctx) return SHK_ERR_ARG;
  if (const int rc = state_ready(ctx, "shk_junctions_reset", ctx->junc.tab.p != nullptr, "the junction table")) return rc;
  if (const int rc = launch_junction_clear(ctx)) return rc;
  ctx->junc.dirty = false;
  SHK_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return SHK_OK;
}

// ---- indels mode (indels.hip): the table and its counters live in the context, the batches' tails add to them ----
int shk_indels_enable(shk_ctx *ctx, uint32_t min_support, uint32_t min_intron, uint64_t capacity)
{
  if (!ctx) return SHK_ERR_ARG;
  if (const int rc = refuse_tickets(ctx, "shk_indels_enable")) return rc;
  IndelState &I = ctx->indel;
  if (min_support) {
    int rc;
    if (min_intron < 1 || min_intron > 65535) { ctx->last_error = "shk_indels_enable: min_intron is 1 .. 65535"; return SHK_ERR_ARG; }
    if ((rc = check_mode_index(ctx, "shk_indels_enable", NEED_GENE_START | NEED_BASES))) return rc;
    if (capacity > (1ull << 40)) { ctx->last_error = "shk_indels_enable: capacity beyond 2^40 entries"; return SHK_ERR_ARG; }
    if (ctx->gene_start.back() >= 0xFFFFFFFFull) { ctx->last_error = "shk_indels_enable: the records hold 2^32 - 1 bases or more (32-bit positions in the table's keys)"; return SHK_ERR_STATE; }
    uint64_t cap = 64;
    while (cap < capacity) cap <<= 1;
    if (I.tab.p && I.dirty && min_intron != I.min_intron) {
      ctx->last_error = "shk_indels_enable: another min_intron than the table's (shk_indels_reset first)";
      return SHK_ERR_ARG;
    }
    if (!I.stats.p) {
      SHK_HIP(ctx, hipSetDevice(ctx->prm.device));
      if ((rc = I.stats.alloc_exact(ctx, INDEL_STATS))) return rc;
    }
    if ((rc = state_shape(ctx, I.tab, (size_t)cap, I.dirty, "shk_indels_enable: another capacity than the table's (shk_indels_reset first)",
                          [&] { return launch_indel_clear(ctx); })))
      return rc;
    I.min_intron = min_intron;
  }
  I.floor = min_support;
  return SHK_OK;
}

// the table's counters as they stand, behind everything enqueued so far
static int indel_read_stats(shk_ctx *ctx, unsigned long long st[INDEL_STATS])
{
  SHK_HIP(ctx, hipMemcpyAsync(st, ctx->indel.stats.p, INDEL_STATS * sizeof(unsigned long long), hipMemcpyDeviceToHost, ctx->stream));
  SHK_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return SHK_OK;
}

int shk_indels_get(shk_ctx *ctx, uint32_t min_mates, shk_indel *out, uint64_t cap, uint64_t *n)
{
  if (!ctx || !n) return SHK_ERR_ARG;
  const IndelState &I = ctx->indel;
  if (const int rc = state_ready(ctx, "shk_indels_get", I.tab.p != nullptr, "indels mode")) return rc;
  // once per sample: the whole table to the host, the occupied entries ordered there.  Key order IS (gene, x, kind, len, seq) order: the
  // genes' bases are numbered gene after gene, and the event's half of the key is laid out in that order (indel_key)
  std::vector<IndelEntry> tab(I.tab.cap);
  unsigned long long st[INDEL_STATS];
  SHK_HIP(ctx, hipMemcpyAsync(tab.data(), I.tab.p, tab.size() * sizeof(IndelEntry), hipMemcpyDeviceToHost, ctx->stream));
  if (const int rc = indel_read_stats(ctx, st)) return rc;
  if (st[INDEL_STATS - 1]) {
    ctx->last_error = "shk_indels_get: the table was full for " + std::to_string(st[INDEL_STATS - 1]) + " observations (shk_indels_reset, then a larger capacity)";
    return SHK_ERR_INDEX_TOO_LARGE;
  }
  tab.erase(std::remove_if(tab.begin(), tab.end(), [&](const IndelEntry &e) { return e.key == INDEL_EMPTY || (uint64_t)e.fwd + e.rev < min_mates; }), tab.end());
  *n = tab.size();
  if (!out) return SHK_OK;
  if (cap < tab.size()) return SHK_ERR_ARG;
  std::sort(tab.begin(), tab.end(), [](const IndelEntry &a, const IndelEntry &b) { return a.key < b.key; });
  const std::vector<uint64_t> &gs = ctx->gene_start;
  for (size_t i = 0; i < tab.size(); ++i) {
    const uint64_t gx = tab[i].key >> 32;
    // x < len_g strictly: the last gene that starts at or in front of it (genes without a record have no bases)
    const size_t g = (size_t)(std::upper_bound(gs.begin(), gs.end(), gx) - gs.begin()) - 1;
    out[i].gene = (uint32_t)g;
    out[i].x = (uint32_t)(gx - gs[g]);
    indel_key_event((uint32_t)tab[i].key, out[i]);
    out[i].fwd = tab[i].fwd;
    out[i].rev = tab[i].rev;
    out[i].reserved = 0;
  }
  return SHK_OK;
}

int shk_indels_stats(shk_ctx *ctx, shk_indel_stats *out)
{
  if (!ctx || !out) return SHK_ERR_ARG;
  if (const int rc = state_ready(ctx, "shk_indels_stats", ctx->indel.tab.p != nullptr, "indels mode")) return rc;
  unsigned long long st[INDEL_STATS];
  if (const int rc = indel_read_stats(ctx, st)) return rc;
  *out = shk_indel_stats{st[0], st[1], st[2], st[3], st[4], st[5], st[6]};
  return SHK_OK;
}

int shk_indels_add(shk_ctx *ctx, const shk_indel *in, uint64_t n, const shk_indel_stats *stats)
{
  if (!ctx || (!in && n)) return SHK_ERR_ARG;
  if (const int rc = state_ready(ctx, "shk_indels_add", ctx->indel.tab.p != nullptr, "indels mode")) return rc;
  std::vector<IndelEntry> keyed;
  try {
    keyed.resize(n);
  } catch (...) {
    return SHK_ERR_NOMEM;
  }
  for (uint64_t i = 0; i < n; ++i) {
    unsigned long long key = 0;
    if (const int bad = indel_entry_key(in[i], ctx->gene_start.data(), ctx->gene_start.size() - 1, &key)) {
      ctx->last_error = "shk_indels_add: entry " + std::to_string(i) + " " + INDEL_ENTRY_RULES[bad];   // (the validation: indel_host.hpp)
      return SHK_ERR_ARG;
    }
    keyed[i] = IndelEntry{key, in[i].fwd, in[i].rev};
  }
  if (n == 0 && !stats) return SHK_OK;
  // (once per worker and sample: a buffer for the length of the call; the entries, then the counters)
  DevArray<IndelEntry> staged;
  if (const int rc = staged.alloc_exact(ctx, n + 4)) return rc;
  unsigned long long st[INDEL_STATS] = {0, 0, 0, 0, 0, 0, 0};
  if (stats) {
    const uint64_t v[INDEL_STATS] = {stats->mates, stats->deletions, stats->insertions, stats->complex_gaps, stats->long_insertions, stats->nonbase_insertions, stats->dropped};
    for (uint32_t c = 0; c < INDEL_STATS; ++c) st[c] = v[c];
  }
  unsigned long long *const d_stats = reinterpret_cast<unsigned long long *>(staged.p + n);   // (4 entries = 8 words >= INDEL_STATS)
  if (n) SHK_HIP(ctx, hipMemcpyAsync(staged.p, keyed.data(), n * sizeof(IndelEntry), hipMemcpyHostToDevice, ctx->stream));
  SHK_HIP(ctx, hipMemcpyAsync(d_stats, st, sizeof(st), hipMemcpyHostToDevice, ctx->stream));
  ctx->indel.dirty = true;
  int rc = launch_indel_add(ctx, staged.p, n, stats ? d_stats : nullptr);
  const hipError_t e = hipStreamSynchronize(ctx->stream);
  if (rc == SHK_OK && e != hipSuccess) rc = set_hip_error(ctx, e, "hipStreamSynchronize");
  return rc;
}

int shk_indels_reset(shk_ctx *ctx)
{
  if (!ctx) return SHK_ERR_ARG;
  if (const int rc = state_ready(ctx, "shk_indels_reset", ctx->indel.tab.p != nullptr, "indels mode")) return rc;
  if (const int rc = launch_indel_clear(ctx)) return rc;
  ctx->indel.dirty = false;
  SHK_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return SHK_OK;
}

// a caller's counters (another worker's or rank's state) added to the pileup state
int shk_pileup_add(shk_ctx *ctx, const uint32_t *counts, uint64_t n_entries, uint64_t mates, int device)
{
  if (!ctx) return SHK_ERR_ARG;
  if (const int rc = state_ready(ctx, "shk_pileup_add", ctx->pileup.mates.p != nullptr, "pileup mode")) return rc;
  if (n_entries != 4 * ctx->gene_start.back() || (!counts && n_entries)) { ctx->last_error = "shk_pileup_add: n_entries is not 4 * gene_start[nidx]"; return SHK_ERR_ARG; }
  uint32_t *staged = nullptr;
  if (!device && n_entries) {
    // (once per worker or rank and sample: a buffer for the length of the call)
    SHK_HIP(ctx, hipMalloc((void **)&staged, n_entries * sizeof(uint32_t)));
    if (hipError_t e = hipMemcpyAsync(staged, counts, n_entries * sizeof(uint32_t), hipMemcpyHostToDevice, ctx->stream)) { (void)hipFree(staged); return set_hip_error(ctx, e, "hipMemcpyAsync"); }
  }
  int rc = launch_pileup_add(ctx, staged ? staged : counts, n_entries, mates);
  const hipError_t e = hipStreamSynchronize(ctx->stream);
  if (staged) (void)hipFree(staged);
  if (rc == SHK_OK && e != hipSuccess) rc = set_hip_error(ctx, e, "hipStreamSynchronize");
  return rc;
}

// ---- variants mode (variants.hip): read-outs of the pileup state against DeviceIndex::recbase ----
static int variants_check(shk_ctx *ctx, const char *who, const shk_variant_params *p)
{
  if (!p || p->min_depth < 1 || p->min_alt < 1 || p->frac_den < 1 || p->frac_den > 65535 || p->frac_num > p->frac_den) {
    ctx->last_error = std::string(who) + ": parameters outside min_depth >= 1, min_alt >= 1, 1 <= frac_den <= 65535, frac_num <= frac_den";
    return SHK_ERR_ARG;
  }
  if (!ctx->pileup.mates.p) { ctx->last_error = std::string(who) + ": pileup mode was never enabled on this context"; return SHK_ERR_STATE; }
  if (!ctx->idx.recbase) { ctx->last_error = std::string(who) + ": the index was finalized without shk_ref_keep_bases"; return SHK_ERR_STATE; }
  return counters_read_mates(ctx, PILEUP_RULES, who, nullptr);   // (tickets, the stream drained, the mate guard)
}

int shk_variants_get(shk_ctx *ctx, const shk_variant_params *p, shk_variant *out, uint64_t cap, uint64_t *n)
{
  if (!ctx || !n) return SHK_ERR_ARG;
  if (const int rc = variants_check(ctx, "shk_variants_get", p)) return rc;
  return variants_call(ctx, *p, out, cap, n);
}

int shk_variants_summary(shk_ctx *ctx, const shk_variant_params *p, shk_gene_variants *out, uint32_t n_genes)
{
  if (!ctx) return SHK_ERR_ARG;
  if (const int rc = variants_check(ctx, "shk_variants_summary", p)) return rc;
  if ((uint64_t)n_genes + 1 > ctx->gene_start.size() || (!out && n_genes)) return SHK_ERR_ARG;
  if (n_genes == 0) return SHK_OK;
  if (const int rc = launch_variants_summary(ctx, *p)) return rc;
  SHK_HIP(ctx, hipMemcpyAsync(out, ctx->var.summary.p, (size_t)n_genes * sizeof(shk_gene_variants), hipMemcpyDeviceToHost, ctx->stream));
  SHK_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return SHK_OK;
}

// ---- alignments mode (align.hip): per-batch records, handed out as segments mode's are ----
int shk_alignments_enable(shk_ctx *ctx, uint32_t min_support)
{
  if (!ctx) return SHK_ERR_ARG;
  if (const int rc = refuse_tickets(ctx, "shk_alignments_enable")) return rc;
  if (min_support) {
    if (const int rc = check_mode_index(ctx, "shk_alignments_enable", NEED_GENE_START | NEED_BASES)) return rc;
  }
  ctx->align = min_support;
  return SHK_OK;
}

int shk_alignments_extend(shk_ctx *ctx, uint32_t mismatch_penalty, uint32_t end_bonus)
{
  if (!ctx) return SHK_ERR_ARG;
  if (mismatch_penalty > 15 || end_bonus > 15) { ctx->last_error = "shk_alignments_extend: mismatch_penalty and end_bonus are at most 15"; return SHK_ERR_ARG; }
  if (const int rc = refuse_tickets(ctx, "shk_alignments_extend")) return rc;
  ctx->ext_p = mismatch_penalty;
  ctx->ext_b = end_bonus;
  return SHK_OK;
}

// ---- spliced ends (align.hip's step 3b): the context's site list and the step's parameters ----
int shk_splice_sites_set(shk_ctx *ctx, const shk_splice_site *sites, uint64_t n)
{
  if (!ctx || (!sites && n)) return SHK_ERR_ARG;
  if (const int rc = check_mode_index(ctx, "shk_splice_sites_set", NEED_GENE_START)) return rc;
  if (const int rc = refuse_tickets(ctx, "shk_splice_sites_set")) return rc;
  if (n >= (1ull << 31)) { ctx->last_error = "shk_splice_sites_set: fewer than 2^31 sites"; return SHK_ERR_ARG; }
  const uint64_t n_genes = ctx->gene_start.size() - 1;
  for (uint64_t i = 0; i < n; ++i) {
    const shk_splice_site &t = sites[i];
    const uint64_t len_g = t.gene < n_genes ? ctx->gene_start[t.gene + 1] - ctx->gene_start[t.gene] : 0;
    const bool inside = t.gene < n_genes && t.donor >= 1 && t.donor < t.acceptor && (uint64_t)t.acceptor + 1 <= len_g;
    const bool ascends = i == 0 || std::make_tuple(sites[i - 1].gene, sites[i - 1].donor, sites[i - 1].acceptor) < std::make_tuple(t.gene, t.donor, t.acceptor);
    if (!inside || !ascends) {
      ctx->last_error = "shk_splice_sites_set: site " + std::to_string(i) + (inside ? " does not ascend in (gene, donor, acceptor)" : " lies outside its record (gene < n_records, 1 <= donor < acceptor <= len - 1)");
      return SHK_ERR_ARG;
    }
  }
  SHK_HIP(ctx, hipSetDevice(ctx->prm.device));
  SHK_HIP(ctx, hipStreamSynchronize(ctx->stream));   // (the list a batch read may go)
  if (n == 0) {
    (void)ctx->splice.d.release();
    std::vector<shk_splice_site>().swap(ctx->splice.sites);
    ctx->splice.h = 0;
    return SHK_OK;
  }
  std::vector<uint32_t> off;
  std::vector<uint2> by_donor, by_acceptor;
  std::vector<shk_splice_site> own;
  try {
    off.assign(n_genes + 1, 0);
    by_donor.resize(n);
    by_acceptor.resize(n);
    own.assign(sites, sites + n);
    for (uint64_t i = 0; i < n; ++i) {
      ++off[own[i].gene + 1];
      by_donor[i] = by_acceptor[i] = make_uint2(own[i].donor, own[i].acceptor);
    }
    for (uint64_t g = 0; g < n_genes; ++g) off[g + 1] += off[g];
    for (uint64_t g = 0; g < n_genes; ++g) {
      std::sort(by_acceptor.begin() + off[g], by_acceptor.begin() + off[g + 1], [](const uint2 &a, const uint2 &b) { return a.y != b.y ? a.y < b.y : a.x < b.x; });
    }
    for (uint2 &t : by_acceptor) std::swap(t.x, t.y);   // {acceptor, donor}
  } catch (...) {
    return SHK_ERR_NOMEM;
  }
  // the new list is whole on the device before the earlier one goes: a call that fails leaves the context as it was
  const size_t word = shk::splice_sites_word((uint32_t)n_genes);
  DevArray<uint32_t> fresh;
  if (const int rc = fresh.alloc_exact(ctx, word + 4 * n)) return rc;
  uint32_t *const d_new = fresh.p;
  hipError_t e = hipMemcpyAsync(d_new, off.data(), off.size() * sizeof(uint32_t), hipMemcpyHostToDevice, ctx->stream);
  if (e == hipSuccess) e = hipMemcpyAsync(d_new + word, by_donor.data(), n * sizeof(uint2), hipMemcpyHostToDevice, ctx->stream);
  if (e == hipSuccess) e = hipMemcpyAsync(d_new + word + 2 * n, by_acceptor.data(), n * sizeof(uint2), hipMemcpyHostToDevice, ctx->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);   // (the vectors go with this call)
  if (e != hipSuccess) return shk::set_hip_error(ctx, e, "shk_splice_sites_set: copying the list");
  ctx->splice.d = std::move(fresh);
  ctx->splice.sites.swap(own);
  return SHK_OK;
}

int shk_alignments_splice(shk_ctx *ctx, uint32_t min_overhang, uint32_t max_cost, uint32_t min_gap)
{
  if (!ctx) return SHK_ERR_ARG;
  if (min_overhang > SHK_SPLICE_MAX_OVERHANG || max_cost > 64 || min_gap > 64) {
    ctx->last_error = "shk_alignments_splice: min_overhang is at most SHK_SPLICE_MAX_OVERHANG, max_cost and min_gap at most 64";
    return SHK_ERR_ARG;
  }
  if (const int rc = refuse_tickets(ctx, "shk_alignments_splice")) return rc;
  if (min_overhang && !ctx->splice.d.p) { ctx->last_error = "shk_alignments_splice: no site list (shk_splice_sites_set first)"; return SHK_ERR_STATE; }
  ctx->splice.h = min_overhang;
  ctx->splice.cost = max_cost;
  ctx->splice.gap = min_gap;
  return SHK_OK;
}

int shk_alignments_last(const shk_ctx *ctx, shk_alignments *out)
{
  if (!ctx || !out) return SHK_ERR_ARG;
  if (!ctx->last_rec.align_valid) return SHK_ERR_STATE;
  out->n_assoc = ctx->last_rec.n_assoc;
  out->entries = ctx->last_rec.align;
  return SHK_OK;
}

// ---- pairs mode (pairs.hip): per-batch records as alignments mode's; the fragments state lives in the context, the batches' tails add to it ----
int shk_pairs_enable(shk_ctx *ctx, uint32_t min_intron, uint32_t max_frag, uint32_t n_bins)
{
  if (!ctx) return SHK_ERR_ARG;
  if (const int rc = refuse_tickets(ctx, "shk_pairs_enable")) return rc;
  if (n_bins) {
    if (n_bins < 2 || n_bins > 4096 || min_intron < 1) { ctx->last_error = "shk_pairs_enable: n_bins is 0 or 2 .. 4096 and min_intron at least 1"; return SHK_ERR_ARG; }
    if (const int rc = check_mode_index(ctx, "shk_pairs_enable", NEED_GENE_START | NEED_BASES)) return rc;
    if (!ctx->align) { ctx->last_error = "shk_pairs_enable: alignments mode is off (shk_alignments_enable first)"; return SHK_ERR_STATE; }
    FragmentState &F = ctx->frag;
    const size_t entries = (size_t)n_bins + 6;
    if (const int rc = state_shape(ctx, F.hist, entries, F.dirty, "shk_pairs_enable: another n_bins than the state's (shk_fragments_reset first)", [&]() -> int {
          SHK_HIP(ctx, hipMemsetAsync(F.hist.p, 0, entries * sizeof(unsigned long long), ctx->stream));
          return SHK_OK;
        }))
      return rc;
    F.min_intron = min_intron;
    F.max_frag = max_frag;
  }
  ctx->frag.n_bins = n_bins;
  return SHK_OK;
}

int shk_pairs_last(const shk_ctx *ctx, shk_pairs *out)
{
  if (!ctx || !out) return SHK_ERR_ARG;
  if (!ctx->last_rec.pairs_valid) return SHK_ERR_STATE;
  out->n_assoc = ctx->last_rec.n_assoc;
  out->entries = ctx->last_rec.pairs;
  return SHK_OK;
}

// ---- rescue mode (rescue.hip): per-batch records as pairs mode's; nothing lives in the context but the parameters ----
int shk_rescue_enable(shk_ctx *ctx, uint32_t min_intron, uint32_t max_frag, uint32_t max_cost, uint32_t min_gap)
{
  if (!ctx) return SHK_ERR_ARG;
  if (const int rc = refuse_tickets(ctx, "shk_rescue_enable")) return rc;
  if (max_frag) {
    if (max_frag > 4096 || min_intron < 1 || max_cost > 255 || min_gap > 255) {
      ctx->last_error = "shk_rescue_enable: max_frag is 0 or 1 .. 4096, min_intron at least 1, max_cost and min_gap at most 255";
      return SHK_ERR_ARG;
    }
    if (const int rc = check_mode_index(ctx, "shk_rescue_enable", NEED_GENE_START | NEED_BASES)) return rc;
    if (!ctx->align) { ctx->last_error = "shk_rescue_enable: alignments mode is off (shk_alignments_enable first)"; return SHK_ERR_STATE; }
    ctx->rescue_min_intron = min_intron;
    ctx->rescue_max_cost = max_cost;
    ctx->rescue_min_gap = min_gap;
  }
  ctx->rescue_max_frag = max_frag;
  return SHK_OK;
}

int shk_rescue_last(const shk_ctx *ctx, shk_rescues *out)
{
  if (!ctx || !out) return SHK_ERR_ARG;
  if (!ctx->last_rec.rescue_valid) return SHK_ERR_STATE;
  out->n_assoc = ctx->last_rec.n_assoc;
  out->entries = ctx->last_rec.rescue;
  return SHK_OK;
}

int shk_fragments_get(shk_ctx *ctx, uint64_t *hist, uint32_t n_bins, uint64_t classes[6])
{
  if (!ctx || !hist || !classes) return SHK_ERR_ARG;
  if (const int rc = state_ready(ctx, "shk_fragments_get", ctx->frag.hist.p != nullptr, "pairs mode")) return rc;
  if (n_bins != ctx->frag.bins()) { ctx->last_error = "shk_fragments_get: n_bins is not the state's"; return SHK_ERR_ARG; }
  std::vector<unsigned long long> h((size_t)n_bins + 6);
  SHK_HIP(ctx, hipMemcpyAsync(h.data(), ctx->frag.hist.p, h.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost, ctx->stream));
  SHK_HIP(ctx, hipStreamSynchronize(ctx->stream));
  for (uint32_t b = 0; b < n_bins; ++b) hist[b] = h[b];
  for (uint32_t c = 0; c < 6; ++c) classes[c] = h[(size_t)n_bins + c];
  return SHK_OK;
}

int shk_fragments_reset(shk_ctx *ctx)
{
  if (!ctx) return SHK_ERR_ARG;
  FragmentState &F = ctx->frag;
  if (const int rc = state_ready(ctx, "shk_fragments_reset", F.hist.p != nullptr, "pairs mode")) return rc;
  SHK_HIP(ctx, hipMemsetAsync(F.hist.p, 0, F.hist.cap * sizeof(unsigned long long), ctx->stream));
  F.dirty = false;
  SHK_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return SHK_OK;
}

// the text form of one record (the header's walk): host code only
int shk_alignment_cigar(const shk_mate_alignment *a, uint32_t L, uint32_t min_intron, char *buf, size_t cap, uint32_t *nm)
{
  if (!a || !buf) return SHK_ERR_ARG;
  if (a->n_blocks == 0) {
    if (cap < 2) return SHK_ERR_ARG;
    buf[0] = '*'; buf[1] = 0;
    if (nm) *nm = 0;
    return SHK_OK;
  }
  if (a->n_blocks > SHK_MAX_SEGMENTS) return SHK_ERR_ARG;
  // the operations, merged as they come: at most S + 4 M + 3 (I, N or D) + S
  uint64_t len[2 + 3 * SHK_MAX_SEGMENTS];
  char op[2 + 3 * SHK_MAX_SEGMENTS];
  int n_ops = 0;
  auto push = [&](char o, uint64_t l) {
    if (!l) return;
    if (n_ops && op[n_ops - 1] == o) { len[n_ops - 1] += l; return; }
    op[n_ops] = o; len[n_ops] = l; ++n_ops;
  };
  uint64_t edits = a->mismatches, q_end = 0, x_end = 0;
  for (uint32_t r = 0; r < a->n_blocks; ++r) {
    const uint64_t x = a->block[r].x, q = a->block[r].q, l = a->block[r].len;
    if (!l || q + l > L) return SHK_ERR_ARG;
    if (r == 0) push('S', q);
    else {
      if (q < q_end || x < x_end) return SHK_ERR_ARG;
      const uint64_t R = q - q_end, G = x - x_end;
      push('I', R);
      edits += R;
      if (G >= min_intron) push('N', G);
      else { push('D', G); edits += G; }
    }
    push('M', l);
    q_end = q + l; x_end = x + l;
  }
  push('S', L - q_end);
  size_t at = 0;
  for (int o = 0; o < n_ops; ++o) {
    char t[24];
    const int w = snprintf(t, sizeof(t), "%llu%c", (unsigned long long)len[o], op[o]);
    if (at + (size_t)w + 1 > cap) return SHK_ERR_ARG;
    memcpy(buf + at, t, (size_t)w);
    at += (size_t)w;
  }
  buf[at] = 0;
  if (nm) *nm = (uint32_t)edits;
  return SHK_OK;
}

int shk_classify(shk_ctx *ctx, const shk_batch *b, shk_result *result)
{
  if (!ctx || !result) return SHK_ERR_ARG;
  uint64_t t = 0;
  int rc = shk_classify_submit(ctx, b, &t);
  if (rc) return rc;
  return shk_classify_wait(ctx, t, result);
}

int shk_gene_counts(shk_ctx *ctx, uint64_t *counts, uint32_t n)
{
  if (!ctx || !counts || n > 65536) return SHK_ERR_ARG;
  SHK_HIP(ctx, hipSetDevice(ctx->prm.device));
  SHK_HIP(ctx, hipStreamSynchronize(ctx->stream));
  SHK_HIP(ctx, hipMemcpy(counts, ctx->d_gene_counts, (size_t)n * sizeof(uint64_t), hipMemcpyDeviceToHost));
  return SHK_OK;
}

int shk_gene_counts_reset(shk_ctx *ctx)
{
  if (!ctx) return SHK_ERR_ARG;
  SHK_HIP(ctx, hipSetDevice(ctx->prm.device));
  SHK_HIP(ctx, hipMemsetAsync(ctx->d_gene_counts, 0, 65536 * sizeof(unsigned long long), ctx->stream));
  SHK_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return SHK_OK;
}

// ---- the path's one exchange step: all-reduce of the per-gene counters over RCCL ------------------
// Both forms reduce INTO the contexts' separate totals buffers: the per-GPU counters stay local, so classifying more
// reads and reducing again gives the totals again (not totals times the number of GPUs).

// contexts that share a device: their counters are added on that device (RCCL takes a device once per communicator)
__global__ void gene_counts_add_kernel(unsigned long long *__restrict__ dst, const unsigned long long *__restrict__ src, uint32_t n)
{
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) dst[i] += src[i];
}

// one process, several contexts (`shark --gpus N [--devices ...]`): normally one context per GPU; contexts that share a GPU
// (--devices 0,0: the N-context code paths rehearsed on one device) are summed on it first, and the collective runs over
// the distinct devices' first contexts
int shk_gene_counts_allreduce(shk_ctx **ctxs, int n_ctx, uint64_t *totals, uint32_t n)
{
  if (!ctxs || n_ctx < 1 || n > 65536) return SHK_ERR_ARG;
  for (int i = 0; i < n_ctx; ++i)
    if (!ctxs[i]) return SHK_ERR_ARG;
  shk_ctx *c0 = ctxs[0];
  for (int i = 0; i < n_ctx; ++i) {
    SHK_HIP(ctxs[i], hipSetDevice(ctxs[i]->prm.device));
    SHK_HIP(ctxs[i], hipStreamSynchronize(ctxs[i]->stream));
  }
  // leaders: the first context of every distinct device, in the order given
  std::vector<int> leader_of((size_t)n_ctx, 0), leaders;
  for (int i = 0; i < n_ctx; ++i) {
    int l = -1;
    for (int j : leaders)
      if (ctxs[j]->prm.device == ctxs[i]->prm.device) { l = j; break; }
    if (l < 0) { l = i; leaders.push_back(i); }
    leader_of[(size_t)i] = l;
  }
  const int n_lead = (int)leaders.size();
  const bool shared = n_lead != n_ctx;
  const size_t bytes = 65536 * sizeof(unsigned long long);
  if (shared) {
    // per device: totals of the leader = sum of the counters of the contexts on it (the streams are idle: synchronised above)
    for (int l : leaders) {
      shk_ctx *lc = ctxs[l];
      SHK_HIP(lc, hipSetDevice(lc->prm.device));
      SHK_HIP(lc, hipMemcpyAsync(lc->d_gene_totals, lc->d_gene_counts, bytes, hipMemcpyDeviceToDevice, lc->stream));
      for (int i = 0; i < n_ctx; ++i)
        if (i != l && leader_of[(size_t)i] == l)
          gene_counts_add_kernel<<<65536 / 256, 256, 0, lc->stream>>>(lc->d_gene_totals, ctxs[i]->d_gene_counts, 65536);
      SHK_HIP(lc, hipGetLastError());
      SHK_HIP(lc, hipStreamSynchronize(lc->stream));
    }
  }
  const char *force = getenv("SHK_FORCE_RCCL");
  const unsigned long long *src = shared ? c0->d_gene_totals : c0->d_gene_counts;
  if (n_lead > 1 || (force && force[0] == '1')) {
    RcclApi &api = rccl();
    if (!api.ok) { c0->last_error = "librccl.so.1 could not be loaded"; return SHK_ERR_HIP; }
    std::vector<int> devs((size_t)n_lead);
    for (int i = 0; i < n_lead; ++i) devs[(size_t)i] = ctxs[leaders[(size_t)i]]->prm.device;
    // the communicators of a group of contexts are created once and live in the (leading) contexts
    bool have = true;
    for (int l : leaders) have = have && ctxs[l]->group_comm && ctxs[l]->group_devs == devs;
    if (!have) {
      for (int i = 0; i < n_ctx; ++i)
        if (ctxs[i]->group_comm) { (void)api.CommDestroy(ctxs[i]->group_comm); ctxs[i]->group_comm = nullptr; }
      std::vector<rccl_comm_t> comms((size_t)n_lead, nullptr);
      const int init_rc = with_stdout_on_stderr([&] { return api.CommInitAll(comms.data(), n_lead, devs.data()); });
      if (init_rc != 0) { c0->last_error = "ncclCommInitAll failed"; return SHK_ERR_HIP; }
      for (int i = 0; i < n_lead; ++i) { ctxs[leaders[(size_t)i]]->group_comm = comms[(size_t)i]; ctxs[leaders[(size_t)i]]->group_devs = devs; }
      // RCCL sets its channels up on a communicator's FIRST collective (of the order of the whole reduction of 512 KiB, or more): one
      // throw-away all-reduce (of a scratch-free kind: the totals buffers onto themselves, before they hold anything when no device is
      // shared; with shared devices their sums are made again below), so that the reduction a caller times is a steady-state one
      int wrc = api.GroupStart();
      for (int i = 0; i < n_lead && wrc == 0; ++i) {
        shk_ctx *lc = ctxs[leaders[(size_t)i]];
        (void)hipSetDevice(devs[(size_t)i]);
        wrc = api.AllReduce(lc->d_gene_totals, lc->d_gene_totals, 65536, 5, 0, lc->group_comm, lc->stream);
      }
      if (wrc == 0) wrc = api.GroupEnd();
      for (int i = 0; i < n_lead; ++i) {
        (void)hipSetDevice(devs[(size_t)i]);
        (void)hipStreamSynchronize(ctxs[leaders[(size_t)i]]->stream);
      }
      if (wrc != 0) { c0->last_error = "ncclAllReduce (warm-up) failed"; return SHK_ERR_HIP; }
      if (shared) {   // the warm-up has overwritten the per-device sums: make them again
        for (int l : leaders) {
          shk_ctx *lc = ctxs[l];
          SHK_HIP(lc, hipSetDevice(lc->prm.device));
          SHK_HIP(lc, hipMemcpyAsync(lc->d_gene_totals, lc->d_gene_counts, bytes, hipMemcpyDeviceToDevice, lc->stream));
          for (int i = 0; i < n_ctx; ++i)
            if (i != l && leader_of[(size_t)i] == l)
              gene_counts_add_kernel<<<65536 / 256, 256, 0, lc->stream>>>(lc->d_gene_totals, ctxs[i]->d_gene_counts, 65536);
          SHK_HIP(lc, hipGetLastError());
          SHK_HIP(lc, hipStreamSynchronize(lc->stream));
        }
      }
    }
    int rc = api.GroupStart();
    for (int i = 0; i < n_lead && rc == 0; ++i) {
      shk_ctx *lc = ctxs[leaders[(size_t)i]];
      (void)hipSetDevice(devs[(size_t)i]);
      // ncclUint64 = 5, ncclSum = 0; 65 536 x 8 B per GPU (in place over the per-device sums when contexts share a device)
      rc = api.AllReduce(shared ? lc->d_gene_totals : lc->d_gene_counts, lc->d_gene_totals, 65536, 5, 0, lc->group_comm, lc->stream);
    }
    if (rc == 0) rc = api.GroupEnd();
    for (int i = 0; i < n_lead; ++i) {
      (void)hipSetDevice(devs[(size_t)i]);
      (void)hipStreamSynchronize(ctxs[leaders[(size_t)i]]->stream);
    }
    if (rc != 0) { c0->last_error = "ncclAllReduce failed"; return SHK_ERR_HIP; }
    src = c0->d_gene_totals;
  }
  if (shared) {   // every context's totals buffer holds the totals, as with one context per device
    for (int i = 0; i < n_ctx; ++i) {
      const int l = leader_of[(size_t)i];
      if (l == i) continue;
      SHK_HIP(ctxs[i], hipSetDevice(ctxs[i]->prm.device));
      SHK_HIP(ctxs[i], hipMemcpy(ctxs[i]->d_gene_totals, ctxs[l]->d_gene_totals, bytes, hipMemcpyDeviceToDevice));
    }
  }
  if (totals) {
    SHK_HIP(c0, hipSetDevice(c0->prm.device));
    SHK_HIP(c0, hipMemcpy(totals, src, (size_t)n * sizeof(uint64_t), hipMemcpyDeviceToHost));
  }
  return SHK_OK;
}

// one process per GPU (torch.distributed.run / mpirun style launchers): rank 0 makes an id, the launcher's own
// channel carries its SHK_DIST_ID_BYTES bytes to the other ranks, every rank joins with its context
int shk_dist_unique_id(uint8_t *id)
{
  if (!id) return SHK_ERR_ARG;
  RcclApi &api = rccl();
  if (!api.ok) return SHK_ERR_HIP;
  rccl_uid u;
  if (api.GetUniqueId(&u) != 0) return SHK_ERR_HIP;
  static_assert(sizeof(u) == SHK_DIST_ID_BYTES, "ncclUniqueId is 128 bytes");
  memcpy(id, &u, sizeof(u));
  return SHK_OK;
}

int shk_dist_init(shk_ctx *ctx, const uint8_t *id, int rank, int world)
{
  if (!ctx || !id || world < 1 || rank < 0 || rank >= world) return SHK_ERR_ARG;
  RcclApi &api = rccl();
  if (!api.ok) { ctx->last_error = "librccl.so.1 could not be loaded"; return SHK_ERR_HIP; }
  SHK_HIP(ctx, hipSetDevice(ctx->prm.device));
  if (ctx->dist_comm) { (void)api.CommDestroy(ctx->dist_comm); ctx->dist_comm = nullptr; }
  rccl_uid u;
  memcpy(&u, id, sizeof(u));
  rccl_comm_t comm = nullptr;
  const int rc = with_stdout_on_stderr([&] { return api.CommInitRank(&comm, world, u, rank); });
  if (rc != 0) { ctx->last_error = "ncclCommInitRank failed"; return SHK_ERR_HIP; }
  ctx->dist_comm = comm;
  ctx->dist_rank = rank;
  ctx->dist_world = world;
  // the communicator's first collective sets RCCL's channels up: made here (every rank is in this call), on the totals buffer, so
  // that shk_dist_gene_counts_allreduce is a steady-state collective from its first use on
  if (api.AllReduce(ctx->d_gene_totals, ctx->d_gene_totals, 65536, 5, 0, comm, ctx->stream) != 0) {
    ctx->last_error = "ncclAllReduce (warm-up) failed";
    return SHK_ERR_HIP;
  }
  SHK_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return SHK_OK;
}

int shk_dist_info(const shk_ctx *ctx, int *rank, int *world)
{
  if (!ctx || !rank || !world) return SHK_ERR_ARG;
  *rank = 0;
  *world = 1;
  if (ctx->dist_comm) {
    // asked of the communicator, not remembered from shk_dist_init's arguments
    if (rccl().CommUserRank(ctx->dist_comm, rank) != 0 || rccl().CommCount(ctx->dist_comm, world) != 0) return SHK_ERR_HIP;
  }
  return SHK_OK;
}

int shk_dist_gene_counts_allreduce(shk_ctx *ctx, uint64_t *totals, uint32_t n)
{
  if (!ctx || n > 65536) return SHK_ERR_ARG;
  SHK_HIP(ctx, hipSetDevice(ctx->prm.device));
  const unsigned long long *src = ctx->d_gene_counts;
  if (ctx->dist_comm) {
    // stream order: behind every classify call enqueued so far
    if (rccl().AllReduce(ctx->d_gene_counts, ctx->d_gene_totals, 65536, 5, 0, ctx->dist_comm, ctx->stream) != 0) {
      ctx->last_error = "ncclAllReduce failed";
      return SHK_ERR_HIP;
    }
    src = ctx->d_gene_totals;
  }
  SHK_HIP(ctx, hipStreamSynchronize(ctx->stream));
  if (totals) SHK_HIP(ctx, hipMemcpy(totals, src, (size_t)n * sizeof(uint64_t), hipMemcpyDeviceToHost));
  return SHK_OK;
}

int shk_timing_enable(shk_ctx *ctx, int enable)
{
  if (!ctx) return SHK_ERR_ARG;
  ctx->timing = enable != 0;
  ctx->ev_used = 0;
  return SHK_OK;
}

int shk_timing_get(shk_ctx *ctx, shk_timing *t)
{
  if (!ctx || !t) return SHK_ERR_ARG;
  SHK_HIP(ctx, hipSetDevice(ctx->prm.device));
  SHK_HIP(ctx, hipStreamSynchronize(ctx->stream));
  double total = 0.0, pre = 0.0;
  for (size_t i = 0; i < ctx->ev_used; ++i) {
    float ms = 0.f;
    SHK_HIP(ctx, hipEventElapsedTime(&ms, ctx->ev_start[i], ctx->ev_stop[i]));
    total += ms;
    SHK_HIP(ctx, hipEventElapsedTime(&ms, ctx->ev_pre[i], ctx->ev_start[i]));
    pre += ms;
  }
  *t = ctx->last;
  t->n_launches = ctx->ev_used;
  t->total_ms = total;
  t->prepass_ms = pre;
  return SHK_OK;
}

int shk_count_work(shk_ctx *ctx, const shk_batch *b, shk_work_counters *out)
{
  if (!ctx || !out) return SHK_ERR_ARG;
  if (ctx->mode != 2) return SHK_ERR_STATE;
  int rc = check_batch(ctx, b);
  if (rc) return rc;
  SHK_HIP(ctx, hipSetDevice(ctx->prm.device));
  shk_result tmp{};
  return classify_resident(ctx, b, 0, &tmp, out);
}

void *shk_alloc_pinned(size_t bytes)
{
  void *p = nullptr;
  if (hipHostMalloc(&p, bytes ? bytes : 1, hipHostMallocDefault) != hipSuccess) return nullptr;
  return p;
}

void shk_free_pinned(void *p)
{
  if (p) (void)hipHostFree(p);
}

}  // extern "C"
