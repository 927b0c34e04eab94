// pairs.hip -- pairs mode's kernel (gfx950): per association what its two mates' alignment records say together -- orientation class, left
// mate, template span, the introns either mate shows, fragment length, proper pair, MAPQ -- and the fragments state, the sample's
// fragment-size histogram (include/shark_hip.h, "pairs").  It reads what align_kernel has just stored and changes none of it.
//
// Shape: one LANE per read (align_kernel: one wave), workgroups of 256, at most PR_MAX_BLOCKS of them with a stride loop.  A lane reads
// gene_off[i] and gene_off[i + 1] coalesced and loops over its associations (almost always 0 or 1); per association the two mates' 128
// bytes are eight 16-byte loads -- one whole cache line per lane, every byte used -- and the record is two 16-byte stores.
//
// No index into registers is a run-time value: the last block's fields are selected by compares against n_blocks, a mate's three possible
// intron intervals sit at constant places (an absent one is empty), and the union of the two mates' intervals needs no sort: within one
// mate the intervals ascend and are disjoint (its blocks do), so |A u B| = |A| + |B| - sum of the nine pairwise overlaps.  No scratch
// memory.
//
// The fragments state (Guideline 12: the in-range bins of a sample sit on a few hundred addresses): a workgroup keeps hist and classes in
// LDS as 32-bit counters (n_bins + 6 words, at most 16.4 KiB; a batch has fewer than 2^32 associations), adds to hist with LDS atomics
// where the pair is found and to classes once per wave from per-lane counters, and flushes once behind a barrier when its stride loop
// has ended: one 64-bit global atomic per NON-ZERO word.  A batch that is not counted stores its records and touches neither.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "shark_internal.hpp"

namespace shk {

static_assert(sizeof(shk_pair) == 32, "a pair's record is two 16-byte stores");
static_assert(sizeof(shk_mate_alignment) == 64 && SHK_MAX_SEGMENTS == 4, "the record layout the loads below take apart");

namespace {

constexpr uint32_t PR_THREADS = 256;
constexpr uint32_t PR_MAX_BLOCKS = 512;         // 131 072 lanes: two workgroups per CU; a larger batch takes the stride loop's next trips
constexpr uint32_t PR_MAX_BINS = 4096;          // shk_pairs_enable's bound
constexpr uint32_t PR_CLASSES = 6;

struct PairParams {
  const uint32_t *gene_off;
  const uint32_t *counters;
  uint64_t n;                      // reads
  const uint64_t *off[2];          // nullptr: the batch has no such mate
  const uint4 *align;              // [(j * 2 + mate) * 4 + v]: shk_mate_alignment as four 16-byte words
  uint4 *out;                      // [j * 2 + v]
  unsigned long long *state;       // hist[n_bins], classes[6]; nullptr: the batch is not counted
  uint32_t cap;                    // associations `align` and `out` hold
  uint32_t skip_if_long;
  uint32_t min_intron, max_frag, n_bins;
  uint32_t n_lanes;                // of the launch: a lane's step through the reads
};

// what one mate's record says (the header's "per mate"); a mate without a block: has == 0 and everything else 0
struct MateEnds {
  uint32_t has, strand;
  int32_t s, e;
  uint32_t cl, cr;
  int32_t ilo[3], ihi[3];          // intron intervals at constant places; an absent one is [0, 0)
};

// v0 = {n_blocks, strand, matches, mismatches}, v1 = {x0, q0, len0, x1}, v2 = {q1, len1, x2, q2}, v3 = {len2, x3, q3, len3}
__device__ __forceinline__ MateEnds mate_ends(const uint4 v0, const uint4 v1, const uint4 v2, const uint4 v3, uint32_t L, uint32_t min_intron)
{
  MateEnds M;
  const uint32_t nb = v0.x;
  M.has = nb >= 1u ? 1u : 0u;
  M.strand = M.has && v0.y ? 1u : 0u;
  // the last block by compares against n_blocks (a record holds at most four)
  const uint32_t lx = nb <= 1u ? v1.x : (nb == 2u ? v1.w : (nb == 3u ? v2.z : v3.y));
  const uint32_t lq = nb <= 1u ? v1.y : (nb == 2u ? v2.x : (nb == 3u ? v2.w : v3.z));
  const uint32_t ll = nb <= 1u ? v1.z : (nb == 2u ? v2.y : (nb == 3u ? v3.x : v3.w));
  M.s = M.has ? (int32_t)v1.x : 0;
  M.e = M.has ? (int32_t)(lx + ll) : 0;
  M.cl = M.has ? v1.y : 0u;
  M.cr = M.has ? L - (lq + ll) : 0u;
  // the gap behind block t: [x_t + len_t, x_{t+1})
  const int32_t lo0 = (int32_t)(v1.x + v1.z), hi0 = (int32_t)v1.w;
  const int32_t lo1 = (int32_t)(v1.w + v2.y), hi1 = (int32_t)v2.z;
  const int32_t lo2 = (int32_t)(v2.z + v3.x), hi2 = (int32_t)v3.y;
  const bool i0 = nb >= 2u && hi0 > lo0 && (uint32_t)(hi0 - lo0) >= min_intron;
  const bool i1 = nb >= 3u && hi1 > lo1 && (uint32_t)(hi1 - lo1) >= min_intron;
  const bool i2 = nb >= 4u && hi2 > lo2 && (uint32_t)(hi2 - lo2) >= min_intron;
  M.ilo[0] = i0 ? lo0 : 0; M.ihi[0] = i0 ? hi0 : 0;
  M.ilo[1] = i1 ? lo1 : 0; M.ihi[1] = i1 ? hi1 : 0;
  M.ilo[2] = i2 ? lo2 : 0; M.ihi[2] = i2 ? hi2 : 0;
  return M;
}

__device__ __forceinline__ uint32_t clamp_len(uint64_t len) { return len > 0x7FFFFFFFull ? 0x7FFFFFFFu : (uint32_t)len; }   // (align_kernel's L)

__device__ __forceinline__ uint32_t wave_sum_u32(uint32_t v)
{
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) v += (uint32_t)__shfl_xor((int)v, o, 64);
  return v;
}

// STAGED: the histogram through LDS (the product).  !STAGED: one global atomic per pair and per association (tools/pairs_price.py times it
// once against the product, SHK_PAIRS_GLOBAL_ATOMICS=1; no other use).
template <bool STAGED>
__global__ __launch_bounds__(PR_THREADS) void pair_kernel(const PairParams P)
{
  // align_kernel's three: the batch will be assembled again and comes through here again; or it will be refused in wait
  if (P.counters[CTR_OVERFLOW] || (P.skip_if_long && P.counters[CTR_LONG]) || P.counters[CTR_VOUCH_BAD]) return;
  __shared__ uint32_t lds[STAGED ? PR_MAX_BINS + PR_CLASSES : 1];
  const bool counted = P.state != nullptr;      // (a kernel argument: the same in every lane)
  const uint32_t n_words = P.n_bins + PR_CLASSES;
  if constexpr (STAGED) {
    if (counted) {
      for (uint32_t w = threadIdx.x; w < n_words; w += PR_THREADS) lds[w] = 0u;
      __syncthreads();
    }
  }
  uint32_t n_cls[PR_CLASSES] = {0u, 0u, 0u, 0u, 0u, 0u};   // this lane's associations per class (constant indices only)
  for (uint64_t i = (uint64_t)blockIdx.x * PR_THREADS + threadIdx.x; i < P.n; i += P.n_lanes) {
    const uint32_t o0 = P.gene_off[i], o1 = P.gene_off[i + 1];
    if (o1 <= o0 || o1 > P.cap) continue;       // (align_kernel's guard for a read whose associations the buffers do not hold)
    const uint32_t n_assoc = o1 - o0;
    const uint32_t mapq = n_assoc == 1u ? 60u : (n_assoc == 2u ? 3u : (n_assoc <= 4u ? 1u : 0u));
    const uint32_t L0 = P.off[0] ? clamp_len(P.off[0][i + 1] - P.off[0][i]) : 0u;
    const uint32_t L1 = P.off[1] ? clamp_len(P.off[1][i + 1] - P.off[1][i]) : 0u;
    for (uint32_t j = o0; j < o1; ++j) {
      const uint4 *a = P.align + (uint64_t)j * 8u;
      const uint4 a0 = a[0], a1 = a[1], a2 = a[2], a3 = a[3], b0 = a[4], b1 = a[5], b2 = a[6], b3 = a[7];
      const MateEnds A = mate_ends(a0, a1, a2, a3, L0, P.min_intron), B = mate_ends(b0, b1, b2, b3, L1, P.min_intron);
      const bool both = A.has && B.has;
      const bool opposite = both && A.strand != B.strand;
      const bool a_is_f = A.strand == 0u;       // (read under `opposite` only: F is the mate on strand 0)
      const int32_t s_f = a_is_f ? A.s : B.s, e_f = a_is_f ? A.e : B.e, s_r = a_is_f ? B.s : A.s, e_r = a_is_f ? B.e : A.e;
      uint32_t cls = (A.has ? 1u : 0u) + (B.has ? 2u : 0u);             // 0, 1, 2; 3: both
      if (both) cls = !opposite ? 5u : (s_f <= s_r && e_f <= e_r ? 3u : 4u);
      // the mate with the smaller s, then the smaller e, then mate 0; the one mate where there is one
      const bool b_left = both ? (B.s < A.s || (B.s == A.s && B.e < A.e)) : (B.has != 0u);
      const int32_t tstart = both ? std::min(A.s, B.s) : (A.has ? A.s : B.s);
      const int32_t tend = both ? std::max(A.e, B.e) : (A.has ? A.e : B.e);
      // the union of the intron intervals: each mate's own are disjoint, so the nine pairwise overlaps are what is counted twice
      int32_t introns = 0;
#pragma unroll
      for (int t = 0; t < 3; ++t) introns += (A.ihi[t] - A.ilo[t]) + (B.ihi[t] - B.ilo[t]);
#pragma unroll
      for (int t = 0; t < 3; ++t) {
#pragma unroll
        for (int u = 0; u < 3; ++u) {
          const int32_t ov = std::min(A.ihi[t], B.ihi[u]) - std::max(A.ilo[t], B.ilo[u]);
          introns -= ov > 0 ? ov : 0;
        }
      }
      const uint32_t frag = cls == 3u ? (uint32_t)(tend - tstart) - (uint32_t)introns + (a_is_f ? A.cl : B.cl) + (a_is_f ? B.cr : A.cr) : 0u;
      const uint32_t proper = cls == 3u && frag <= P.max_frag ? 1u : 0u;
      uint4 r0, r1;
      r0.x = cls; r0.y = b_left ? 1u : 0u; r0.z = proper; r0.w = mapq;
      r1.x = (uint32_t)tstart; r1.y = (uint32_t)tend; r1.z = (uint32_t)introns; r1.w = frag;
      P.out[(uint64_t)j * 2u] = r0;
      P.out[(uint64_t)j * 2u + 1u] = r1;
      if (counted) {
        const uint32_t bin = std::min(frag, P.n_bins - 1u);
        if constexpr (STAGED) {
#pragma unroll
          for (uint32_t c = 0; c < PR_CLASSES; ++c) n_cls[c] += cls == c ? 1u : 0u;
          if (cls == 3u && n_assoc == 1u) atomicAdd(&lds[bin], 1u);
        } else {
          atomicAdd(P.state + P.n_bins + cls, 1ull);
          if (cls == 3u && n_assoc == 1u) atomicAdd(P.state + bin, 1ull);
        }
      }
    }
  }
  if constexpr (STAGED) {
    if (counted) {
      // (every lane of the workgroup arrives here: the returns above are taken by all or none, the loop has no barrier inside)
#pragma unroll
      for (uint32_t c = 0; c < PR_CLASSES; ++c) {
        const uint32_t t = wave_sum_u32(n_cls[c]);
        if ((threadIdx.x & 63u) == 0u && t) atomicAdd(&lds[P.n_bins + c], t);
      }
      __syncthreads();
      for (uint32_t w = threadIdx.x; w < n_words; w += PR_THREADS) {
        const uint32_t v = lds[w];
        if (v) atomicAdd(P.state + w, (unsigned long long)v);
      }
    }
  }
}

}  // namespace

int launch_pairs(Ctx *ctx, const Slot &s, uint64_t cap_assoc, bool skip_if_long, hipStream_t stream)
{
  if (!s.pairs || !s.align || !s.rec_align.d.p || !s.rec_pairs.d.p || s.pairs > PR_MAX_BINS || (s.pairs_count && ctx->frag.bins() != s.pairs)) {
    ctx->last_error = "pairs mode without its state";
    return SHK_ERR_STATE;
  }
  if (s.n == 0) return SHK_OK;
  PairParams P{};
  P.gene_off = s.d_gene_off.p;
  P.counters = s.d_counters;
  P.n = s.n;
  P.off[0] = s.p.seq1 ? s.p.off1 : nullptr;
  P.off[1] = s.p.seq2 ? s.p.off2 : nullptr;
  P.align = reinterpret_cast<const uint4 *>(s.rec_align.d.p);
  P.out = reinterpret_cast<uint4 *>(s.rec_pairs.d.p);
  P.state = s.pairs_count ? ctx->frag.hist.p : nullptr;
  // (launch_alignments' bound on the associations its records hold, and this mode's own array)
  P.cap = (uint32_t)std::min<uint64_t>(std::min<uint64_t>(std::min<uint64_t>(s.d_gene_ids.cap, cap_assoc), std::min<uint64_t>(s.rec_align.d.cap / 2, s.rec_pairs.d.cap)), 0xFFFFFFFFull);
  P.skip_if_long = skip_if_long ? 1u : 0u;
  P.min_intron = s.pairs_min_intron;
  P.max_frag = s.pairs_max_frag;
  P.n_bins = s.pairs;
  const unsigned blocks = (unsigned)std::min<uint64_t>((s.n + PR_THREADS - 1) / PR_THREADS, PR_MAX_BLOCKS);
  P.n_lanes = blocks * PR_THREADS;
  if (!ctx->env_pairs_global) hipLaunchKernelGGL(pair_kernel<true>, dim3(blocks), dim3(PR_THREADS), 0, stream, P);
  else hipLaunchKernelGGL(pair_kernel<false>, dim3(blocks), dim3(PR_THREADS), 0, stream, P);
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? SHK_OK : set_hip_error(ctx, e, "pair_kernel");
}

}  // namespace shk
