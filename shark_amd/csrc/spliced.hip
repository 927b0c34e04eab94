// spliced.hip -- the two consumers of segments mode on the device (gfx950): spliced depth and the junction table (include/shark_hip.h,
// "spliced depth and the junction table").  Both read a mate's KEPT SPANS (kept_spans.hpp) from the four records
// segments_kernel stored for it, behind that kernel in the batch's tail.
//
// spliced_accumulate_kernel has depth_accumulate_kernel's shape (depth.hip): one thread per read, whole waves, persistent beyond
// 2 048 workgroups, the same three early returns, a mate's length from the batch's offsets.  Two sinks, each off when its pointer is
// null:
//
//   depth      the union of a mate's kept spans into depth mode's difference array.  The spans come sorted by (lo, hi); a running
//              `reach` (the largest hi so far, 0 at first: the clip at the record's start) cuts from each span what earlier ones
//              cover, so the pieces added are disjoint and a base counts once per mate: +1 at gene_start[g] + max(lo, reach),
//              -1 at gene_start[g] + min(hi, len_g), where that piece is not empty.
//   junctions  every consecutive pair (A, B) of the kept spans with pos_B > pos_A into an open-addressing table of 16-byte entries
//              {key, mates, intron}: key = (gene_start[g] + hi_A) << 32 | (gene_start[g] + lo_B), all ones = empty; the entry is
//              claimed with a 64-bit compare-and-swap from empty, linear probing for at most `capacity` steps; then mates += 1 and
//              intron = min(intron, pos_B - pos_A).  A key that finds no entry adds 1 to `dropped`.  A key never changes once it is
//              set and every operation commutes, so the table's CONTENT (not its layout) is independent of scheduling.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "kept_spans.hpp"
#include "shark_internal.hpp"

namespace shk {

namespace {

constexpr int SP_THREADS = 256;

struct SplicedParams {
  const uint32_t *gene_off;
  const uint16_t *gene_ids;
  const uint32_t *counters;
  uint64_t n, cap;                 // reads; associations `entries` holds (segments_kernel's cap)
  const uint64_t *off[2];          // nullptr: the batch has no such mate
  const shk_segment *entries;      // [(j * 2 + mate) * SHK_MAX_SEGMENTS + r]
  const uint64_t *gene_start;
  uint32_t n_genes;                // entries of gene_start - 1
  uint32_t k;
  uint32_t skip_if_long;
  // depth sink
  uint32_t depth_min;
  uint32_t *diff;
  unsigned long long *mates;
  // junction sink
  uint32_t junc_min;
  JunctionEntry *tab;
  uint64_t tab_mask;               // capacity - 1 (a power of two)
  unsigned long long *dropped;
};

__device__ __forceinline__ uint64_t sp_wave_sum_u64(uint64_t v)
{
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// one observation of `key` with this intron
__device__ __forceinline__ void junction_insert(const SplicedParams &P, uint64_t key, uint32_t intron)
{
  uint64_t h = ((key * 0x9E3779B97F4A7C15ull) >> 20) & P.tab_mask;
  for (uint64_t step = 0; step <= P.tab_mask; ++step) {
    JunctionEntry *e = P.tab + h;
    unsigned long long cur = __hip_atomic_load(&e->key, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // (a key is set once: only `empty` can be stale, and the swap settles that)
    if (cur == JUNCTION_EMPTY) {
      cur = atomicCAS(&e->key, JUNCTION_EMPTY, (unsigned long long)key);
      if (cur == JUNCTION_EMPTY) cur = key;
    }
    if (cur == key) {
      atomicAdd(&e->mates, 1u);
      atomicMin(&e->intron, intron);
      return;
    }
    h = (h + 1) & P.tab_mask;
  }
  atomicAdd(P.dropped, 1ull);
}

// One thread per read, persistent.  The loop runs in whole waves (`base` is wave-uniform), so every lane reaches the reduction.
__global__ __launch_bounds__(SP_THREADS) void spliced_accumulate_kernel(const SplicedParams P)
{
  // the batch will be assembled again and comes through here again; or it will be refused in wait (depth_accumulate_kernel's rule)
  if (P.counters[CTR_OVERFLOW] || (P.skip_if_long && P.counters[CTR_LONG]) || P.counters[CTR_VOUCH_BAD]) return;
  const uint32_t lane = threadIdx.x & 63u;
  const uint64_t stride = (uint64_t)gridDim.x * SP_THREADS;
  uint64_t counted = 0;
  for (uint64_t base = (uint64_t)blockIdx.x * SP_THREADS + (threadIdx.x & ~63u); base < P.n; base += stride) {
    const uint64_t i = base + lane;
    if (i >= P.n) continue;
    const uint32_t o0 = P.gene_off[i], o1 = P.gene_off[i + 1];
    if (o1 <= o0 || o1 > P.cap) continue;
    uint32_t L[2] = {0u, 0u};
#pragma unroll
    for (int m = 0; m < 2; ++m)
      if (P.off[m]) {
        const uint64_t len = P.off[m][i + 1] - P.off[m][i];
        L[m] = len > 0x7FFFFFFFull ? 0x7FFFFFFFu : (uint32_t)len;   // (segments_kernel's L)
      }
    for (uint32_t j = o0; j < o1; ++j) {
      const uint32_t g = P.gene_ids[j];
      if (g >= P.n_genes) continue;
      const uint64_t start = P.gene_start[g];
      const int64_t len_g = (int64_t)(P.gene_start[g + 1] - start);
#pragma unroll
      for (int m = 0; m < 2; ++m) {
        const shk_segment *e = P.entries + ((uint64_t)j * 2u + (uint32_t)m) * SHK_MAX_SEGMENTS;
        if (P.diff) {
          const KeptSpans S = kept_spans(e, L[m], P.k, P.depth_min);
          int64_t reach = 0;
          bool added = false;
#pragma unroll
          for (int r = 0; r < SHK_MAX_SEGMENTS; ++r)
            if ((uint32_t)r < S.n) {
              const int64_t lo = S.lo[r] > reach ? (int64_t)S.lo[r] : reach;
              const int64_t hi = S.hi[r] < len_g ? (int64_t)S.hi[r] : len_g;
              if (hi > lo) {
                atomicAdd(&P.diff[start + (uint64_t)lo], 1u);
                atomicAdd(&P.diff[start + (uint64_t)hi], 0xFFFFFFFFu);
                added = true;
              }
              reach = hi > reach ? hi : reach;
            }
          counted += added ? 1u : 0u;
        }
        if (P.tab) {
          const KeptSpans S = kept_spans(e, L[m], P.k, P.junc_min);
#pragma unroll
          for (int r = 0; r + 1 < SHK_MAX_SEGMENTS; ++r)
            if ((uint32_t)r + 1u < S.n && S.pos[r + 1] > S.pos[r]) {
              const int64_t donor = S.hi[r], acceptor = S.lo[r + 1];
              // (a span is a union of record windows: 0 <= lo, hi <= len_g; anything else is not stored)
              if (donor >= 0 && donor <= len_g && acceptor >= 0 && acceptor < len_g)
                junction_insert(P, (start + (uint64_t)donor) << 32 | (start + (uint64_t)acceptor), (uint32_t)((int64_t)S.pos[r + 1] - (int64_t)S.pos[r]));
            }
        }
      }
    }
  }
  if (P.diff) {
    counted = sp_wave_sum_u64(counted);
    if (lane == 0 && counted) atomicAdd(P.mates, (unsigned long long)counted);
  }
}

__global__ __launch_bounds__(256) void junction_clear_kernel(JunctionEntry *__restrict__ tab, uint64_t capacity, unsigned long long *__restrict__ dropped)
{
  const uint64_t tid = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x, nth = (uint64_t)gridDim.x * blockDim.x;
  for (uint64_t i = tid; i < capacity; i += nth) {
    JunctionEntry e;
    e.key = JUNCTION_EMPTY;
    e.mates = 0u;
    e.intron = 0xFFFFFFFFu;
    tab[i] = e;
  }
  if (tid == 0) *dropped = 0ull;
}

}  // namespace

int launch_spliced_accumulate(Ctx *ctx, const Slot &s, const shk_segment *entries, uint64_t cap_assoc, bool skip_if_long, hipStream_t stream)
{
  const DeviceIndex &ix = ctx->idx;
  const bool depth = s.sp_depth != 0, junc = s.sp_junc != 0;
  if (!ix.gene_start || !entries || (depth && (!ctx->depth.counts.p || !ctx->depth.mates.p)) || (junc && (!ctx->junc.tab.p || !ctx->junc.dropped.p))) {
    ctx->last_error = "spliced depth / junction table without its state";
    return SHK_ERR_STATE;
  }
  if (s.n == 0 || (!depth && !junc)) return SHK_OK;
  SplicedParams P{};
  P.gene_off = s.d_gene_off.p;
  P.gene_ids = s.d_gene_ids.p;
  P.counters = s.d_counters;
  P.n = s.n;
  P.cap = std::min<uint64_t>(std::min<uint64_t>(s.d_gene_ids.cap, cap_assoc), 0xFFFFFFFFull);   // (launch_segments')
  P.off[0] = s.p.seq1 ? s.p.off1 : nullptr;
  P.off[1] = s.p.seq2 ? s.p.off2 : nullptr;
  P.entries = entries;
  P.gene_start = ix.gene_start;
  P.n_genes = (uint32_t)(ctx->gene_start.size() - 1);
  P.k = s.p.k;
  P.skip_if_long = skip_if_long ? 1u : 0u;
  if (depth) {
    P.depth_min = s.sp_depth;
    P.diff = ctx->depth.counts.p;
    P.mates = ctx->depth.mates.p;
    ctx->depth.scan_current = false;
  }
  if (junc) {
    P.junc_min = s.sp_junc;
    P.tab = ctx->junc.tab.p;
    P.tab_mask = ctx->junc.tab.cap - 1;
    P.dropped = ctx->junc.dropped.p;
  }
  // one thread per read up to 2 048 workgroups, persistent beyond (launch_depth_accumulate's bound)
  const uint64_t want = (s.n + SP_THREADS - 1) / SP_THREADS;
  hipLaunchKernelGGL(spliced_accumulate_kernel, dim3((unsigned)std::min<uint64_t>(want, 2048)), dim3(SP_THREADS), 0, stream, P);
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? SHK_OK : set_hip_error(ctx, e, "spliced_accumulate_kernel");
}

int launch_junction_clear(Ctx *ctx)
{
  const uint64_t cap = ctx->junc.tab.cap, want = (cap + 255) / 256;
  hipLaunchKernelGGL(junction_clear_kernel, dim3((unsigned)std::min<uint64_t>(want, 2048)), dim3(256), 0, ctx->stream, ctx->junc.tab.p, cap, ctx->junc.dropped.p);
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? SHK_OK : set_hip_error(ctx, e, "junction_clear_kernel");
}

}  // namespace shk
