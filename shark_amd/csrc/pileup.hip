// pileup.hip -- pileup mode's kernel (gfx950): per record base, how many counted mates show A, C, G or T there (include/shark_hip.h,
// "pileup").  The third consumer of segments mode on the device: it turns a mate's KEPT SPANS (kept_spans.hpp) back into
// the mate's bytes, behind segments_kernel's records at m = SHK_MAX_SEGMENTS in the batch's tail.
//
// placement_kernel's and segments_kernel's outer shape: one wavefront per read with associations, persistent beyond 2 048 workgroups;
// spliced_accumulate_kernel's three early returns and its walk over the sorted spans with a running `reach`, so the owned pieces are
// exactly the pieces spliced depth adds.  Everything up to a piece's bounds is wave-uniform (the read, its associations, a mate's four
// 20-byte records, its kept spans): scalar work.  Per owned piece the lanes take 64 consecutive record coordinates per pass; a lane
// loads its one byte of the mate (ascending addresses on strand 0, descending on strand 1: one or two 64-byte lines per pass either
// way), applies the -q mask as pl_window does, and issues ONE atomic add without a return value on counts[(gene_start[g] + x) * 4 + b].
// The four counters of a base share 16 bytes, so a pass touches 16 consecutive 64-byte lines of the state.  No LDS, nothing capped.
//
// Pileup mates are wave-uniform too: counted in a scalar, one 64-bit atomic per wave at the end.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "kept_spans.hpp"
#include "placement_common.hpp"
#include "shark_internal.hpp"

namespace shk {

namespace {

struct PileupParams {
  const uint32_t *gene_off;
  const uint16_t *gene_ids;
  const uint32_t *counters;
  uint64_t n, cap;                 // reads; associations `entries` holds (segments_kernel's cap)
  const uint8_t *seq[2];           // nullptr: the batch has no such mate
  const uint64_t *off[2];
  const uint8_t *qual[2];          // nullptr: no masking
  int32_t mq;
  uint32_t k;
  const shk_segment *entries;      // [(j * 2 + mate) * SHK_MAX_SEGMENTS + r]
  const uint64_t *gene_start;
  uint32_t n_genes;                // entries of gene_start - 1
  uint32_t skip_if_long;
  uint32_t s_min;
  uint32_t *counts;                // [(gene_start[g] + x) * 4 + b]
  unsigned long long *mates;
};

__global__ __launch_bounds__(PL_THREADS) void pileup_kernel(const PileupParams P)
{
  // the batch will be assembled again and comes through here again; or it will be refused in wait (spliced_accumulate_kernel's rule)
  if (P.counters[CTR_OVERFLOW] || (P.skip_if_long && P.counters[CTR_LONG]) || P.counters[CTR_VOUCH_BAD]) return;
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);   // (the same in every lane: what follows from it is scalar)
  const uint64_t n_waves = (uint64_t)gridDim.x * PL_WAVES;
  uint64_t counted = 0;
  for (uint64_t i = (uint64_t)blockIdx.x * PL_WAVES + wave; i < P.n; i += n_waves) {
    const uint32_t o0 = P.gene_off[i], o1 = P.gene_off[i + 1];
    if (o1 <= o0 || o1 > P.cap) continue;
    for (uint32_t m = 0; m < 2; ++m) {
      if (!P.seq[m]) continue;
      const uint64_t a = P.off[m][i], len = P.off[m][i + 1] - a;
      const uint32_t L = len > 0x7FFFFFFFull ? 0x7FFFFFFFu : (uint32_t)len;   // (segments_kernel's L)
      const uint8_t *const seq = P.seq[m] + a;
      const uint8_t *const qual = P.qual[m] ? P.qual[m] + a : nullptr;
      for (uint32_t j = o0; j < o1; ++j) {
        const uint32_t g = P.gene_ids[j];
        if (g >= P.n_genes) continue;
        const uint64_t start = P.gene_start[g];
        const int64_t len_g = (int64_t)(P.gene_start[g + 1] - start);
        const shk_segment *e = P.entries + ((uint64_t)j * 2u + m) * SHK_MAX_SEGMENTS;
        const uint32_t strand = e[0].strand;   // (rank 0's: every kept span lies on it)
        const KeptSpans S = kept_spans(e, L, P.k, P.s_min);
        int64_t reach = 0;
        bool owned = false;
#pragma unroll
        for (int r = 0; r < SHK_MAX_SEGMENTS; ++r)
          if ((uint32_t)r < S.n) {
            const int64_t lo = S.lo[r] > reach ? (int64_t)S.lo[r] : reach;
            const int64_t hi = S.hi[r] < len_g ? (int64_t)S.hi[r] : len_g;
            // the mate's byte under record coordinate x: strand 0 at x - pos, strand 1 at pos + L - 1 - x
            const int64_t from = strand ? (int64_t)S.pos[r] + (int64_t)L - 1 : -(int64_t)S.pos[r];
            for (int64_t x0 = lo; x0 < hi; x0 += 64) {
              const int64_t x = x0 + (int64_t)lane;
              const uint64_t idx = (uint64_t)(strand ? from - x : from + x);
              // (a span lies inside [pos, pos + L), so idx < L; the compare keeps a lane inside the mate whatever the records hold)
              if (x < hi && idx < (uint64_t)L) {
                uint32_t ch = seq[idx];
                if (qual && (int32_t)(int8_t)qual[idx] < P.mq) ch = (ch - 64u) & 0xFFu;
                const uint32_t c = base_code(ch);
                if (c < 4u) atomicAdd(&P.counts[(start + (uint64_t)x) * 4u + (strand ? 3u - c : c)], 1u);
              }
            }
            owned = owned || hi > lo;
            reach = hi > reach ? hi : reach;
          }
        counted += owned ? 1u : 0u;
      }
    }
  }
  if (lane == 0 && counted) atomicAdd(P.mates, (unsigned long long)counted);
}

}  // namespace

int launch_pileup(Ctx *ctx, const Slot &s, const shk_segment *entries, uint64_t cap_assoc, bool skip_if_long, hipStream_t stream)
{
  const DeviceIndex &ix = ctx->idx;
  if (!ix.gene_start || !entries || !s.pileup || !ctx->pileup.counts.p || !ctx->pileup.mates.p) {
    ctx->last_error = "pileup mode without its state";
    return SHK_ERR_STATE;
  }
  if (s.n == 0) return SHK_OK;
  PileupParams P{};
  P.gene_off = s.d_gene_off.p;
  P.gene_ids = s.d_gene_ids.p;
  P.counters = s.d_counters;
  P.n = s.n;
  P.cap = std::min<uint64_t>(std::min<uint64_t>(s.d_gene_ids.cap, cap_assoc), 0xFFFFFFFFull);   // (launch_segments')
  P.seq[0] = s.p.seq1; P.off[0] = s.p.off1; P.qual[0] = s.p.hasq ? s.p.qual1 : nullptr;
  P.seq[1] = s.p.seq2; P.off[1] = s.p.off2; P.qual[1] = s.p.hasq ? s.p.qual2 : nullptr;
  P.mq = s.p.mq;
  P.k = s.p.k;
  P.entries = entries;
  P.gene_start = ix.gene_start;
  P.n_genes = (uint32_t)(ctx->gene_start.size() - 1);
  P.skip_if_long = skip_if_long ? 1u : 0u;
  P.s_min = s.pileup;
  P.counts = ctx->pileup.counts.p;
  P.mates = ctx->pileup.mates.p;
  // one wave per read up to 2 048 workgroups, persistent beyond (launch_segments' bound)
  const uint64_t want = (s.n + PL_WAVES - 1) / PL_WAVES;
  hipLaunchKernelGGL(pileup_kernel, dim3((unsigned)std::min<uint64_t>(want, 2048)), dim3(PL_THREADS), 0, stream, P);
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? SHK_OK : set_hip_error(ctx, e, "pileup_kernel");
}

}  // namespace shk
