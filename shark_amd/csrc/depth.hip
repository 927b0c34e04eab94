// depth.hip -- depth mode's kernels (gfx950): per-base read depth along each gene, accumulated on the device over all counted
// batches (include/shark_hip.h, "depth").
//
// State: a DIFFERENCE ARRAY over all bases of the records that carry an id, gene g at [gene_start[g], gene_start[g + 1]), plus one
// entry.  A counted mate that covers [lo, hi) of gene g adds +1 at gene_start[g] + lo and -1 (modulo 2^32) at gene_start[g] + hi:
// two no-return atomic adds, whatever the mate's length.  Addition commutes, so the array does not depend on the order in which
// mates, batches or contexts arrive.  hi = len_g lands on the next gene's first entry (or on the spare entry): right for ONE prefix
// sum over the whole array, since every interval's +1 and -1 have both been passed at any later base.
//
// Read-out: depth[x] = the inclusive prefix sum of the difference array at x, modulo 2^32.  device_scan.hpp scans exclusively, so
// the array is scanned over ALL its entries (the spare one included) into a second array of the same size, and
// depth[x] = scan[x + 1].  The element count is 64-bit there and the grid (entries / 4096) stays far below 2^31: no chunking.
//
// Summary: per gene {len, covered, max, sum}, one workgroup of 256 threads per gene, the workgroups striding over the genes
// (DESIGN.md 10 on the choice).
#include <hip/hip_runtime.h>

#include <algorithm>

#include "device_scan.hpp"
#include "shark_internal.hpp"

namespace shk {

namespace {

constexpr int DP_THREADS = 256;

struct DepthParams {
  const uint32_t *gene_off;
  const uint16_t *gene_ids;
  const uint32_t *counters;
  uint64_t n, cap;                 // reads; records `place` holds (placement_kernel's cap)
  const uint64_t *off[2];          // nullptr: the batch has no such mate
  const shk_placement *place;
  const uint64_t *gene_start;
  uint32_t n_genes;                // entries of gene_start - 1
  uint32_t min_support;
  uint32_t skip_if_long;
  uint32_t *diff;
  unsigned long long *mates;
};

__device__ __forceinline__ uint64_t dp_wave_sum_u64(uint64_t v)
{
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// One thread per read, persistent.  The loop runs in whole waves (`base` is wave-uniform), so every lane reaches the reduction.
__global__ __launch_bounds__(DP_THREADS) void depth_accumulate_kernel(const DepthParams P)
{
  // the batch will be assembled again (gene_hist_kernel's rule) and comes through here again; or it will be refused in wait
  if (P.counters[CTR_OVERFLOW] || (P.skip_if_long && P.counters[CTR_LONG]) || P.counters[CTR_VOUCH_BAD]) return;
  const uint32_t lane = threadIdx.x & 63u;
  const uint64_t stride = (uint64_t)gridDim.x * DP_THREADS;
  uint64_t counted = 0;
  for (uint64_t base = (uint64_t)blockIdx.x * DP_THREADS + (threadIdx.x & ~63u); base < P.n; base += stride) {
    const uint64_t i = base + lane;
    if (i >= P.n) continue;
    const uint32_t o0 = P.gene_off[i], o1 = P.gene_off[i + 1];
    if (o1 <= o0 || o1 > P.cap) continue;
    uint32_t L[2] = {0u, 0u};
#pragma unroll
    for (int m = 0; m < 2; ++m)
      if (P.off[m]) {
        const uint64_t len = P.off[m][i + 1] - P.off[m][i];
        L[m] = len > 0x7FFFFFFFull ? 0x7FFFFFFFu : (uint32_t)len;   // (placement_kernel's L)
      }
    for (uint32_t j = o0; j < o1; ++j) {
      const uint32_t g = P.gene_ids[j];
      if (g >= P.n_genes) continue;
      const uint64_t start = P.gene_start[g];
      const int64_t len_g = (int64_t)(P.gene_start[g + 1] - start);
#pragma unroll
      for (int m = 0; m < 2; ++m) {
        const shk_mate_placement r = P.place[j].mate[m];
        if (r.support < P.min_support) continue;
        const int64_t pos = r.pos;
        const int64_t lo = pos > 0 ? pos : 0;
        const int64_t end = pos + (int64_t)L[m];
        const int64_t hi = end < len_g ? end : len_g;
        if (hi <= lo) continue;
        atomicAdd(&P.diff[start + (uint64_t)lo], 1u);
        atomicAdd(&P.diff[start + (uint64_t)hi], 0xFFFFFFFFu);
        ++counted;
      }
    }
  }
  counted = dp_wave_sum_u64(counted);
  if (lane == 0 && counted) atomicAdd(P.mates, (unsigned long long)counted);
}

// {len, covered, max, sum} of gene g over depth[gene_start[g] .. gene_start[g + 1]): wave reduce, then the four waves through LDS
__global__ __launch_bounds__(DP_THREADS) void depth_summary_kernel(const uint32_t *__restrict__ depth, const uint64_t *__restrict__ gene_start, uint32_t n_genes,
                                                                   shk_gene_depth *__restrict__ out)
{
  __shared__ uint64_t s_sum[DP_THREADS / 64];
  __shared__ uint32_t s_cov[DP_THREADS / 64], s_max[DP_THREADS / 64];
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  for (uint32_t g = blockIdx.x; g < n_genes; g += gridDim.x) {
    const uint64_t a = gene_start[g], b = gene_start[g + 1];
    uint64_t sum = 0;
    uint32_t cov = 0, mx = 0;
    for (uint64_t x = a + threadIdx.x; x < b; x += DP_THREADS) {
      const uint32_t d = depth[x];
      sum += d;
      cov += d != 0u;
      mx = d > mx ? d : mx;
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
      sum += __shfl_xor(sum, o, 64);
      cov += __shfl_xor(cov, o, 64);
      const uint32_t t = __shfl_xor(mx, o, 64);
      mx = t > mx ? t : mx;
    }
    if (lane == 0) { s_sum[wave] = sum; s_cov[wave] = cov; s_max[wave] = mx; }
    __syncthreads();
    if (threadIdx.x == 0) {
      shk_gene_depth r;
      r.len = (uint32_t)(b - a);
      r.covered = s_cov[0] + s_cov[1] + s_cov[2] + s_cov[3];
      r.max = std::max(std::max(s_max[0], s_max[1]), std::max(s_max[2], s_max[3]));
      r.pad = 0;
      r.sum = s_sum[0] + s_sum[1] + s_sum[2] + s_sum[3];
      out[g] = r;
    }
    __syncthreads();   // (the next gene's partial results overwrite the LDS words)
  }
}

}  // namespace

int launch_depth_accumulate(Ctx *ctx, const Slot &s, bool skip_if_long, hipStream_t stream)
{
  const DeviceIndex &ix = ctx->idx;
  if (!ix.gene_start || !ctx->depth.counts.p || !ctx->depth.mates.p || !s.rec_place.d.p) { ctx->last_error = "depth mode without its state"; return SHK_ERR_STATE; }
  if (s.n == 0) return SHK_OK;
  DepthParams P{};
  P.gene_off = s.d_gene_off.p;
  P.gene_ids = s.d_gene_ids.p;
  P.counters = s.d_counters;
  P.n = s.n;
  P.cap = std::min<uint64_t>(std::min<uint64_t>(s.d_gene_ids.cap, s.rec_place.d.cap), 0xFFFFFFFFull);   // (launch_placement's)
  P.off[0] = s.p.seq1 ? s.p.off1 : nullptr;
  P.off[1] = s.p.seq2 ? s.p.off2 : nullptr;
  P.place = s.rec_place.d.p;
  P.gene_start = ix.gene_start;
  P.n_genes = (uint32_t)(ctx->gene_start.size() - 1);
  P.min_support = s.depth;
  P.skip_if_long = skip_if_long ? 1u : 0u;
  P.diff = ctx->depth.counts.p;
  P.mates = ctx->depth.mates.p;
  // one thread per read up to 2 048 workgroups (launch_placement's bound), persistent beyond
  const uint64_t want = (s.n + DP_THREADS - 1) / DP_THREADS;
  ctx->depth.scan_current = false;
  hipLaunchKernelGGL(depth_accumulate_kernel, dim3((unsigned)std::min<uint64_t>(want, 2048)), dim3(DP_THREADS), 0, stream, P);
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? SHK_OK : set_hip_error(ctx, e, "depth_accumulate_kernel");
}

int depth_scan(Ctx *ctx)
{
  const uint64_t entries = ctx->gene_start.back() + 1;
  // (no batch has added to the state since the last scan: a caller that reads gene after gene pays for one scan)
  DepthState &D = ctx->depth;
  if (D.scan_current) return SHK_OK;
  int rc;
  if (!D.scan.p && (rc = D.scan.alloc_exact(ctx, entries))) return rc;
  if (!D.scan_temp.p && (rc = D.scan_temp.alloc_exact(ctx, scan_temp_words(entries)))) return rc;
  (void)exclusive_scan_u32(D.counts.p, D.scan.p, entries, D.scan_temp.p, ctx->stream);
  SHK_HIP(ctx, hipGetLastError());
  D.scan_current = true;
  return SHK_OK;
}

int launch_depth_summary(Ctx *ctx)
{
  const uint32_t n_genes = (uint32_t)(ctx->gene_start.size() - 1);
  if (n_genes == 0) return SHK_OK;
  DepthState &D = ctx->depth;
  if (!D.summary.p)
    if (const int rc = D.summary.alloc_exact(ctx, n_genes)) return rc;
  hipLaunchKernelGGL(depth_summary_kernel, dim3(std::min<uint32_t>(n_genes, 2048u)), dim3(DP_THREADS), 0, ctx->stream, (const uint32_t *)(D.scan.p + 1),
                     (const uint64_t *)ctx->idx.gene_start, n_genes, D.summary.p);
  SHK_HIP(ctx, hipGetLastError());
  return SHK_OK;
}

}  // namespace shk
