// variants.hip -- variants mode's kernels (gfx950): the pileup state held against the records' bases on the device (include/shark_hip.h,
// "variants"), and shk_pileup_add's element-wise add.  Read-outs only: nothing here runs in a batch's tail.
//
// All three read-out kernels stream the state once: 16 bytes of counters and 1 byte of DeviceIndex::recbase per record base.  A lane takes
// FOUR consecutive positions -- four 16-byte loads of counters (a base's four counters are one aligned uint4) and one aligned dword of
// recbase --, a wavefront 256 (VR_WAVE_POS), a workgroup of four wavefronts 1 024 (VR_BLOCK_POS).  Position p = wave base + 4 * lane + j.
//
//   variants_count_kernel   evaluates the site predicate, ballots the four sub-positions and stores ONE uint32 per wavefront: its sites.
//   exclusive_scan_u32      over those counts (device_scan.hip; its tile is 4 096 counts = 2^20 positions); the total is the answer's n.
//   variants_write_kernel   evaluates the predicate again, ranks a site inside its wavefront in position order (the ballots of the four
//                           sub-positions below the lane, plus the lane's own lower sub-positions) and stores the 32-byte record at the
//                           wavefront's offset: (gene, x) order with no sort, and n is known before a record is written.  Only a site
//                           looks its gene up (binary search in gene_start for the last g that starts at or in front of p).
//   variants_summary_kernel per gene {observed, mismatches, covered, sites}: a wavefront whose positions lie in one gene (one search, one
//                           compare with the next start) reduces across its lanes and issues at most four atomics; a wavefront that
//                           straddles a boundary searches and adds per position.  The accumulators are cleared per call.
//
// Plain C++ and vector atomics; no LDS.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "device_scan.hpp"
#include "shark_internal.hpp"

namespace shk {

namespace {

constexpr int VR_THREADS = 256;
constexpr uint32_t VR_LANE_POS = 4;                                     // positions per lane: one dword of recbase
constexpr uint32_t VR_WAVE_POS = 64 * VR_LANE_POS;                      // 256
constexpr uint32_t VR_BLOCK_POS = VR_WAVE_POS * (VR_THREADS / 64);      // 1 024
static_assert(sizeof(shk_variant) == 32 && sizeof(shk_gene_variants) == 24, "the records the kernels store");

struct VarParams {
  const uint32_t *counts;      // [p * 4 + b], 16-byte aligned
  const uint8_t *recbase;      // [p], padded to a dword behind `total`
  uint64_t total;              // positions: gene_start[nidx]
  uint32_t min_depth, min_alt, frac_num, frac_den;
};

// the four positions of a lane as they come from memory: r = 4 and counters 0 behind the end
struct LanePos {
  uint4 c[VR_LANE_POS];
  uint32_t r[VR_LANE_POS];
};

__device__ __forceinline__ LanePos vr_load(const VarParams &P, uint64_t p0)
{
  LanePos q;
  const uint32_t rr = p0 < P.total ? *reinterpret_cast<const uint32_t *>(P.recbase + p0) : 0x04040404u;
  const uint4 *c = reinterpret_cast<const uint4 *>(P.counts);
#pragma unroll
  for (uint32_t j = 0; j < VR_LANE_POS; ++j) {
    const bool in = p0 + j < P.total;
    q.c[j] = in ? c[p0 + j] : make_uint4(0u, 0u, 0u, 0u);
    q.r[j] = in ? (rr >> (8u * j)) & 0xFFu : 4u;
  }
  return q;
}

// the header's rule for one position with r < 4: alt = the b != r with the largest n[b], ties to the smallest b; site iff the three hold
__device__ __forceinline__ bool vr_site(const VarParams &P, const uint4 c, uint32_t r, uint32_t &alt, uint64_t &T)
{
  const uint32_t n[4] = {c.x, c.y, c.z, c.w};
  T = (uint64_t)c.x + c.y + c.z + c.w;
  uint32_t a = 4u, best = 0u;
#pragma unroll
  for (uint32_t b = 0; b < 4; ++b)
    if (b != r && (a == 4u || n[b] > best)) { a = b; best = n[b]; }
  alt = a;
  return r < 4u && T >= P.min_depth && best >= P.min_alt && (uint64_t)best * P.frac_den >= (uint64_t)P.frac_num * T;
}

// the last g with gene_start[g] <= p, for p < gene_start[n_genes]: genes without a base share a start with their successor, so g has one
__device__ __forceinline__ uint32_t vr_gene_of(const uint64_t *__restrict__ gs, uint32_t n_genes, uint64_t p)
{
  uint32_t lo = 0, hi = n_genes;   // gs[lo] <= p < gs[hi]
  while (hi - lo > 1u) {
    const uint32_t mid = (lo + hi) >> 1;
    if (gs[mid] <= p) lo = mid; else hi = mid;
  }
  return lo;
}

__global__ __launch_bounds__(VR_THREADS) void variants_count_kernel(const VarParams P, uint32_t *__restrict__ wave_sites)
{
  const uint32_t lane = threadIdx.x & 63u;
  const uint64_t w = (uint64_t)blockIdx.x * (VR_THREADS / 64) + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const uint64_t base = w * VR_WAVE_POS;
  if (base >= P.total) return;
  const LanePos q = vr_load(P, base + (uint64_t)lane * VR_LANE_POS);
  uint32_t sites = 0;
#pragma unroll
  for (uint32_t j = 0; j < VR_LANE_POS; ++j) {
    uint32_t alt;
    uint64_t T;
    sites += (uint32_t)__popcll(__ballot(vr_site(P, q.c[j], q.r[j], alt, T)));
  }
  if (lane == 0) wave_sites[w] = sites;
}

__global__ __launch_bounds__(VR_THREADS) void variants_write_kernel(const VarParams P, const uint32_t *__restrict__ wave_offs, const uint64_t *__restrict__ gene_start,
                                                                    uint32_t n_genes, shk_variant *__restrict__ out, uint64_t n_out)
{
  const uint32_t lane = threadIdx.x & 63u;
  const uint64_t w = (uint64_t)blockIdx.x * (VR_THREADS / 64) + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const uint64_t base = w * VR_WAVE_POS;
  if (base >= P.total) return;
  const uint64_t p0 = base + (uint64_t)lane * VR_LANE_POS;
  const LanePos q = vr_load(P, p0);
  bool site[VR_LANE_POS];
  uint32_t alt[VR_LANE_POS];
  uint32_t below = 0;            // sites of the lanes in front of this one
  const uint64_t lt = (1ull << lane) - 1ull;
#pragma unroll
  for (uint32_t j = 0; j < VR_LANE_POS; ++j) {
    uint64_t T;
    site[j] = vr_site(P, q.c[j], q.r[j], alt[j], T);
    below += (uint32_t)__popcll(__ballot(site[j]) & lt);
  }
  uint64_t at = (uint64_t)wave_offs[w] + below;
#pragma unroll
  for (uint32_t j = 0; j < VR_LANE_POS; ++j)
    if (site[j]) {
      // (at < n_out by construction: the scan's total sized the array; the compare keeps a store inside it whatever the state did meanwhile)
      if (at < n_out) {
        const uint64_t p = p0 + j;
        const uint32_t g = vr_gene_of(gene_start, n_genes, p);
        uint4 *o = reinterpret_cast<uint4 *>(out + at);
        o[0] = make_uint4(g, (uint32_t)(p - gene_start[g]), q.r[j], alt[j]);
        o[1] = q.c[j];
      }
      ++at;
    }
}

__device__ __forceinline__ uint64_t vr_wave_sum(uint64_t v)
{
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

__device__ __forceinline__ void vr_add(shk_gene_variants *o, uint64_t obs, uint64_t mis, uint32_t cov, uint32_t sites)
{
  if (obs) atomicAdd(reinterpret_cast<unsigned long long *>(&o->observed), (unsigned long long)obs);
  if (mis) atomicAdd(reinterpret_cast<unsigned long long *>(&o->mismatches), (unsigned long long)mis);
  if (cov) atomicAdd(&o->covered, cov);
  if (sites) atomicAdd(&o->sites, sites);
}

__global__ __launch_bounds__(VR_THREADS) void variants_summary_kernel(const VarParams P, const uint64_t *__restrict__ gene_start, uint32_t n_genes,
                                                                      shk_gene_variants *__restrict__ out)
{
  const uint32_t lane = threadIdx.x & 63u;
  const uint64_t w = (uint64_t)blockIdx.x * (VR_THREADS / 64) + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const uint64_t base = w * VR_WAVE_POS;
  if (base >= P.total) return;
  const uint64_t end = base + VR_WAVE_POS < P.total ? base + VR_WAVE_POS : P.total;
  const uint64_t p0 = base + (uint64_t)lane * VR_LANE_POS;
  const LanePos q = vr_load(P, p0);
  // (wave-uniform: the gene of the wavefront's first position, and whether its last one lies in it too)
  const uint32_t g0 = vr_gene_of(gene_start, n_genes, base);
  const bool one_gene = gene_start[g0 + 1] >= end;
  uint64_t obs = 0, mis = 0;
  uint32_t cov = 0, sites = 0;
#pragma unroll
  for (uint32_t j = 0; j < VR_LANE_POS; ++j) {
    const uint32_t r = q.r[j];
    if (r >= 4u) continue;          // (no part in anything; positions behind the end come as r = 4)
    uint32_t alt;
    uint64_t T;
    const bool site = vr_site(P, q.c[j], r, alt, T);
    const uint32_t nr = r == 0u ? q.c[j].x : r == 1u ? q.c[j].y : r == 2u ? q.c[j].z : q.c[j].w;
    const uint32_t c1 = T >= P.min_depth ? 1u : 0u, s1 = site ? 1u : 0u;
    if (one_gene) {
      obs += T; mis += T - nr; cov += c1; sites += s1;
    } else {
      vr_add(out + vr_gene_of(gene_start, n_genes, p0 + j), T, T - nr, c1, s1);
    }
  }
  if (one_gene) {
    obs = vr_wave_sum(obs);
    mis = vr_wave_sum(mis);
    const uint64_t both = vr_wave_sum(((uint64_t)cov << 32) | sites);   // (each at most 256: one reduction for the two)
    if (lane == 0) vr_add(out + g0, obs, mis, (uint32_t)(both >> 32), (uint32_t)both);
  }
}

// shk_pileup_add: state[i] += add[i], one base's four counters (16 bytes) per lane and step
__global__ __launch_bounds__(VR_THREADS) void pileup_add_kernel(uint4 *__restrict__ state, const uint4 *__restrict__ add, uint64_t n_bases,
                                                                unsigned long long *__restrict__ mates_ctr, unsigned long long mates)
{
  const uint64_t stride = (uint64_t)gridDim.x * VR_THREADS;
  const uint64_t t = (uint64_t)blockIdx.x * VR_THREADS + threadIdx.x;
  for (uint64_t i = t; i < n_bases; i += stride) {
    uint4 x = state[i];
    const uint4 y = add[i];
    x.x += y.x; x.y += y.y; x.z += y.z; x.w += y.w;
    state[i] = x;
  }
  if (t == 0 && mates) atomicAdd(mates_ctr, mates);
}

VarParams var_params(const Ctx *ctx, const shk_variant_params &prm)
{
  VarParams P{};
  P.counts = ctx->pileup.counts.p;
  P.recbase = ctx->idx.recbase;
  P.total = ctx->gene_start.back();
  P.min_depth = prm.min_depth; P.min_alt = prm.min_alt; P.frac_num = prm.frac_num; P.frac_den = prm.frac_den;
  return P;
}

}  // namespace

int launch_pileup_add(Ctx *ctx, const uint32_t *d_add, uint64_t n_entries, uint64_t mates)
{
  if (!ctx->pileup.counts.p || !ctx->pileup.mates.p) { ctx->last_error = "pileup mode without its state"; return SHK_ERR_STATE; }
  if (n_entries == 0 && mates == 0) return SHK_OK;
  // (the state comes from hipMalloc; a caller's device pointer has to be as aligned as a base's four counters are)
  if (reinterpret_cast<uintptr_t>(d_add) & 15u) { ctx->last_error = "shk_pileup_add: the device pointer is not 16-byte aligned"; return SHK_ERR_ARG; }
  const uint64_t n_bases = n_entries / 4;
  const unsigned grid = (unsigned)std::max<uint64_t>(1, std::min<uint64_t>((n_bases + VR_THREADS - 1) / VR_THREADS, 8192));
  hipLaunchKernelGGL(pileup_add_kernel, dim3(grid), dim3(VR_THREADS), 0, ctx->stream, reinterpret_cast<uint4 *>(ctx->pileup.counts.p), reinterpret_cast<const uint4 *>(d_add), n_bases,
                     ctx->pileup.mates.p, (unsigned long long)mates);
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? SHK_OK : set_hip_error(ctx, e, "pileup_add_kernel");
}

int variants_call(Ctx *ctx, const shk_variant_params &prm, shk_variant *out, uint64_t cap, uint64_t *n_sites)
{
  if (!ctx->pileup.counts.p || !ctx->idx.recbase || !ctx->idx.gene_start) { ctx->last_error = "variants mode without its state"; return SHK_ERR_STATE; }
  const VarParams P = var_params(ctx, prm);
  *n_sites = 0;
  if (P.total == 0) return SHK_OK;
  const uint64_t n_waves = (P.total + VR_WAVE_POS - 1) / VR_WAVE_POS;
  const unsigned grid = (unsigned)((P.total + VR_BLOCK_POS - 1) / VR_BLOCK_POS);   // (total < 2^32: at most 2^22 workgroups)
  // (a property of the index: allocated once)
  VariantScratch &V = ctx->var;
  int rc;
  if (!V.waves.p && (rc = V.waves.alloc_exact(ctx, n_waves))) return rc;
  if (!V.temp.p && (rc = V.temp.alloc_exact(ctx, scan_temp_words(n_waves)))) return rc;
  hipLaunchKernelGGL(variants_count_kernel, dim3(grid), dim3(VR_THREADS), 0, ctx->stream, P, V.waves.p);
  SHK_HIP(ctx, hipGetLastError());
  const uint64_t *d_total = exclusive_scan_u32(V.waves.p, V.waves.p, n_waves, V.temp.p, ctx->stream);
  SHK_HIP(ctx, hipGetLastError());
  uint64_t n = 0;
  SHK_HIP(ctx, hipMemcpyAsync(&n, d_total, sizeof(n), hipMemcpyDeviceToHost, ctx->stream));
  SHK_HIP(ctx, hipStreamSynchronize(ctx->stream));
  *n_sites = n;
  if (!out || n == 0) return SHK_OK;
  if (cap < n) return SHK_ERR_ARG;
  if (V.out.cap < n && (rc = V.out.alloc_exact(ctx, (size_t)n))) return rc;
  hipLaunchKernelGGL(variants_write_kernel, dim3(grid), dim3(VR_THREADS), 0, ctx->stream, P, (const uint32_t *)V.waves.p,
                     (const uint64_t *)ctx->idx.gene_start, (uint32_t)(ctx->gene_start.size() - 1), V.out.p, n);
  SHK_HIP(ctx, hipGetLastError());
  SHK_HIP(ctx, hipMemcpyAsync(out, V.out.p, (size_t)n * sizeof(shk_variant), hipMemcpyDeviceToHost, ctx->stream));
  SHK_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return SHK_OK;
}

int launch_variants_summary(Ctx *ctx, const shk_variant_params &prm)
{
  if (!ctx->pileup.counts.p || !ctx->idx.recbase || !ctx->idx.gene_start) { ctx->last_error = "variants mode without its state"; return SHK_ERR_STATE; }
  const uint32_t n_genes = (uint32_t)(ctx->gene_start.size() - 1);
  if (n_genes == 0) return SHK_OK;
  DevArray<shk_gene_variants> &summary = ctx->var.summary;
  if (!summary.p)
    if (const int rc = summary.alloc_exact(ctx, n_genes)) return rc;
  SHK_HIP(ctx, hipMemsetAsync(summary.p, 0, (size_t)n_genes * sizeof(shk_gene_variants), ctx->stream));
  const VarParams P = var_params(ctx, prm);
  if (P.total == 0) return SHK_OK;
  const unsigned grid = (unsigned)((P.total + VR_BLOCK_POS - 1) / VR_BLOCK_POS);
  hipLaunchKernelGGL(variants_summary_kernel, dim3(grid), dim3(VR_THREADS), 0, ctx->stream, P, (const uint64_t *)ctx->idx.gene_start, n_genes, summary.p);
  SHK_HIP(ctx, hipGetLastError());
  return SHK_OK;
}

}  // namespace shk
