// device_scan.hip -- kernels behind device_scan.hpp (exclusive prefix sum, gfx950).
#include "device_scan.hpp"
#include "shark_internal.hpp"   // CTR_*: the counter block that the one-record form fills in

namespace shk {

static_assert(SCAN_ITEMS == 16 && SCAN_THREADS == 256, "the kernels below load four uint4 per thread and combine four waves");

// the 16 items of a thread: vector accesses when the tile is whole and the pointer aligned, else item by item (0 behind n)
template <bool VEC>
__device__ __forceinline__ void load_items(const uint32_t *__restrict__ in, uint64_t base, uint64_t n, uint32_t (&v)[SCAN_ITEMS])
{
  if (VEC && base + SCAN_ITEMS <= n) {
    const uint4 *p = reinterpret_cast<const uint4 *>(in + base);
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const uint4 a = p[q];
      v[4 * q] = a.x; v[4 * q + 1] = a.y; v[4 * q + 2] = a.z; v[4 * q + 3] = a.w;
    }
  } else {
#pragma unroll
    for (int i = 0; i < SCAN_ITEMS; ++i) v[i] = base + i < n ? in[base + i] : 0u;
  }
}

__device__ __forceinline__ uint64_t wave_sum_u64(uint64_t v)
{
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// inclusive scan of one 32-bit value per lane across the wave (modulo 2^32)
__device__ __forceinline__ uint32_t wave_inclusive_scan_u32(uint32_t v)
{
  const int lane = threadIdx.x & 63;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const uint32_t t = __shfl_up(v, o, 64);
    if (lane >= o) v += t;
  }
  return v;
}

template <bool VEC>
__global__ __launch_bounds__(SCAN_THREADS) void scan_tile_sums_kernel(const uint32_t *__restrict__ in, uint64_t n, uint64_t *__restrict__ tile_sums)
{
  __shared__ uint64_t lds[SCAN_THREADS / 64];
  const uint64_t base = (uint64_t)blockIdx.x * SCAN_TILE + (uint64_t)threadIdx.x * SCAN_ITEMS;
  uint32_t v[SCAN_ITEMS];
  load_items<VEC>(in, base, n, v);
  uint64_t s = 0;
#pragma unroll
  for (int i = 0; i < SCAN_ITEMS; ++i) s += v[i];
  s = wave_sum_u64(s);
  if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) tile_sums[blockIdx.x] = lds[0] + lds[1] + lds[2] + lds[3];
}

// one workgroup of 1024 threads: exclusive scan of the tile sums in place (each thread a run of consecutive tiles); total -> *total_out
constexpr int SCAN_OFFS_THREADS = 1024;
__global__ __launch_bounds__(SCAN_OFFS_THREADS) void scan_tile_offsets_kernel(uint64_t *__restrict__ tile_sums, uint64_t ntiles, uint64_t *__restrict__ total_out)
{
  __shared__ uint64_t lds[SCAN_OFFS_THREADS / 64];
  const uint64_t per = (ntiles + SCAN_OFFS_THREADS - 1) / SCAN_OFFS_THREADS;
  const uint64_t lo = (uint64_t)threadIdx.x * per, hi = lo + per < ntiles ? lo + per : ntiles;
  uint64_t s = 0;
  for (uint64_t i = lo; i < hi; ++i) s += tile_sums[i];
  // inclusive scan of the threads' sums: within the wave, then over the 16 wave totals
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  uint64_t inc = s;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const uint64_t t = __shfl_up(inc, o, 64);
    if (lane >= o) inc += t;
  }
  if (lane == 63) lds[wave] = inc;
  __syncthreads();
  uint64_t add = 0, tot = 0;
#pragma unroll
  for (int w = 0; w < SCAN_OFFS_THREADS / 64; ++w) {
    const uint64_t t = lds[w];
    if (w < wave) add += t;
    tot += t;
  }
  uint64_t run = add + inc - s;
  for (uint64_t i = lo; i < hi; ++i) {
    const uint64_t t = tile_sums[i];
    tile_sums[i] = run;
    run += t;
  }
  if (threadIdx.x == 0) *total_out = tot;
}

template <bool VEC>
__global__ __launch_bounds__(SCAN_THREADS) void scan_apply_kernel(const uint32_t *__restrict__ in, uint32_t *__restrict__ out, uint64_t n,
                                                                 const uint64_t *__restrict__ tile_offs)
{
  __shared__ uint32_t lds[SCAN_THREADS / 64];
  const uint64_t base = (uint64_t)blockIdx.x * SCAN_TILE + (uint64_t)threadIdx.x * SCAN_ITEMS;
  uint32_t v[SCAN_ITEMS];
  load_items<VEC>(in, base, n, v);
  uint32_t s = 0;
#pragma unroll
  for (int i = 0; i < SCAN_ITEMS; ++i) s += v[i];
  // (the outputs are 32-bit: everything below is modulo 2^32; the 64-bit total comes from the tile sums)
  const uint32_t inc = wave_inclusive_scan_u32(s);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 63) lds[wave] = inc;
  __syncthreads();
  uint32_t add = 0;
#pragma unroll
  for (int w = 0; w < SCAN_THREADS / 64; ++w) add += w < wave ? lds[w] : 0u;
  uint32_t run = (uint32_t)tile_offs[blockIdx.x] + add + inc - s;
#pragma unroll
  for (int i = 0; i < SCAN_ITEMS; ++i) {
    const uint32_t t = v[i];
    v[i] = run;
    run += t;
  }
  if (VEC && base + SCAN_ITEMS <= n) {
    uint4 *p = reinterpret_cast<uint4 *>(out + base);
#pragma unroll
    for (int q = 0; q < 4; ++q) p[q] = make_uint4(v[4 * q], v[4 * q + 1], v[4 * q + 2], v[4 * q + 3]);
  } else {
#pragma unroll
    for (int i = 0; i < SCAN_ITEMS; ++i)
      if (base + i < n) out[base + i] = v[i];
  }
}

// exclusive scan in -> out (may alias); returns the device pointer holding the 64-bit total
const uint64_t *exclusive_scan_u32(const uint32_t *in, uint32_t *out, uint64_t n, uint64_t *temp, hipStream_t stream)
{
  const uint64_t ntiles = (n + SCAN_TILE - 1) / SCAN_TILE;
  uint64_t *total = temp + ntiles;
  if (n == 0) {
    (void)hipMemsetAsync(total, 0, sizeof(uint64_t), stream);
    return total;
  }
  const bool vec = ((reinterpret_cast<uintptr_t>(in) | reinterpret_cast<uintptr_t>(out)) & 15u) == 0;
  if (vec) hipLaunchKernelGGL(scan_tile_sums_kernel<true>, dim3((unsigned)ntiles), dim3(SCAN_THREADS), 0, stream, in, n, temp);
  else hipLaunchKernelGGL(scan_tile_sums_kernel<false>, dim3((unsigned)ntiles), dim3(SCAN_THREADS), 0, stream, in, n, temp);
  hipLaunchKernelGGL(scan_tile_offsets_kernel, dim3(1), dim3(SCAN_OFFS_THREADS), 0, stream, temp, ntiles, total);
  if (vec) hipLaunchKernelGGL(scan_apply_kernel<true>, dim3((unsigned)ntiles), dim3(SCAN_THREADS), 0, stream, in, out, n, temp);
  else hipLaunchKernelGGL(scan_apply_kernel<false>, dim3((unsigned)ntiles), dim3(SCAN_THREADS), 0, stream, in, out, n, temp);
  return total;
}

// ---------------------------------------------------------------------------
// The one-record form (device_scan.hpp, OneRecordResult).  The two kernels below are scan_tile_offsets_kernel and scan_apply_kernel
// with something behind them.  They repeat those kernels' text instead of sharing it through a function: the index build, the sort and
// the depth / variants read-outs run the kernels above, and moving their bodies changed the order of their instructions.
// ---------------------------------------------------------------------------
// the thread that writes the total does finalize_total_kernel's job, and gene_hist_kernel's as well -- every association is gene 0's
__global__ __launch_bounds__(SCAN_OFFS_THREADS) void scan_tile_offsets_one_kernel(uint64_t *__restrict__ tile_sums, uint64_t ntiles, uint64_t *__restrict__ total_out,
                                                                                  uint32_t *__restrict__ counters, uint64_t gene_ids_cap, uint32_t count_genes,
                                                                                  uint32_t skip_if_long, unsigned long long *__restrict__ gene_counts,
                                                                                  const uint32_t *__restrict__ spec_verdict, uint32_t spec_L1, uint32_t spec_L2)
{
  __shared__ uint64_t lds[SCAN_OFFS_THREADS / 64];
  const uint64_t per = (ntiles + SCAN_OFFS_THREADS - 1) / SCAN_OFFS_THREADS;
  const uint64_t lo = (uint64_t)threadIdx.x * per, hi = lo + per < ntiles ? lo + per : ntiles;
  uint64_t s = 0;
  for (uint64_t i = lo; i < hi; ++i) s += tile_sums[i];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  uint64_t inc = s;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const uint64_t t = __shfl_up(inc, o, 64);
    if (lane >= o) inc += t;
  }
  if (lane == 63) lds[wave] = inc;
  __syncthreads();
  uint64_t add = 0, tot = 0;
#pragma unroll
  for (int w = 0; w < SCAN_OFFS_THREADS / 64; ++w) {
    const uint64_t t = lds[w];
    if (w < wave) add += t;
    tot += t;
  }
  uint64_t run = add + inc - s;
  for (uint64_t i = lo; i < hi; ++i) {
    const uint64_t t = tile_sums[i];
    tile_sums[i] = run;
    run += t;
  }
  if (threadIdx.x != 0) return;
  *total_out = tot;
  const bool overflow = tot > gene_ids_cap;
  counters[CTR_ASSOC_LO] = (uint32_t)tot;
  counters[CTR_ASSOC_HI] = (uint32_t)(tot >> 32);
  counters[CTR_OVERFLOW] = overflow ? 1u : 0u;
  // a speculated batch (OneRecordResult::spec_verdict): uniform_check_kernel's words are final by now.  Not uniform, or of other
  // lengths than the classify launch assumed: the counts scanned here mean nothing.  The host sees the word, runs the batch again
  // and this kernel counts it then
  bool miss = false;
  if (spec_verdict) {
    miss = spec_verdict[0] != 1u || spec_verdict[1] != spec_L1 || spec_verdict[2] != spec_L2;
    if (miss) counters[CTR_SPEC_MISS] = 1u;
  }
  // (gene_hist_kernel's rule: a batch that the host finishes by its slow path comes through here again and is counted then)
  if (count_genes && !overflow && !miss && !(skip_if_long && counters[CTR_LONG]) && tot) atomicAdd(&gene_counts[0], (unsigned long long)tot);
}

// the tile's associations are all gene 0's, and the workgroup writes them: ids [tile_offs[b], tile_offs[b] + the tile's sum), cut at
// gene_ids_cap; none when the batch overflows (the epilogue above has set the flag).  Coalesced: 16 bytes per lane between a head
// that reaches the first 16-byte boundary and a tail, both of fewer than 8 ids
template <bool VEC>
__global__ __launch_bounds__(SCAN_THREADS) void scan_apply_fill_kernel(const uint32_t *__restrict__ in, uint32_t *__restrict__ out, uint64_t n,
                                                                      const uint64_t *__restrict__ tile_offs, uint16_t *__restrict__ gene_ids, uint64_t gene_ids_cap,
                                                                      const uint32_t *__restrict__ counters)
{
  __shared__ uint32_t lds[SCAN_THREADS / 64];
  const uint64_t base = (uint64_t)blockIdx.x * SCAN_TILE + (uint64_t)threadIdx.x * SCAN_ITEMS;
  uint32_t v[SCAN_ITEMS];
  load_items<VEC>(in, base, n, v);
  uint32_t s = 0;
#pragma unroll
  for (int i = 0; i < SCAN_ITEMS; ++i) s += v[i];
  const uint32_t inc = wave_inclusive_scan_u32(s);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 63) lds[wave] = inc;
  __syncthreads();
  uint32_t add = 0, tile = 0;   // tile: the tile's sum (a tile of 0 / 1 counts: at most SCAN_TILE)
#pragma unroll
  for (int w = 0; w < SCAN_THREADS / 64; ++w) {
    add += w < wave ? lds[w] : 0u;
    tile += lds[w];
  }
  const uint64_t off = tile_offs[blockIdx.x];
  uint32_t run = (uint32_t)off + add + inc - s;
#pragma unroll
  for (int i = 0; i < SCAN_ITEMS; ++i) {
    const uint32_t t = v[i];
    v[i] = run;
    run += t;
  }
  if (VEC && base + SCAN_ITEMS <= n) {
    uint4 *p = reinterpret_cast<uint4 *>(out + base);
#pragma unroll
    for (int q = 0; q < 4; ++q) p[q] = make_uint4(v[4 * q], v[4 * q + 1], v[4 * q + 2], v[4 * q + 3]);
  } else {
#pragma unroll
    for (int i = 0; i < SCAN_ITEMS; ++i)
      if (base + i < n) out[base + i] = v[i];
  }
  if (counters[CTR_OVERFLOW]) return;
  const uint64_t lo = off < gene_ids_cap ? off : gene_ids_cap;
  const uint64_t hi = tile < gene_ids_cap - lo ? lo + tile : gene_ids_cap;
  uint64_t head = ((16u - (uint32_t)(reinterpret_cast<uintptr_t>(gene_ids + lo) & 15u)) & 15u) / 2;
  if (head > hi - lo) head = hi - lo;
  if (threadIdx.x < head) gene_ids[lo + threadIdx.x] = 0;
  const uint64_t body = lo + head, n8 = (hi - body) / 8;
  uint4 *p8 = reinterpret_cast<uint4 *>(gene_ids + body);
  for (uint64_t i = threadIdx.x; i < n8; i += SCAN_THREADS) p8[i] = make_uint4(0u, 0u, 0u, 0u);
  const uint64_t tail = body + 8 * n8;
  if (threadIdx.x < hi - tail) gene_ids[tail + threadIdx.x] = 0;
}

// the same three launches as exclusive_scan_u32, with the epilogue and the fill; n >= 1
const uint64_t *exclusive_scan_assemble_one(const uint32_t *count, uint32_t *gene_off, uint64_t n, uint64_t *temp, const OneRecordResult &r,
                                            hipStream_t stream)
{
  const uint64_t ntiles = (n + SCAN_TILE - 1) / SCAN_TILE;
  uint64_t *total = temp + ntiles;
  const bool vec = ((reinterpret_cast<uintptr_t>(count) | reinterpret_cast<uintptr_t>(gene_off)) & 15u) == 0;
  if (vec) hipLaunchKernelGGL(scan_tile_sums_kernel<true>, dim3((unsigned)ntiles), dim3(SCAN_THREADS), 0, stream, count, n, temp);
  else hipLaunchKernelGGL(scan_tile_sums_kernel<false>, dim3((unsigned)ntiles), dim3(SCAN_THREADS), 0, stream, count, n, temp);
  hipLaunchKernelGGL(scan_tile_offsets_one_kernel, dim3(1), dim3(SCAN_OFFS_THREADS), 0, stream, temp, ntiles, total, r.counters, r.gene_ids_cap,
                     r.count_genes ? 1u : 0u, r.skip_if_long ? 1u : 0u, r.gene_counts, r.spec_verdict, r.spec_L1, r.spec_L2);
  if (vec) hipLaunchKernelGGL(scan_apply_fill_kernel<true>, dim3((unsigned)ntiles), dim3(SCAN_THREADS), 0, stream, count, gene_off, n, temp, r.gene_ids,
                              r.gene_ids_cap, r.counters);
  else hipLaunchKernelGGL(scan_apply_fill_kernel<false>, dim3((unsigned)ntiles), dim3(SCAN_THREADS), 0, stream, count, gene_off, n, temp, r.gene_ids,
                          r.gene_ids_cap, r.counters);
  return total;
}

}  // namespace shk
