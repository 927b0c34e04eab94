// placement_build.hip -- the table placement mode looks a read's k-mers up in (shk_ref_keep_positions), built on the
// device from the uploaded reference bytes and the record -> gene id mapping of main.cpp:160-187.
//
// It answers "(gene g, canonical k-mer) -> the ONE valid window x of g's record with that canonical k-mer and its orientation, or
// none, or ambiguous" exactly: an entry stores the whole key.  It has nothing to do with the Bloom filter and is built the same
// way for every index kind.
//
//   1. one thread per reference position i: key = pl_hash32(gene, canonical k-mer) << 32 | i (all ones where no valid window starts,
//      or a window that is its own reverse complement)
//   2. radix sort of the keys: equal (gene, k-mer) pairs are now neighbours (with the few other pairs of the same 32-bit hash
//      between them), by ascending position
//   3. head flags: a key is a head iff no key in front of it IN ITS HASH GROUP is the same pair (compared in full, from the bytes);
//      exclusive scan -> the entry's index
//   4. every head writes its entry; it is ambiguous iff a key behind it in its hash group is the same pair
//   5. directory: pdir[b] = first entry of bucket b (top bits of the hash)
// Every step is a function of the sorted keys alone, so the table's bytes do not depend on the order threads run in.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <vector>

#include "device_scan.hpp"
#include "device_sort.hpp"
#include "placement_common.hpp"
#include "shark_internal.hpp"

namespace shk {

namespace {

constexpr uint64_t PL_KEY_NONE = ~0ull;

struct PlWindow {
  uint64_t kmer;    // canonical k-mer | orientation << 63, or PL_NO_KMER
  uint32_t gene;
  uint32_t x;       // offset in the record
};

// the window that starts at global position i (binary search for its record)
__device__ __forceinline__ PlWindow pl_ref_window(const uint8_t *__restrict__ bytes, const uint64_t *__restrict__ rec_off, uint32_t n_rec,
                                                  const uint32_t *__restrict__ rec_nidx, uint32_t k, uint64_t i)
{
  uint32_t lo = 0, hi = n_rec;  // invariant: rec_off[lo] <= i < rec_off[hi]
  while (hi - lo > 1) {
    const uint32_t mid = (lo + hi) >> 1;
    if (rec_off[mid] <= i) lo = mid; else hi = mid;
  }
  PlWindow w;
  w.gene = rec_nidx[lo];
  w.x = (uint32_t)(i - rec_off[lo]);
  w.kmer = i + k <= rec_off[lo + 1] ? pl_window(bytes + i, nullptr, 0, k) : PL_NO_KMER;
  return w;
}

__global__ __launch_bounds__(256) void pl_keys_kernel(const uint8_t *__restrict__ bytes, uint64_t total, const uint64_t *__restrict__ rec_off, uint32_t n_rec,
                                                      const uint32_t *__restrict__ rec_nidx, uint32_t k, uint64_t *__restrict__ keys)
{
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= total) return;
  const PlWindow w = pl_ref_window(bytes, rec_off, n_rec, rec_nidx, k, i);
  keys[i] = w.kmer == PL_NO_KMER ? PL_KEY_NONE : (((uint64_t)pl_hash32(w.gene, w.kmer & ~(1ull << 63)) << 32) | i);
}

__device__ __forceinline__ bool pl_same_pair(const PlWindow &a, const PlWindow &b)
{
  return a.gene == b.gene && ((a.kmer ^ b.kmer) & ~(1ull << 63)) == 0ull;
}

__global__ __launch_bounds__(256) void pl_heads_kernel(const uint64_t *__restrict__ keys, uint64_t total, const uint8_t *__restrict__ bytes,
                                                       const uint64_t *__restrict__ rec_off, uint32_t n_rec, const uint32_t *__restrict__ rec_nidx, uint32_t k,
                                                       uint32_t *__restrict__ flags)
{
  const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= total) return;
  const uint64_t key = keys[t];
  uint32_t head = 0;
  if (key != PL_KEY_NONE) {
    const PlWindow me = pl_ref_window(bytes, rec_off, n_rec, rec_nidx, k, key & 0xFFFFFFFFull);
    head = 1;
    for (uint64_t u = t; u > 0 && (keys[u - 1] >> 32) == (key >> 32); --u) {
      const PlWindow o = pl_ref_window(bytes, rec_off, n_rec, rec_nidx, k, keys[u - 1] & 0xFFFFFFFFull);
      if (pl_same_pair(me, o)) { head = 0; break; }
    }
  }
  flags[t] = head;
}

__global__ __launch_bounds__(256) void pl_write_kernel(const uint64_t *__restrict__ keys, uint64_t total, const uint32_t *__restrict__ idx,
                                                       const uint8_t *__restrict__ bytes, const uint64_t *__restrict__ rec_off, uint32_t n_rec,
                                                       const uint32_t *__restrict__ rec_nidx, uint32_t k, uint4 *__restrict__ ptab, uint64_t ptab_n)
{
  const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= total) return;
  const uint64_t key = keys[t];
  if (key == PL_KEY_NONE) return;
  const uint32_t o = idx[t];
  const bool head = t + 1 < total ? idx[t + 1] != o : (uint64_t)o + 1 == ptab_n;   // (exclusive scan of the head flags)
  if (!head || o >= ptab_n) return;
  const PlWindow me = pl_ref_window(bytes, rec_off, n_rec, rec_nidx, k, key & 0xFFFFFFFFull);
  bool ambiguous = false;
  for (uint64_t u = t + 1; u < total && (keys[u] >> 32) == (key >> 32); ++u) {
    const PlWindow w = pl_ref_window(bytes, rec_off, n_rec, rec_nidx, k, keys[u] & 0xFFFFFFFFull);
    if (pl_same_pair(me, w)) { ambiguous = true; break; }
  }
  const uint64_t canon = me.kmer & ~(1ull << 63);
  uint4 e;
  e.x = (uint32_t)canon;
  e.y = (uint32_t)(canon >> 32);
  e.z = ambiguous ? PTAB_AMBIGUOUS : (me.x | ((uint32_t)(me.kmer >> 63) << 31));
  e.w = me.gene;
  ptab[o] = e;
}

__device__ __forceinline__ uint32_t pl_entry_bucket(const uint4 e, uint32_t lg) { return pl_hash32(e.w, ((uint64_t)e.y << 32) | e.x) >> (32u - lg); }

// pdir[b] = first entry whose bucket is >= b; every word of pdir[0 .. 2^lg] is written by exactly one thread
__global__ __launch_bounds__(256) void pl_dir_kernel(const uint4 *__restrict__ ptab, uint64_t n, uint32_t lg, uint32_t *__restrict__ pdir)
{
  const uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= n) return;
  const uint64_t b = pl_entry_bucket(ptab[j], lg);
  const uint64_t first = j ? (uint64_t)pl_entry_bucket(ptab[j - 1], lg) + 1 : 0;
  for (uint64_t q = first; q <= b; ++q) pdir[q] = (uint32_t)j;
  if (j + 1 == n)
    for (uint64_t q = b + 1; q <= (1ull << lg); ++q) pdir[q] = (uint32_t)n;
}

unsigned grid_for(uint64_t n, unsigned threads) { return (unsigned)((n + threads - 1) / threads); }

}  // namespace

int build_placement_table(Ctx *ctx, const uint8_t *d_bytes, uint64_t total, const uint64_t *d_rec_off, uint32_t n_rec, const uint32_t *d_rec_nidx,
                          uint64_t *keys_a, uint64_t *keys_b)
{
  DeviceIndex &ix = ctx->idx;
  hipStream_t st = ctx->stream;
  const uint32_t k = ctx->prm.k;
  for (uint32_t r = 0; r < n_rec; ++r)
    if (ctx->ref_off[r + 1] - ctx->ref_off[r] >= (1ull << 31)) {
      ctx->last_error = "shk_ref_keep_positions: a record has >= 2^31 bases";
      return SHK_ERR_INDEX_TOO_LARGE;
    }
  uint32_t *d_flags = nullptr, *d_hist = nullptr;
  uint64_t *d_scan = nullptr, *d_sort_scan = nullptr;
  int rc = SHK_OK;
  auto cleanup = [&]() { (void)hipFree(d_flags); (void)hipFree(d_hist); (void)hipFree(d_scan); (void)hipFree(d_sort_scan); };
#define PB_HIP(call)                                                                       \
  do {                                                                                     \
    hipError_t e__ = (call);                                                               \
    if (e__ != hipSuccess) { rc = set_hip_error(ctx, e__, #call); cleanup(); return rc; } \
  } while (0)

  uint64_t n_u = 0;
  const uint64_t *sorted = nullptr;
  // (an index of more than 65 536 records carries no table: shk_placement_enable refuses it)
  const bool have = total > 0 && keys_a && keys_b && d_rec_nidx && !ix.wrap;
  if (have) {
    hipLaunchKernelGGL(pl_keys_kernel, dim3(grid_for(total, 256)), dim3(256), 0, st, d_bytes, total, d_rec_off, n_rec, d_rec_nidx, k, keys_a);
    PB_HIP(hipGetLastError());
    PB_HIP(hipMalloc((void **)&d_hist, radix_sort_hist_words(total) * sizeof(uint32_t)));
    PB_HIP(hipMalloc((void **)&d_sort_scan, scan_temp_words(radix_sort_hist_words(total)) * sizeof(uint64_t)));
    sorted = radix_sort_u64(keys_a, keys_b, total, 64, d_hist, d_sort_scan, st);
    if (!sorted) { cleanup(); ctx->last_error = "radix sort launch failed"; return SHK_ERR_HIP; }
    PB_HIP(hipMalloc((void **)&d_flags, (total + 1) * sizeof(uint32_t)));
    PB_HIP(hipMalloc((void **)&d_scan, scan_temp_words(total) * sizeof(uint64_t)));
    hipLaunchKernelGGL(pl_heads_kernel, dim3(grid_for(total, 256)), dim3(256), 0, st, sorted, total, d_bytes, d_rec_off, n_rec, d_rec_nidx, k, d_flags);
    PB_HIP(hipGetLastError());
    const uint64_t *d_tot = exclusive_scan_u32(d_flags, d_flags, total, d_scan, st);
    PB_HIP(hipGetLastError());
    PB_HIP(hipMemcpyAsync(&n_u, d_tot, sizeof(uint64_t), hipMemcpyDeviceToHost, st));
    PB_HIP(hipStreamSynchronize(st));
  }
  if (n_u > (1ull << 30)) { cleanup(); ctx->last_error = "shk_ref_keep_positions: more than 2^30 distinct (gene, k-mer) pairs"; return SHK_ERR_INDEX_TOO_LARGE; }
  // two buckets per entry or more: most buckets hold no entry or one, so a lookup is the directory's two words and one 16-byte entry
  uint32_t lg = 6;
  while ((1ull << lg) < 2 * n_u) ++lg;
  PB_HIP(hipMalloc((void **)&ix.ptab, (n_u + 1) * sizeof(uint4)));
  PB_HIP(hipMalloc((void **)&ix.pdir, ((1ull << lg) + 2) * sizeof(uint32_t)));
  PB_HIP(hipMemsetAsync(ix.pdir, 0, ((1ull << lg) + 2) * sizeof(uint32_t), st));
  if (n_u) {
    hipLaunchKernelGGL(pl_write_kernel, dim3(grid_for(total, 256)), dim3(256), 0, st, sorted, total, (const uint32_t *)d_flags, d_bytes, d_rec_off, n_rec,
                       d_rec_nidx, k, ix.ptab, n_u);
    PB_HIP(hipGetLastError());
    hipLaunchKernelGGL(pl_dir_kernel, dim3(grid_for(n_u, 256)), dim3(256), 0, st, (const uint4 *)ix.ptab, n_u, lg, ix.pdir);
    PB_HIP(hipGetLastError());
  }
  PB_HIP(hipStreamSynchronize(st));
  ix.ptab_lg = lg;
  ix.ptab_n = n_u;
  cleanup();
#undef PB_HIP
  return SHK_OK;
}

}  // namespace shk
