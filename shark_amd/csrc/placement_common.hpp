// placement_common.hpp -- what the builder of the placement table (placement_build.hip) and its readers (placement.hip, segments.hip) share.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kmer_device.hpp"

namespace shk {

// where a (gene, canonical k-mer) pair lives in DeviceIndex::ptab: the entries are sorted by this hash, its top ptab_lg bits
// name the bucket of pdir.  (XXH64's avalanche over the k-mer with the gene folded in: for one gene a bijection of the k-mer.)
__host__ __device__ __forceinline__ uint32_t pl_hash32(uint32_t gene, uint64_t canon)
{
  return (uint32_t)(xxh64_u64(canon ^ ((uint64_t)(gene + 1u) * XP1)) >> 32);
}

// DeviceIndex::ptab's z word of a (gene, k-mer) pair with two or more windows in the gene's record (shark_internal.hpp)
constexpr uint32_t PTAB_AMBIGUOUS = 0xFFFFFFFFu;   // (no window has x = 2^31 - 1: a record has fewer than 2^31 bases)

constexpr uint64_t PL_NO_KMER = ~0ull;

// the window of k bytes at s: canonical k-mer | orientation << 63 (1: the window's own k-mer is the canonical one), or PL_NO_KMER
// for a window with a character that is no base or one that is its own reverse complement.  q != nullptr: the quality mask
// (FastqSplitter.hpp:106: a masked character is the character minus 64)
__device__ __forceinline__ uint64_t pl_window(const uint8_t *__restrict__ s, const uint8_t *__restrict__ q, int32_t mq, uint32_t k)
{
  uint64_t fw = 0;
  uint32_t bad = 0;
  for (uint32_t j = 0; j < k; ++j) {
    uint32_t ch = s[j];
    if (q && (int32_t)(int8_t)q[j] < mq) ch = (ch - 64u) & 0xFFu;
    const uint32_t c = base_code(ch);
    bad |= c >> 2;
    fw = (fw << 2) | (c & 3u);
  }
  if (bad) return PL_NO_KMER;
  const uint64_t rc = revcomp_left_aligned(fw << (64 - 2 * k), k);
  if (fw == rc) return PL_NO_KMER;
  return fw < rc ? (fw | (1ull << 63)) : rc;
}

// ---- the readers' side (placement_kernel, segments_kernel): one wavefront per read, the first PL_CACHED_CHUNKS x 64 slots of a mate in LDS ----
constexpr int PL_THREADS = 256, PL_WAVES = PL_THREADS / 64;
constexpr uint32_t PL_CACHED_CHUNKS = 8;        // 512 slots per mate in LDS: 2 x 4 KiB per wave
constexpr uint64_t PL_NO_VOTE = ~0ull;

__device__ __forceinline__ uint64_t wave_min_u64(uint64_t v)
{
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) {
    const uint64_t t = __shfl_xor(v, o, 64);
    v = t < v ? t : v;
  }
  return v;
}

// the vote of slot p of a mate of length L whose window is w (pl_window) for gene g, or PL_NO_VOTE: (strand, pos) packed so that
// unsigned order is "strand 0 first, then the smaller pos" (pl_vote_strand, pl_vote_pos take it apart).  P: the kernel's parameter block
// with the table (ptab, pdir, ptab_lg) and k
template <typename Params>
__device__ __forceinline__ uint64_t pl_vote(const Params &P, uint32_t g, uint64_t w, uint32_t p, uint32_t L)
{
  if (w == PL_NO_KMER) return PL_NO_VOTE;
  const uint64_t canon = w & ~(1ull << 63);
  const uint32_t b = pl_hash32(g, canon) >> (32u - P.ptab_lg);
  const uint32_t first = P.pdir[b], last = P.pdir[b + 1];
  for (uint32_t j = first; j < last; ++j) {
    const uint4 e = P.ptab[j];
    if (e.x == (uint32_t)canon && e.y == (uint32_t)(canon >> 32) && e.w == g) {
      if (e.z == PTAB_AMBIGUOUS) return PL_NO_VOTE;
      const uint32_t x = e.z & 0x7FFFFFFFu;
      const uint32_t strand = (e.z >> 31) ^ (uint32_t)(w >> 63);
      const int32_t pos = strand ? (int32_t)(x + p + P.k - L) : (int32_t)(x - p);
      return ((uint64_t)strand << 32) | ((uint32_t)pos ^ 0x80000000u);
    }
  }
  return PL_NO_VOTE;
}
__device__ __forceinline__ uint32_t pl_vote_strand(uint64_t key) { return (uint32_t)(key >> 32); }
__device__ __forceinline__ int32_t pl_vote_pos(uint64_t key) { return (int32_t)((uint32_t)key ^ 0x80000000u); }

}  // namespace shk
