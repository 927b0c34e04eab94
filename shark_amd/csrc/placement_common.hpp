// placement_common.hpp -- what the builder of the placement table (placement_build.hip) and its reader (placement.hip) share.
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

}  // namespace shk
