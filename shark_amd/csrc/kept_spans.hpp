// kept_spans.hpp -- the kept spans of a mate (include/shark_hip.h, "spliced depth and the junction table"): what the consumers of
// segments mode on the device (spliced.hip) share.  Steps 1 and 2 of the header's junction rule, defined once.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/shark_hip.h"

namespace shk {

static_assert(SHK_MAX_SEGMENTS == 4 && sizeof(shk_segment) == 20, "kept_spans sorts four records of five words");

// at most four record spans [lo, hi) with the pos of their diagonal, sorted by (lo, hi); entries n .. 3 are not spans
struct KeptSpans {
  int32_t lo[SHK_MAX_SEGMENTS], hi[SHK_MAX_SEGMENTS], pos[SHK_MAX_SEGMENTS];
  uint32_t n;
};

// one comparator of the network: order (a, b) by key, then by rank -- the keys with their ranks are all distinct, so the network's
// result is the stable sort's whatever its comparators are
#define SHK_KS_CSWAP(a, b)                                                              \
  do {                                                                                  \
    if (key[a] > key[b] || (key[a] == key[b] && rnk[a] > rnk[b])) {                     \
      const uint64_t tk = key[a]; key[a] = key[b]; key[b] = tk;                         \
      const uint32_t tr = rnk[a]; rnk[a] = rnk[b]; rnk[b] = tr;                         \
      const int32_t tp = S.pos[a]; S.pos[a] = S.pos[b]; S.pos[b] = tp;                  \
    }                                                                                   \
  } while (0)

// The kept spans of one mate of L bytes at floor s_min (>= 1) from its SHK_MAX_SEGMENTS ranked records e[0 .. 3] (rank order, empty
// slots last, as segments_kernel stores them; 16-byte aligned: a mate's four records are 80 bytes): the records with
// support >= s_min on rank 0's strand, sorted by (lo, hi), equal spans in rank order.  Ranks descend in support, so rank 0 below
// s_min leaves nothing.  Constant indices only: everything stays in registers.
__device__ __forceinline__ KeptSpans kept_spans(const shk_segment *__restrict__ e, uint32_t L, uint32_t k, uint32_t s_min)
{
  const uint32_t *w = static_cast<const uint32_t *>(__builtin_assume_aligned(e, 16));
  KeptSpans S;
  uint64_t key[SHK_MAX_SEGMENTS];   // (lo, hi) with the sign bits flipped: unsigned order is (lo, hi) order; all ones: not kept
  uint32_t rnk[SHK_MAX_SEGMENTS];
  const uint32_t strand0 = w[2];
  S.n = 0;
#pragma unroll
  for (int r = 0; r < SHK_MAX_SEGMENTS; ++r) {
    const int32_t pos = (int32_t)w[r * 5 + 0];
    const uint32_t support = w[r * 5 + 1], strand = w[r * 5 + 2], first = w[r * 5 + 3], last = w[r * 5 + 4];
    const bool keep = support >= s_min && strand == strand0;
    const int32_t lo = strand ? pos + (int32_t)(L - k - last) : pos + (int32_t)first;
    const int32_t hi = strand ? pos + (int32_t)(L - first) : pos + (int32_t)(last + k);
    key[r] = keep ? ((uint64_t)((uint32_t)lo ^ 0x80000000u) << 32) | ((uint32_t)hi ^ 0x80000000u) : ~0ull;
    rnk[r] = (uint32_t)r;
    S.pos[r] = pos;
    S.n += keep ? 1u : 0u;
  }
  // five comparators sort four
  SHK_KS_CSWAP(0, 1);
  SHK_KS_CSWAP(2, 3);
  SHK_KS_CSWAP(0, 2);
  SHK_KS_CSWAP(1, 3);
  SHK_KS_CSWAP(1, 2);
#pragma unroll
  for (int r = 0; r < SHK_MAX_SEGMENTS; ++r) {
    S.lo[r] = (int32_t)((uint32_t)(key[r] >> 32) ^ 0x80000000u);
    S.hi[r] = (int32_t)((uint32_t)key[r] ^ 0x80000000u);
  }
  return S;
}

#undef SHK_KS_CSWAP

}  // namespace shk
