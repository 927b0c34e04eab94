// kmer_table.hpp -- the LDS-resident exact table of a one-gene index KEYED BY THE CANONICAL K-MER ITSELF: layout, host-side
// construction and the lookup rule (plain C++, next to lds_table.hpp: index_build.hip builds the image, classify_uni_kernel's KX
// instantiations read it in LDS through kxtab_lookup below, the host-only tool shark-kxtab-check lets the CPU tests verify
// construction and exactness without a GPU).
//
// The reference's answer for a k-mer depends only on its filter position, so the set K of canonical k-mers whose position is a
// set bit -- the gene's own k-mers and the k-mers that collide with them in the filter -- decides hit or miss exactly; a table of K
// answers a probe without XXH64.  A key c is a canonical k-mer of k <= 17 bases: c < 2^34.
//
//   a  = c & 0xFFFF, b = c >> 16                              (16 + 18 bits)
//   t  = b ^ (((a + 1) * m1) >> 6 & 0x3FFFF)                       the TAG (18 bits); group g = t & 0x1FFF
//   a' = a ^ ((t * m2) >> 16 & 0xFFFF)
//   slot = (a' + D[g]) mod 2^16;   slot >= KXTAB_SLOTS: a miss;   else the key is in the table iff T[slot] == t and t != 0
//
// (a, b) -> (a, t) -> (a', t) are two Feistel steps: a bijection on 34 bits for any m1, m2.  A stored tag names its group, hence the
// displacement the entry was placed with, hence a' = slot - D[g], hence (a, b): entry and slot determine the key, a match is exact
// over all 2^34 values.  T is stored as T16[KXTAB_SLOTS] (the tag's low 16 bits) and T2 (its high 2 bits, four slots a byte); the
// all-zero entry means empty, so no key may have the tag 0 and a probe whose tag is 0 is a miss.  Only 57 344 of the ring's 2^16 slot
// numbers exist: 114 688 + 14 336 + 16 384 (D: 8 192 x uint16) = 145 408 bytes <= LTAB_BYTES, the LDS the exact-table kernels reserve.
// The builder looks for (m1, m2) under which no key has the tag 0, no two keys of a group share a', and every group finds a
// displacement that puts all its keys on free existing slots (greedy, largest group first, as ltab_build does).  Two keys of a group
// share a' with probability 2^-16: 1.5 such pairs are expected among 40 000 keys, so about one attempt in five succeeds and
// KXTAB_TRIES pairs of multipliers are tried; an attempt that fails does so in its first pass over the keys.
#pragma once
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <vector>

#if defined(__HIPCC__)
#define SHK_KX_FN __host__ __device__ __forceinline__
#else
#define SHK_KX_FN inline
#endif

namespace shk {

constexpr uint32_t KXTAB_KEY_BITS = 34;                      // k <= 17
constexpr uint32_t KXTAB_RING_LG = 16, KXTAB_GROUP_LG = 13, KXTAB_TAG_BITS = KXTAB_KEY_BITS - KXTAB_RING_LG;
constexpr uint32_t KXTAB_SLOTS = 57344;                      // slot numbers that exist (a multiple of 64)
constexpr uint32_t KXTAB_T2_OFF = KXTAB_SLOTS * 2u;          // byte offsets into the image: T16 at 0
constexpr uint32_t KXTAB_D_OFF = KXTAB_T2_OFF + KXTAB_SLOTS / 4u;
constexpr uint32_t KXTAB_BYTES = KXTAB_D_OFF + (1u << KXTAB_GROUP_LG) * 2u;   // 145 408
constexpr uint32_t KXTAB_MAX_KEYS = 44000;                   // load <= 0.77 of the existing slots
constexpr uint32_t KXTAB_TRIES = 64;
constexpr uint32_t KXTAB_TAG_MASK = (1u << KXTAB_TAG_BITS) - 1u;
// the multipliers of attempt n: odd, 24 bits (a 24-bit multiply is a full-rate instruction on the device)
inline constexpr uint32_t kxtab_m1(uint32_t attempt) { return (0x9E3779u + 0x370E6u * attempt) & 0xFFFFFFu; }
inline constexpr uint32_t kxtab_m2(uint32_t attempt) { return (0x85EBCBu + 0x58366u * attempt) & 0xFFFFFFu; }

// the tag of a key and its slot before the displacement (low 16 bits count)
SHK_KX_FN void kxtab_mix(const uint64_t c, const uint32_t m1, const uint32_t m2, uint32_t &tag, uint32_t &base)
{
  const uint32_t lo = (uint32_t)c, a = lo & 0xFFFFu;
  const uint32_t m = m1 & 0xFFFFFFu;
  tag = (uint32_t)(c >> KXTAB_RING_LG) ^ (((a * m + m) >> 6) & KXTAB_TAG_MASK);   // ((a + 1) m1: the key 0, poly-A, has a tag other than 0)
  base = lo ^ ((tag * (m2 & 0xFFFFFFu)) >> 16);
}

// The lookup rule: is c (< 2^34) a key of the image?  The builder's check, the host tool and the tests go through this, and so do the
// kernels where a hit is the expected answer (the tiles' round).
// (Every read stays inside the image whatever c is: a slot number that does not exist reads T2's and D's bytes and is a miss.)
SHK_KX_FN bool kxtab_lookup(const uint8_t *img, const uint32_t m1, const uint32_t m2, const uint64_t c)
{
  uint32_t tag, base;
  kxtab_mix(c, m1, m2, tag, base);
  const uint32_t d = *reinterpret_cast<const uint16_t *>(img + KXTAB_D_OFF + ((tag << 1) & ((2u << KXTAB_GROUP_LG) - 2u)));
  const uint32_t s2 = ((base + d) << 1) & ((2u << KXTAB_RING_LG) - 2u);          // twice the slot number
  const uint32_t t16 = *reinterpret_cast<const uint16_t *>(img + s2);
  const uint32_t t2 = img[KXTAB_T2_OFF + (s2 >> 3)];
  const uint32_t e = t16 | (((t2 >> (s2 & 6u)) & 3u) << 16);
  return (s2 < 2u * KXTAB_SLOTS) & (e == tag) & (tag != 0u);
}

// The same rule in two stages, for the kernels' probes of reads from elsewhere, where a miss is the expected answer: every lane runs
// the first, the second runs behind a ballot that a wave of misses does not pass (classify_uni_tiles.inc).
// THE CANDIDATE STAGE: mixing, D, the slot, T16, and the compare of the tag's low 16 bits -- a key of the image always passes it (all
// 18 bits of its entry agree), and a value that is no key passes it about 2 in 100 000 times: an occupied slot of its group whose
// entry differs in the bits 16 and 17 only, an empty slot under a tag whose low half is 0, a slot number that does not exist whose
// two bytes (T2's or D's) happen to agree.  `tag` and `s2` (twice the slot number) are what the confirm stage needs.
SHK_KX_FN bool kxtab_candidate(const uint8_t *img, const uint32_t m1, const uint32_t m2, const uint64_t c, uint32_t &tag, uint32_t &s2)
{
  uint32_t base;
  kxtab_mix(c, m1, m2, tag, base);
  const uint32_t d = *reinterpret_cast<const uint16_t *>(img + KXTAB_D_OFF + ((tag << 1) & ((2u << KXTAB_GROUP_LG) - 2u)));
  s2 = ((base + d) << 1) & ((2u << KXTAB_RING_LG) - 2u);
  const uint16_t t16 = *reinterpret_cast<const uint16_t *>(img + s2);
  return t16 == (uint16_t)tag;
}

// THE CONFIRM STAGE, for a candidate: the entry's two high bits (T2), the slot number exists, the tag is not the empty entry's.
// candidate && confirm == kxtab_lookup for every c.
SHK_KX_FN bool kxtab_confirm(const uint8_t *img, const uint32_t tag, const uint32_t s2)
{
  const uint32_t t2 = img[KXTAB_T2_OFF + (s2 >> 3)];
  return (s2 < 2u * KXTAB_SLOTS) & (((t2 >> (s2 & 6u)) & 3u) == (tag >> 16)) & (tag != 0u);
}

// The image (KXTAB_BYTES) for a sorted set of distinct keys and a pair of multipliers.  The displacement search tests 64
// displacements a step against the ring's occupancy kept as 64-bit words (40 000 keys: a fraction of a millisecond; slot by slot it
// took half a second).  false = a key has the tag 0, two keys of a group share a base, or some group fits nowhere.
inline bool kxtab_build_with(const std::vector<uint64_t> &keys, const uint32_t m1, const uint32_t m2, std::vector<uint8_t> &img)
{
  constexpr uint32_t NG = 1u << KXTAB_GROUP_LG, NR = 1u << KXTAB_RING_LG, NW = NR / 64u;
  struct K { uint32_t base, tag; };
  std::vector<uint32_t> start(NG + 1, 0u);
  std::vector<K> mixed(keys.size()), ks(keys.size());
  for (size_t i = 0; i < keys.size(); ++i) {
    uint32_t tag, base;
    kxtab_mix(keys[i], m1, m2, tag, base);
    if (tag == 0u) return false;
    mixed[i] = K{base & (NR - 1u), tag};
    ++start[(tag & (NG - 1u)) + 1u];
  }
  for (uint32_t g = 0; g < NG; ++g) start[g + 1] += start[g];
  {
    std::vector<uint32_t> fill(start.begin(), start.end() - 1);
    for (const K &x : mixed) ks[fill[x.tag & (NG - 1u)]++] = x;      // (stable: a group's keys stay in the order of the sorted key list)
  }
  // two keys of a group on one base cannot be told apart by any displacement: other multipliers have to be tried
  // (a handful of keys per group: compared pair by pair; a crowded group -- low-complexity keys -- is sorted first)
  for (uint32_t g = 0; g < NG; ++g) {
    const uint32_t lo = start[g], hi = start[g + 1];
    if (hi - lo > 32u) {
      std::vector<uint32_t> bs;
      for (uint32_t i = lo; i < hi; ++i) bs.push_back(ks[i].base);
      std::sort(bs.begin(), bs.end());
      if (std::adjacent_find(bs.begin(), bs.end()) != bs.end()) return false;
    } else {
      for (uint32_t i = lo; i < hi; ++i)
        for (uint32_t j = i + 1; j < hi; ++j)
          if (ks[i].base == ks[j].base) return false;
    }
  }
  std::vector<uint32_t> order(NG);
  for (uint32_t g = 0; g < NG; ++g) order[g] = g;
  std::stable_sort(order.begin(), order.end(), [&](uint32_t x, uint32_t y) { return start[x + 1] - start[x] > start[y + 1] - start[y]; });
  img.assign(KXTAB_BYTES, 0u);
  uint64_t occ[NW];
  for (uint32_t w = 0; w < NW; ++w) occ[w] = w < KXTAB_SLOTS / 64u ? 0ull : ~0ull;   // (the slot numbers that do not exist are taken)
  // the occupancy of the 64 ring slots from p on
  auto window = [&](const uint32_t p) -> uint64_t {
    const uint32_t w = p >> 6, s = p & 63u;
    return s ? (occ[w] >> s) | (occ[(w + 1u) & (NW - 1u)] << (64u - s)) : occ[w];
  };
  for (const uint32_t g : order) {
    const uint32_t lo = start[g], hi = start[g + 1];
    if (lo == hi) break;
    uint32_t d = NR;
    // (the search starts at a displacement of the group's own: from 0 for every group it is linear probing -- the keys whose base
    //  is a slot number that does not exist all pile up behind the ring's start, and a single key then walks thousands of slots)
    const uint32_t first = (g * 0x9E37u) & (NR - 64u);
    // (... and a key that stands among the slot numbers that do not exist stays there for up to 8 192 displacements: skipped in one step)
    for (uint32_t n = 0, step = 64u; n < NR && d == NR; n += step) {
      const uint32_t d0 = (first + n) & (NR - 1u);
      uint64_t busy = 0ull;
      step = 64u;
      for (uint32_t i = lo; i < hi; ++i) {
        const uint32_t p = (ks[i].base + d0) & (NR - 1u);
        if (p >= KXTAB_SLOTS && ((NR - p) & ~63u) > step) step = (NR - p) & ~63u;
        busy |= window(p);
      }
      if (~busy) d = d0 + (uint32_t)__builtin_ctzll(~busy);
    }
    if (d == NR) return false;
    for (uint32_t i = lo; i < hi; ++i) {
      const uint32_t slot = (ks[i].base + d) & (NR - 1u);
      occ[slot >> 6] |= 1ull << (slot & 63u);
      const uint16_t t16 = (uint16_t)ks[i].tag;
      memcpy(img.data() + 2u * slot, &t16, 2);
      img[KXTAB_T2_OFF + (slot >> 2)] |= (uint8_t)((ks[i].tag >> 16) << (2u * (slot & 3u)));
    }
    const uint16_t d16 = (uint16_t)d;
    memcpy(img.data() + KXTAB_D_OFF + 2u * g, &d16, 2);
  }
  return true;
}

// ... trying the pairs of multipliers in turn.  `keys` in any order, duplicates dropped: the image depends on the SET alone.
// false: too many keys (KXTAB_MAX_KEYS), a key beyond 34 bits, or no attempt worked -- the caller keeps the hashed table.
inline bool kxtab_build(std::vector<uint64_t> keys, std::vector<uint8_t> &img, uint32_t *m1, uint32_t *m2, uint32_t *attempts = nullptr)
{
  std::sort(keys.begin(), keys.end());
  keys.erase(std::unique(keys.begin(), keys.end()), keys.end());
  if (attempts) *attempts = 0;
  if (keys.size() > KXTAB_MAX_KEYS || (!keys.empty() && (keys.back() >> KXTAB_KEY_BITS) != 0ull)) return false;
  for (uint32_t a = 0; a < KXTAB_TRIES; ++a) {
    if (attempts) *attempts = a + 1u;
    if (kxtab_build_with(keys, kxtab_m1(a), kxtab_m2(a), img)) { *m1 = kxtab_m1(a); *m2 = kxtab_m2(a); return true; }
  }
  return false;
}

}  // namespace shk
