// align.hip -- alignments mode's kernel (gfx950): per association and mate the gapped alignment of the mate to its gene's record as at most
// four blocks, with its match and mismatch counts against the record (include/shark_hip.h, "alignments").  The fourth
// consumer of segments mode on the device and the first reader of DeviceIndex::recbase inside a batch: it runs behind segments_kernel's
// records at m = SHK_MAX_SEGMENTS and behind pileup_kernel in the batch's tail.
//
// pileup_kernel's outer shape: one wavefront per read with associations, persistent beyond 2 048 workgroups, its three early returns
// and its guard for a read whose associations the buffers do not hold.  A mate's kept spans (kept_spans.hpp), the ownership walk with
// `reach` and the trimming with the read cursor are wave-uniform: scalar work.  The blocks of a mate are never held as an array: the walk
// keeps ONE open block A; when the next block B appears the gap between them is closed (both ends it can move are A's right and B's
// left), A is final, is counted and goes into the lanes that will store it, and B becomes the open block.  The walk itself always reads
// span 0 and moves the others down.  So no index into registers is ever a run-time value: no scratch memory.
//
// Closure of a gap of R <= 64 read bases: lane t < R loads its read byte and the record bases under it on A's and on B's diagonal, two
// ballots give the not-a-match masks, lane s < R prices split s with two popcounts, split R (all on A) is priced by the wave, and one
// wave minimum over cost << 7 | (64 - s) settles the split and the tie.  Counting: 64 block coordinates per pass, ballot and popcount
// into scalar counters.  A mate's record is one aligned 64-byte line: lanes 0 .. 15 store one dword each.  No LDS.
//
// Two compile-time switches of the one kernel (template parameters): end extension (the header's step 3a) scores a mate's
// two overhangs against the record 64 bases per pass -- two ballots, two popcounts per lane, one wave maximum -- when the first block
// becomes the open block and before the last one is counted; accumulation (aligned pileup) adds every base of a final block to the
// pileup state with one atomic where the counting loop has it loaded.  With both off the kernel is the code it always was.
//
// A third switch: spliced ends (the header's step 3b) try a mate's clipped end of a few bases across the listed junctions
// it could have crossed -- one lane per evaluated read base, one record byte, one ballot and one popcount per candidate site, the sites of
// the range found by a binary search -- behind gap closure and in front of end extension: where block 0 is about to be finished, and in the last pass.
// A placement adds a block through the walk itself: the one place that finishes a block stays the only one.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "kept_spans.hpp"
#include "placement_common.hpp"
#include "shark_internal.hpp"

namespace shk {

static_assert(sizeof(shk_mate_alignment) == 64, "a mate's record is one 64-byte line");

namespace {

constexpr uint32_t AL_WORDS = sizeof(shk_mate_alignment) / 4;   // 16: one per storing lane
constexpr uint32_t AL_MAX_CLOSE = 64;                           // the widest gap closure prices: one read base per lane

struct AlignParams {
  const uint32_t *gene_off;
  const uint16_t *gene_ids;
  const uint32_t *counters;
  uint64_t n;                      // reads
  const uint8_t *seq[2];           // nullptr: the batch has no such mate
  const uint64_t *off[2];
  const uint8_t *qual[2];          // nullptr: no masking
  int32_t mq;
  uint32_t k;
  const shk_segment *entries;      // [(j * 2 + mate) * SHK_MAX_SEGMENTS + r]
  const uint64_t *gene_start;
  const uint8_t *recbase;          // [gene_start[g] + x]: 0 .. 3, every other byte 4
  uint32_t n_genes;                // entries of gene_start - 1
  uint32_t skip_if_long;
  uint32_t s_min;
  uint32_t n_waves;                // of the launch: a wave's step through the reads (a kernel argument costs no register between its uses)
  uint32_t cap;                    // associations `entries` and `out` hold (at most 2^32 - 1: a batch has no more)
  uint32_t *out;                   // [(j * 2 + mate) * AL_WORDS + w]
};

// what the extending and the accumulating instantiations take on top (align_kernel itself keeps its arguments as they were)
struct AlignParamsX : AlignParams {
  uint32_t ext_p, ext_b;           // end extension: mismatch penalty 1 .. 15 and end bonus 0 .. 15 (read by the extending instantiations only)
  uint32_t n_store[2];             // the lanes that store mate m's record: 16, 32 for mate 1 of a single-end batch (as align_kernel works out), 0: no records
  uint32_t *counts;                // aligned pileup: [(gene_start[g] + x) * 4 + b]; `out` may then be nullptr and n_store 0: no records are stored
  unsigned long long *mates;
};

// what the splicing instantiations take on top of those (step 3b; shk_splice_sites_set's three arrays and shk_alignments_splice's values)
// One pointer and one word: where the compiler keeps a kernel argument in registers across the loops, these cost three, not ten.
struct AlignParamsS : AlignParamsX {
  const uint32_t *spl;             // SpliceSites::d: the offsets, the sites by donor, the sites by acceptor (splice_layout)
  uint32_t spl_prm;                // min_overhang 1 .. SHK_SPLICE_MAX_OVERHANG | max_cost << 8 | min_gap << 16
};

// The gene's sites in SpliceSites::d's layout: [g], [g + 1] of the n_genes + 1 offsets, behind them (at an even word) n = off[n_genes] pairs
// {donor, acceptor} ascending per gene in (donor, acceptor) -- the right end's -- and n pairs {acceptor, donor} ascending per gene in
// (acceptor, donor) -- the left end's.
__device__ __forceinline__ const uint2 *splice_sites(const uint32_t *__restrict__ spl, uint32_t n_genes, uint32_t g, bool by_acceptor, uint32_t &n_sites)
{
  const uint32_t s0 = spl[g], s1 = spl[g + 1u];
  n_sites = s1 - s0;
  const uint2 *const sites = reinterpret_cast<const uint2 *>(spl + splice_sites_word(n_genes));
  return sites + s0 + (by_acceptor ? spl[n_genes] : 0u);
}

// one mate's bytes behind the -q mask, read in the record's orientation
struct Mate {
  const uint8_t *seq, *qual;
  int32_t mq;
  uint32_t L, strand;
};

// The read base of read coordinate q (the header's "read coordinate") on the record's strand: 0 .. 3, or 4 for a byte that is no base, a
// masked one, and a q outside the mate (no block or gap holds one: the compare keeps a lane inside the mate whatever the records hold).
__device__ __forceinline__ uint32_t read_base(const Mate &M, int32_t q)
{
  const uint32_t idx = M.strand ? M.L - 1u - (uint32_t)q : (uint32_t)q;
  if (idx >= M.L) return 4u;
  uint32_t ch = M.seq[idx];
  if (M.qual && (int32_t)(int8_t)M.qual[idx] < M.mq) ch = (ch - 64u) & 0xFFu;
  const uint32_t c = base_code(ch);
  return c < 4u ? (M.strand ? 3u - c : c) : 4u;
}

// the record's code at x of a record of len_g bases that starts at rec (4 outside it: nothing reads there, as above)
__device__ __forceinline__ uint32_t record_base(const uint8_t *__restrict__ rec, int32_t len_g, int32_t x)
{
  return (uint32_t)x < (uint32_t)len_g ? (uint32_t)rec[x] : 4u;
}

__device__ __forceinline__ uint32_t wave_min_u32(uint32_t v)
{
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) {
    const uint32_t t = (uint32_t)__shfl_xor((int)v, o, 64);
    v = t < v ? t : v;
  }
  return v;
}

// The split of a gap of R read bases (1 <= R <= 64) that start at read coordinate q0, between a block that ends at record coordinate xa
// and one that starts at xb: the number s of them that go on the left block's diagonal.  Smallest cost, ties to the largest s.
__device__ __forceinline__ uint32_t close_gap(const Mate &M, const uint8_t *__restrict__ rec, int32_t len_g, int32_t q0, int32_t xa, int32_t xb, uint32_t R,
                                              uint32_t lane)
{
  bool not_a = false, not_b = false;
  if (lane < R) {
    const uint32_t b = read_base(M, q0 + (int32_t)lane);
    not_a = !(b < 4u && b == record_base(rec, len_g, xa + (int32_t)lane));
    not_b = !(b < 4u && b == record_base(rec, len_g, xb - (int32_t)R + (int32_t)lane));
  }
  const uint64_t mask_a = __ballot(not_a), mask_b = __ballot(not_b);   // (bits R .. 63 are 0)
  // split s = lane < R: the low s bits of A's mask and the bits from s on of B's (a shift by lane <= 63); split R: all of A's mask
  uint32_t key = 0xFFFFFFFFu;
  if (lane < R) key = ((uint32_t)(__popcll(mask_a & ((1ull << lane) - 1ull)) + __popcll(mask_b >> lane)) << 7) | (AL_MAX_CLOSE - lane);
  const uint32_t key_r = ((uint32_t)__popcll(mask_a) << 7) | (AL_MAX_CLOSE - R);
  const uint32_t best = std::min(wave_min_u32(key), key_r);
  return __builtin_amdgcn_readfirstlane(AL_MAX_CLOSE - (best & 127u));
}

__device__ __forceinline__ uint32_t wave_max_u32(uint32_t v)
{
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) {
    const uint32_t t = (uint32_t)__shfl_xor((int)v, o, 64);
    v = t > v ? t : v;
  }
  return v;
}

constexpr int32_t AL_EXT_BIAS = 15 * 64;   // a pass prices 64 bases at -15 at worst: relative scores lie in [-960, 64], [-960, 79] in the lane that adds the bonus

// End extension (the header's step between 3 and 4) of one end: base t = 0 .. H - 1 of the overhang is read base q + dir * t on record base
// x + dir * t (dir = +1 from the last block's end, -1 from the base in front of block 0); to_end: the overhang's H bases reach the mate's
// end, so e == H earns the bonus.  Returns the e in 0 .. H of largest score, ties to the smallest.  64 bases per pass: two ballots, lane
// t prices e = t0 + t + 1 relative to the pass with two popcounts, one wave maximum over (score + 960) << 7 | (64 - t) settles the pass
// and its tie; the score up to the pass and the best (score, e) so far are 64-bit scalars (|score| <= 15 * 2^31).
__device__ __forceinline__ uint32_t extend_end(const Mate &M, const uint8_t *__restrict__ rec, int32_t len_g, int32_t q, int32_t x, int32_t dir, int32_t H,
                                               bool to_end, uint32_t pen, uint32_t bonus, uint32_t lane)
{
  int64_t base = 0, best = 0;
  uint32_t best_e = 0;
  for (int32_t t0 = 0; t0 < H; t0 += 64) {
    const int32_t t = t0 + (int32_t)lane;
    bool is_m = false, is_x = false;
    if (t < H) {
      const uint32_t b = read_base(M, q + dir * t), rb = record_base(rec, len_g, x + dir * t);
      is_m = b < 4u && b == rb;
      is_x = b < 4u && rb < 4u && b != rb;
    }
    const uint64_t mm = __ballot(is_m), mx = __ballot(is_x);
    const uint64_t low = ~0ull >> (63u - lane);   // bits 0 .. lane
    // (the popcounts as signed numbers: an unsigned difference would wrap and, added to the 64-bit score, stay wrapped)
    int32_t rel = (int32_t)__popcll(mm & low) - (int32_t)pen * (int32_t)__popcll(mx & low);
    if (to_end && t == H - 1) rel += (int32_t)bonus;
    const uint32_t key = t < H ? ((uint32_t)(rel + AL_EXT_BIAS) << 7) | (64u - lane) : 0u;
    const uint32_t top = __builtin_amdgcn_readfirstlane(wave_max_u32(key));   // (lane 0 is inside the overhang: top != 0)
    const int64_t cand = base + ((int32_t)(top >> 7) - AL_EXT_BIAS);
    if (cand > best) {
      best = cand;
      best_e = (uint32_t)t0 + (64u - (top & 127u)) + 1u;
    }
    base += (int32_t)__popcll(mm) - (int32_t)pen * (int32_t)__popcll(mx);
    // nothing behind this pass can score more than every base left matching, and the bonus
    if (base + (int64_t)(H - t0 - 64) + (int64_t)bonus <= best) break;
  }
  return best_e;
}

// Spliced ends (the header's step 3b) of one end.  Lane t < n_eval holds evaluated read base t as b (4 in every other lane: the caller's
// load), which lies on record base x0 + t on the block's own diagonal.  `sites` are the gene's {key, other} pairs ascending in (key, other): {donor, acceptor} for the right end,
// {acceptor, donor} for the left (LEFT); the candidates are those with key in [key_lo, key_hi] whose far block stays inside the record
// (right: acceptor + far <= len_g with far = xe + h - donor = end - donor; left: donor - (acceptor - end) >= 0 with end = x0 - q0 of the
// block, the record coordinate of read base 0 on its diagonal).  A lane's record base under a candidate: right, x < donor ? x : x + shift;
// left, x >= acceptor ? x : x - shift.  One ballot and one popcount price a candidate; the lower bound of key_lo is one binary search, the
// range ends at the first key beyond key_hi.  best's cost and index and the smallest cost of another shift (the null candidate's included)
// are scalars.  Returns whether the end is placed, and then the site in (donor, acceptor).
template <bool LEFT>
__device__ __forceinline__ bool splice_end(const uint32_t b, const uint8_t *__restrict__ rec, int32_t len_g, const uint2 *__restrict__ sites, uint32_t n_sites,
                                           int32_t key_lo, int32_t key_hi, int32_t end, int32_t x0, uint32_t n_eval, uint32_t max_cost, uint32_t min_gap,
                                           uint32_t lane, int32_t &donor, int32_t &acceptor)
{
  uint32_t lo = 0, hi = n_sites;   // the first site with key >= key_lo
  while (lo < hi) {
    const uint32_t mid = lo + ((hi - lo) >> 1);
    if ((int32_t)__builtin_amdgcn_readfirstlane(sites[mid].x) < key_lo) lo = mid + 1u;
    else hi = mid;
  }
  // a lane outside the evaluated bases holds no base: it is "not a match" under every candidate, 64 - n_eval of them, taken off each cost
  const int32_t x = x0 + (int32_t)lane;
  const uint32_t idle = 64u - n_eval;
  // best's cost and its index (c1 == NONE: no candidate yet); c2: the smallest cost over the null candidate and the sites of another shift
  // than best's.  best's (donor, acceptor) are read again where they are compared: two scalar registers fewer across the loop
  constexpr uint32_t NONE = 0xFFFFFFFFu;
  uint32_t c1 = NONE, i1 = 0;
  uint32_t c2 = (uint32_t)__popcll(__ballot(!(b < 4u && b == record_base(rec, len_g, x)))) - idle;
  for (uint32_t i = lo; i < n_sites; ++i) {
    const int32_t key = (int32_t)__builtin_amdgcn_readfirstlane(sites[i].x), other = (int32_t)__builtin_amdgcn_readfirstlane(sites[i].y);
    if (key > key_hi) break;
    const int32_t d = LEFT ? other : key, a = LEFT ? key : other, shift = a - d;
    if (LEFT ? d - (a - end) < 0 : a + (end - d) > len_g) continue;
    const int32_t xc = LEFT ? (x >= a ? x : x - shift) : (x < d ? x : x + shift);
    const uint32_t c = (uint32_t)__popcll(__ballot(!(b < 4u && b == record_base(rec, len_g, xc)))) - idle;
    const int32_t key1 = (int32_t)__builtin_amdgcn_readfirstlane(sites[i1].x), other1 = (int32_t)__builtin_amdgcn_readfirstlane(sites[i1].y);
    const int32_t d1 = LEFT ? other1 : key1, a1 = LEFT ? key1 : other1;
    // ties: the largest donor, then the largest acceptor
    const bool wins = c < c1 || (c == c1 && (d > d1 || (d == d1 && a > a1)));
    if (c1 != NONE && shift == a1 - d1) {
      // the same placement up to where the bases between the two donors lie: the two do not compete
      if (wins) { c1 = c; i1 = i; }
    } else if (wins) {
      c2 = c1 < c2 ? c1 : c2;   // (everything seen so far but the null candidate costs at least what the best did)
      c1 = c; i1 = i;
    } else {
      c2 = c < c2 ? c : c2;
    }
  }
  if (c1 == NONE || c1 > max_cost || (int32_t)c2 - (int32_t)c1 < (int32_t)min_gap) return false;
  const int32_t key1 = (int32_t)__builtin_amdgcn_readfirstlane(sites[i1].x), other1 = (int32_t)__builtin_amdgcn_readfirstlane(sites[i1].y);
  donor = LEFT ? other1 : key1;
  acceptor = LEFT ? key1 : other1;
  return true;
}

// The kernel.  EXT: the ends are extended (step 3a; P.ext_p >= 1, P.ext_b).  ACC: every base of a final block is added to the pileup state
// where it is counted (P.counts, P.mates), and records are stored only where P.n_store says so.  The kernel takes its arguments by value
// as a template parameter: behind a function that takes them by reference the same statements cost one scalar register more.
// align_kernel<false, false, false, AlignParams> is the code and the arguments alignments mode always had; the other three take AlignParamsX,
// whose fields a discarded branch never names.  SPL: the ends are tried across the listed junctions (step 3b; AlignParamsS) -- a left
// placement, tried where block 0 is about to be finished (behind its gap's closure), makes the new block the open block and the shortened
// block 0 the pass's, whose own block goes back to the walk as a span; a right placement gives the last pass a block and runs that pass
// again.  So a block is still finished in exactly one place and the loops carry no new value.
template <bool EXT, bool ACC, bool SPL, class Params>
__global__ __launch_bounds__(PL_THREADS) void align_kernel(const Params P)
{
  // the batch will be assembled again and comes through here again; or it will be refused in wait (pileup_kernel's rule)
  if (P.counters[CTR_OVERFLOW] || (P.skip_if_long && P.counters[CTR_LONG]) || P.counters[CTR_VOUCH_BAD]) return;
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);   // (the same in every lane: what follows from it is scalar)
  // all ones in the lane that stores header word w, as vector values: the same as sixteen compares of the lane id against constants would
  // be kept as 64-bit lane masks in scalar registers across every loop, which the scalar file has no room for.
  // The record's layout over the lanes, lane w holding dword w (`word` below): lanes 0 .. 3 n_blocks, strand, matches, mismatches;
  // lanes 4 + 3 b + {0, 1, 2} block b's x, q, len (b = 0 .. 3); so hdr[w] is 0xFFFFFFFF in lane w and 0 elsewhere, hdr_any is all
  // ones in lanes 0 .. 3, and a finished block reaches its three lanes through `lane - (4 + 3 n_blocks)` being 0, 1 or 2.
  uint32_t hdr[4];
#pragma unroll
  for (uint32_t w = 0; w < 4; ++w) hdr[w] = 0u - (((lane ^ w) - 1u) >> 31);   // (lane == w: 0 - 1 has the top bit)
  const uint32_t hdr_any = hdr[0] | hdr[1] | hdr[2] | hdr[3];
  // (ACC) pileup mates, mates with a block: counted in lane 0 of a vector register through hdr[0] -- a value the lanes share would take two
  //  scalar registers across every loop and a compare of the lane id two more, which the scalar file has no room for
  [[maybe_unused]] uint64_t counted = 0;
  for (uint64_t i = (uint64_t)blockIdx.x * PL_WAVES + wave; i < P.n; i += P.n_waves) {
    const uint32_t o0 = P.gene_off[i], o1 = P.gene_off[i + 1];
    if (o1 <= o0 || o1 > P.cap) continue;
    for (uint32_t m = 0; m < 2; ++m) {
      if (!P.seq[m]) continue;
      // (a single-end batch: mate 2's records are all zero, and they lie behind mate 1's -- lanes 16 .. 31 store them with mate 1's)
      uint32_t n_store;
      if constexpr (EXT || ACC) n_store = P.n_store[m];
      else n_store = m == 0u && !P.seq[1] ? 2u * AL_WORDS : AL_WORDS;
      Mate M{};
      const uint64_t a = P.off[m][i], len = P.off[m][i + 1] - a;
      M.L = len > 0x7FFFFFFFull ? 0x7FFFFFFFu : (uint32_t)len;   // (segments_kernel's L)
      M.seq = P.seq[m] + a;
      M.qual = P.qual[m] ? P.qual[m] + a : nullptr;
      M.mq = P.mq;
      for (uint32_t j = o0; j < o1; ++j) {
        const uint32_t g = P.gene_ids[j];
        uint32_t word = 0;                        // this lane's dword of the record (lanes 0 .. 15)
        uint32_t n_blocks = 0;
        [[maybe_unused]] uint32_t matches = 0, mismatches = 0;
        [[maybe_unused]] uint32_t tally = 0;      // (EXT, ACC) matches in lane 2, mismatches in lane 3
        if (g < P.n_genes) {
          const uint64_t start = P.gene_start[g];
          const int32_t len_g = (int32_t)(P.gene_start[g + 1] - start);   // (a record has fewer than 2^31 bases: the placement table's bound)
          const uint8_t *const rec = P.recbase + start;
          [[maybe_unused]] const int32_t L = (int32_t)M.L;
          // (ACC) this lane's counters of record base `lane` of the gene: a vector value for the same reason
          [[maybe_unused]] uint32_t *lane_counts = nullptr;
          if constexpr (ACC) lane_counts = P.counts + (start + lane) * 4u;
          const shk_segment *e = P.entries + ((uint64_t)j * 2u + m) * SHK_MAX_SEGMENTS;
          M.strand = e[0].strand;   // (rank 0's: every kept span lies on it)
          KeptSpans S = kept_spans(e, M.L, P.k, P.s_min);
          int32_t reach = 0, cursor = 0;
          int32_t ax = 0, aq = 0, al = 0;         // the open block (al == 0: none yet)
          // One pass per kept span and a last one that only closes the open block.  The pass always reads span 0 and then moves the
          // others down, so the loop needs no unrolling to keep its indices constant, and the code that finishes a block exists once.
#pragma nounroll
          for (uint32_t r = 0; r <= S.n; ++r) {
            int32_t bx = 0, bq = 0, bl = 0;       // the block of this pass (bl == 0: none)
            if (r < S.n) {
              // pileup's owned piece
              const int32_t lo = S.lo[0] > reach ? S.lo[0] : reach;
              const int32_t hi = S.hi[0] < len_g ? S.hi[0] : len_g;
              const int32_t pos = S.pos[0];
              reach = S.hi[0] > reach ? S.hi[0] : reach;
              S.lo[0] = S.lo[1]; S.lo[1] = S.lo[2]; S.lo[2] = S.lo[3];
              S.hi[0] = S.hi[1]; S.hi[1] = S.hi[2]; S.hi[2] = S.hi[3];
              S.pos[0] = S.pos[1]; S.pos[1] = S.pos[2]; S.pos[2] = S.pos[3];
              // trimmed by the read bases the blocks before it have explained
              const int32_t over = cursor - (lo - pos);
              const int32_t from = lo + (over > 0 ? over : 0);
              if (hi > lo && from < hi) {
                bx = from; bq = from - pos; bl = hi - from;
                cursor = bq + bl;
              }
              if (!bl) continue;
            }
            if (al) {
              if constexpr (SPL) {
                // Step 3b stands behind step 3: the gap behind the open block is closed first (below it then finds R == 0).
                if (bl) {
                  const int32_t R = bq - (aq + al), G = bx - (ax + al);
                  if (R >= 1 && R <= (int32_t)AL_MAX_CLOSE && G >= R) {
                    const int32_t s = (int32_t)close_gap(M, rec, len_g, aq + al, ax + al, bx, (uint32_t)R, lane);
                    al += s;
                    bx -= R - s; bq -= R - s; bl += R - s;
                  }
                }
                // Block 0 is about to be finished: its left end across a junction, where the mate has at most 3 blocks -- block 0, this
                // pass's, and those the spans still ahead yield, which trimming alone decides: the walk is done ahead over them.  A placement
                // makes the NEW block the open block and the shortened block 0 this pass's; the block this pass had goes back to the walk as
                // span 0 (or, in the last pass, the pass comes again), so the new block is finished here, in the one place that finishes blocks
                if (!n_blocks && aq >= (int32_t)(P.spl_prm & 255u) && aq <= (int32_t)SHK_SPLICE_MAX_OVERHANG) {
                  uint32_t more = bl ? 1u : 0u;
                  int32_t reach_w = reach, cursor_w = cursor;
#pragma unroll
                  for (uint32_t t = 0; t + 2u < SHK_MAX_SEGMENTS; ++t) {
                    if (r + 1u + t < S.n) {
                      const int32_t lo = S.lo[t] > reach_w ? S.lo[t] : reach_w;
                      const int32_t hi = S.hi[t] < len_g ? S.hi[t] : len_g;
                      reach_w = S.hi[t] > reach_w ? S.hi[t] : reach_w;
                      const int32_t over = cursor_w - (lo - S.pos[t]);
                      if (hi > lo && lo + (over > 0 ? over : 0) < hi) {
                        cursor_w = hi - S.pos[t];
                        ++more;
                      }
                    }
                  }
                  if (more <= 2u) {
                    uint32_t n_sites;
                    const uint2 *const sites = splice_sites(P.spl, P.n_genes, P.gene_ids[j], true, n_sites);
                    const int32_t B = al - 1 < (int32_t)SHK_SPLICE_BACK ? al - 1 : (int32_t)SHK_SPLICE_BACK;
                    int32_t d, a;
                    const uint32_t b = (int32_t)lane < aq + B ? read_base(M, (int32_t)lane) : 4u;
                    if (splice_end<true>(b, rec, len_g, sites, n_sites, ax - aq + 1, ax + B, ax - aq, ax - aq, (uint32_t)(aq + B), (P.spl_prm >> 8) & 255u,
                                         P.spl_prm >> 16, lane, d, a)) {
                      if (bl) {
                        S.lo[3] = S.lo[2]; S.lo[2] = S.lo[1]; S.lo[1] = S.lo[0]; S.lo[0] = bx;
                        S.hi[3] = S.hi[2]; S.hi[2] = S.hi[1]; S.hi[1] = S.hi[0]; S.hi[0] = bx + bl;
                        S.pos[3] = S.pos[2]; S.pos[2] = S.pos[1]; S.pos[1] = S.pos[0]; S.pos[0] = bx - bq;
                        reach = 0;       // (the span sets it again: it reached furthest, or it had yielded no block)
                        cursor = bq;
                      }
                      const int32_t n = aq - ax + a;
                      bx = a; bq = n; bl = al - (a - ax);
                      ax = d - n; aq = 0; al = n;
                      --r;
                    }
                  }
                }
                // the last pass: the right end across a junction, where the mate has at most 3 blocks with the open one (the pass comes
                // again for the new block, whose h is 0)
                if (!bl && n_blocks <= 2u) {
                  const int32_t xe = ax + al, qe = aq + al, h = L - qe;
                  if (h >= (int32_t)(P.spl_prm & 255u) && h <= (int32_t)SHK_SPLICE_MAX_OVERHANG) {
                    uint32_t n_sites;
                    const uint2 *const sites = splice_sites(P.spl, P.n_genes, P.gene_ids[j], false, n_sites);
                    const int32_t B = al - 1 < (int32_t)SHK_SPLICE_BACK ? al - 1 : (int32_t)SHK_SPLICE_BACK;
                    int32_t d, a;
                    const uint32_t b = (int32_t)lane < B + h ? read_base(M, qe - B + (int32_t)lane) : 4u;
                    if (splice_end<false>(b, rec, len_g, sites, n_sites, xe - B, xe + h - 1, xe + h, xe - B, (uint32_t)(B + h), (P.spl_prm >> 8) & 255u,
                                          P.spl_prm >> 16, lane, d, a)) {
                      al += d - xe;
                      bx = a; bq = qe + (d - xe); bl = h - (d - xe);
                      --r;
                    }
                  }
                }
                if constexpr (EXT) {
                  // step 3a's left end, behind step 3b: block 0 as it is finished (a placed end has no clip left: H == 0)
                  if (!n_blocks) {
                    const int32_t H = aq < ax ? aq : ax;
                    if (H > 0) {
                      const int32_t e = (int32_t)extend_end(M, rec, len_g, aq - 1, ax - 1, -1, H, aq <= ax, P.ext_p, P.ext_b, lane);
                      ax -= e; aq -= e; al += e;
                    }
                  }
                }
              }
              if constexpr (EXT) {
                // the last pass: the open block is the last one, its right end is extended before it is counted
                if (!bl) {
                  const int32_t hq = L - (aq + al), hx = len_g - (ax + al), H = hq < hx ? hq : hx;
                  if (H > 0) al += (int32_t)extend_end(M, rec, len_g, aq + al, ax + al, 1, H, hq <= hx, P.ext_p, P.ext_b, lane);
                }
              }
              if (!SPL && bl) {
                const int32_t R = bq - (aq + al), G = bx - (ax + al);
                if (R >= 1 && R <= (int32_t)AL_MAX_CLOSE && G >= R) {
                  const int32_t s = (int32_t)close_gap(M, rec, len_g, aq + al, ax + al, bx, (uint32_t)R, lane);
                  al += s;
                  bx -= R - s; bq -= R - s; bl += R - s;
                }
              }
              // A is final: counted over its bases, 64 per pass, and handed to the three lanes that store it
              for (int32_t t0 = 0; t0 < al; t0 += 64) {
                const int32_t t = t0 + (int32_t)lane;
                bool is_m = false, is_x = false;
                [[maybe_unused]] uint32_t seen = 4u;   // (ACC) the read base this lane observes; 4: none
                if (t < al) {
                  const uint32_t b = read_base(M, aq + t), rb = record_base(rec, len_g, ax + t);
                  is_m = b < 4u && b == rb;
                  is_x = b < 4u && rb < 4u && b != rb;
                  // (a block lies inside the record: the compare keeps a lane inside the state whatever the records hold)
                  if constexpr (ACC) seen = (uint32_t)(ax + t) < (uint32_t)len_g ? b : 4u;
                }
                if constexpr (ACC) {
                  // pileup's OBSERVATION at the base's record coordinate (behind the compare above, not inside it: one level of lane masks)
                  if (seen < 4u) atomicAdd(lane_counts + ((uint64_t)(uint32_t)(ax + t0) * 4u + seen), 1u);
                }
                if constexpr (EXT || ACC) {
                  // (the new instantiations count in the lanes that store the two words: two scalar registers fewer across the loops)
                  tally += ((uint32_t)__popcll(__ballot(is_m)) & hdr[2]) | ((uint32_t)__popcll(__ballot(is_x)) & hdr[3]);
                } else {
                  matches += (uint32_t)__popcll(__ballot(is_m));
                  mismatches += (uint32_t)__popcll(__ballot(is_x));
                }
              }
              const uint32_t w = lane - (4u + 3u * n_blocks);
              word = w == 0u ? (uint32_t)ax : (w == 1u ? (uint32_t)aq : (w == 2u ? (uint32_t)al : word));
              ++n_blocks;
            }
            if constexpr (EXT && !SPL) {
              // the first block becomes the open block: its left end is extended (closure moves only A's right and B's left)
              if (!n_blocks && bl) {
                const int32_t H = bq < bx ? bq : bx;
                if (H > 0) {
                  const int32_t e = (int32_t)extend_end(M, rec, len_g, bq - 1, bx - 1, -1, H, bq <= bx, P.ext_p, P.ext_b, lane);
                  bx -= e; bq -= e; bl += e;
                }
              }
            }
            ax = bx; aq = bq; al = bl;
          }
        }
        if constexpr (ACC) counted += (n_blocks ? 1u : 0u) & hdr[0];
        if (n_blocks) {
          if constexpr (EXT || ACC) word = (word & ~hdr_any) | (n_blocks & hdr[0]) | (M.strand & hdr[1]) | tally;
          else word = (word & ~hdr_any) | (n_blocks & hdr[0]) | (M.strand & hdr[1]) | (matches & hdr[2]) | (mismatches & hdr[3]);
        }
        if (lane < n_store) P.out[((uint64_t)j * 2u + m) * AL_WORDS + lane] = word;   // (ACC without records: n_store is 0)
      }
    }
  }
  if constexpr (ACC) {
    if (counted) atomicAdd(P.mates, (unsigned long long)counted);
  }
}

}  // namespace

// the launch: records (store) at floor s_min into out[0 .. out_cap) and / or the final blocks' bases (accumulate) into Ctx::pileup
static int launch_align_kernel(Ctx *ctx, const Slot &s, const shk_segment *entries, uint64_t cap_assoc, bool skip_if_long, bool store, bool accumulate, uint32_t s_min,
                               shk_mate_alignment *out, uint64_t out_cap, hipStream_t stream)
{
  const DeviceIndex &ix = ctx->idx;
  AlignParamsS P{};
  P.gene_off = s.d_gene_off.p;
  P.gene_ids = s.d_gene_ids.p;
  P.counters = s.d_counters;
  P.n = s.n;
  P.cap = (uint32_t)std::min<uint64_t>(std::min<uint64_t>(std::min<uint64_t>(s.d_gene_ids.cap, cap_assoc), store ? out_cap / 2 : ~0ull), 0xFFFFFFFFull);   // (launch_segments')
  P.seq[0] = s.p.seq1; P.off[0] = s.p.off1; P.qual[0] = s.p.hasq ? s.p.qual1 : nullptr;
  P.seq[1] = s.p.seq2; P.off[1] = s.p.off2; P.qual[1] = s.p.hasq ? s.p.qual2 : nullptr;
  P.mq = s.p.mq;
  P.k = s.p.k;
  P.entries = entries;
  P.gene_start = ix.gene_start;
  P.recbase = ix.recbase;
  P.n_genes = (uint32_t)(ctx->gene_start.size() - 1);
  P.skip_if_long = skip_if_long ? 1u : 0u;
  P.s_min = s_min;
  P.out = store ? reinterpret_cast<uint32_t *>(out) : nullptr;
  P.n_store[0] = !store ? 0u : (P.seq[1] ? AL_WORDS : 2u * AL_WORDS);
  P.n_store[1] = !store ? 0u : AL_WORDS;
  P.ext_p = s.ext_p;
  P.ext_b = s.ext_b;
  P.counts = accumulate ? ctx->pileup.counts.p : nullptr;
  P.mates = accumulate ? ctx->pileup.mates.p : nullptr;
  // one wave per read up to 2 048 workgroups, persistent beyond (launch_segments' bound)
  const unsigned blocks = (unsigned)std::min<uint64_t>((s.n + PL_WAVES - 1) / PL_WAVES, 2048);
  P.n_waves = blocks * PL_WAVES;
  const bool ext = s.ext_p != 0;
  // step 3b as submitted; the list is the context's (it changes only while no ticket is outstanding)
  const bool spl = s.spl_h != 0;
  if (spl && !ctx->splice.d.p) {
    ctx->last_error = "spliced ends without a site list";
    return SHK_ERR_STATE;
  }
  P.spl = ctx->splice.d.p;
  P.spl_prm = s.spl_h | s.spl_cost << 8 | s.spl_gap << 16;   // (at most 48, 64, 64)
  const AlignParamsX &PX = P;
  // (everything new off: the kernel and the arguments this mode always had)
  if (spl) {
    if (!ext && !accumulate) hipLaunchKernelGGL((align_kernel<false, false, true, AlignParamsS>), dim3(blocks), dim3(PL_THREADS), 0, stream, P);
    else if (ext && !accumulate) hipLaunchKernelGGL((align_kernel<true, false, true, AlignParamsS>), dim3(blocks), dim3(PL_THREADS), 0, stream, P);
    else if (!ext) hipLaunchKernelGGL((align_kernel<false, true, true, AlignParamsS>), dim3(blocks), dim3(PL_THREADS), 0, stream, P);
    else hipLaunchKernelGGL((align_kernel<true, true, true, AlignParamsS>), dim3(blocks), dim3(PL_THREADS), 0, stream, P);
  } else if (!ext && !accumulate) hipLaunchKernelGGL((align_kernel<false, false, false, AlignParams>), dim3(blocks), dim3(PL_THREADS), 0, stream, static_cast<const AlignParams &>(P));
  else if (ext && !accumulate) hipLaunchKernelGGL((align_kernel<true, false, false, AlignParamsX>), dim3(blocks), dim3(PL_THREADS), 0, stream, PX);
  else if (!ext) hipLaunchKernelGGL((align_kernel<false, true, false, AlignParamsX>), dim3(blocks), dim3(PL_THREADS), 0, stream, PX);
  else hipLaunchKernelGGL((align_kernel<true, true, false, AlignParamsX>), dim3(blocks), dim3(PL_THREADS), 0, stream, PX);
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? SHK_OK : set_hip_error(ctx, e, "align_kernel");
}

int launch_alignments(Ctx *ctx, const Slot &s, const shk_segment *entries, uint64_t cap_assoc, bool skip_if_long, bool store, bool accumulate, hipStream_t stream)
{
  const DeviceIndex &ix = ctx->idx;
  if (!ix.gene_start || !ix.recbase || !entries || (!store && !accumulate) || (store && (!s.align || !s.rec_align.d.p))) {
    ctx->last_error = "alignments mode without its state";
    return SHK_ERR_STATE;
  }
  if (accumulate && (!s.pileup_al || !ctx->pileup.counts.p || !ctx->pileup.mates.p || (store && s.align != s.pileup_al))) {
    ctx->last_error = "aligned pileup without its state";
    return SHK_ERR_STATE;
  }
  if (s.n == 0) return SHK_OK;
  return launch_align_kernel(ctx, s, entries, cap_assoc, skip_if_long, store, accumulate, store ? s.align : s.pileup_al, s.rec_align.d.p, s.rec_align.d.cap, stream);
}

int launch_alignments_into(Ctx *ctx, const Slot &s, const shk_segment *entries, uint64_t cap_assoc, bool skip_if_long, uint32_t s_min, shk_mate_alignment *out,
                           uint64_t out_cap, hipStream_t stream)
{
  const DeviceIndex &ix = ctx->idx;
  if (!ix.gene_start || !ix.recbase || !entries || !s_min || !out) {
    ctx->last_error = "alignment records of the context's own without their state";
    return SHK_ERR_STATE;
  }
  if (s.n == 0) return SHK_OK;
  return launch_align_kernel(ctx, s, entries, cap_assoc, skip_if_long, true, false, s_min, out, out_cap, stream);
}

}  // namespace shk
