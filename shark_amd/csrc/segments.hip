// segments.hip -- segments mode's kernel (gfx950): per association (read, gene) of a finished batch and per mate the m diagonals of
// the gene's record with the most votes, each with the first and the last slot that voted for it, and the number of distinct
// diagonals (include/shark_hip.h, "segments").  An RNA-Seq mate that crosses an exon junction lies on two or more
// diagonals of its gene's genomic record, an intron apart; placement mode keeps one of them.
//
// placement_kernel's shape (placement.hip): behind the assembly of gene_off / gene_ids on the batch's compute stream, one wavefront
// per read with associations, a mate's windows computed once and its first PL_CACHED_CHUNKS x 64 slots kept in LDS, the slots of a
// longer mate recomputed per pass, persistent waves.  The search is placement's as well -- the wave-minimum key not yet counted, one
// ballot per chunk of 64 slots for its votes -- and keeps more of what the ballots say: the first non-empty ballot's lowest set bit is
// the key's first voting slot, the last non-empty ballot's highest set bit its last one.  Ballots are wave-uniform, so this is scalar
// work next to the popcount already taken; no cross-lane reduction is added per key (the one wave minimum per key is placement's).
//
// The top SHK_MAX_SEGMENTS keys live in wave-uniform registers (constant indices only: no scratch memory).  Keys arrive in ascending
// order -- strand 0 first, then the smaller pos -- and a key goes in front of the entries it beats with a STRICT >, so among equal
// supports the earlier key stays ahead: placement's tie rule, entry 0 is the mate's shk_mate_placement.  Nothing is capped.
//
// Cost bound: placement_kernel's -- (D + 1) passes over the mate's chunks for D distinct keys -- plus 4 + 20 m bytes stored per mate.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "placement_common.hpp"
#include "shark_internal.hpp"

namespace shk {

namespace {

constexpr uint32_t SEG_WORDS = sizeof(shk_segment) / sizeof(uint32_t);   // 5
static_assert(sizeof(shk_segment) == 20 && SHK_MAX_SEGMENTS * SEG_WORDS <= 64, "one lane per word of a mate's entries");

struct SegParams {
  const uint32_t *gene_off;
  const uint16_t *gene_ids;
  const uint32_t *counters;
  uint64_t n, cap;             // reads; associations the output arrays hold
  const uint8_t *seq[2];
  const uint64_t *off[2];
  const uint8_t *qual[2];      // nullptr: no masking
  int32_t mq;
  uint32_t k;
  const uint4 *ptab;
  const uint32_t *pdir;
  uint32_t ptab_lg;
  uint32_t m;                  // entries per mate, 1 .. SHK_MAX_SEGMENTS
  uint32_t *n_keys;            // [j * 2 + mate]
  uint32_t *entries;           // shk_segment as words: [((j * 2 + mate) * m + r) * 5 + word]
};

// a value that is the same in every lane, moved to where the compiler knows it
__device__ __forceinline__ uint64_t uniform_u64(uint64_t v)
{
  const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)v), hi = __builtin_amdgcn_readfirstlane((uint32_t)(v >> 32));
  return ((uint64_t)hi << 32) | lo;
}

__global__ __launch_bounds__(PL_THREADS) void segments_kernel(const SegParams P)
{
  __shared__ uint64_t s_kmer[PL_WAVES][PL_CACHED_CHUNKS * 64];
  __shared__ uint64_t s_vote[PL_WAVES][PL_CACHED_CHUNKS * 64];
  // (a batch with more associations than gene_ids holds is assembled again by the host's slow path, and comes through here again)
  if (P.counters[CTR_OVERFLOW]) return;
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  const uint32_t lane_r = lane / SEG_WORDS, lane_w = lane % SEG_WORDS;   // the entry and the word of it this lane stores
  uint64_t *const kmers = s_kmer[wave], *const votes = s_vote[wave];
  const uint64_t n_waves = (uint64_t)gridDim.x * PL_WAVES;
  for (uint64_t i = (uint64_t)blockIdx.x * PL_WAVES + wave; i < P.n; i += n_waves) {
    const uint32_t o0 = P.gene_off[i], o1 = P.gene_off[i + 1];
    if (o1 <= o0 || o1 > P.cap) continue;
    for (uint32_t m = 0; m < 2; ++m) {
      uint32_t L = 0, n_slots = 0;
      const uint8_t *seq = nullptr, *qual = nullptr;
      if (P.seq[m]) {
        const uint64_t a = P.off[m][i], len = P.off[m][i + 1] - a;
        L = len > 0x7FFFFFFFull ? 0x7FFFFFFFu : (uint32_t)len;
        seq = P.seq[m] + a;
        qual = P.qual[m] ? P.qual[m] + a : nullptr;
        n_slots = L >= P.k ? L - P.k + 1u : 0u;
      }
      const uint32_t n_chunks = (n_slots + 63u) >> 6;
      const uint32_t n_cached = n_chunks < PL_CACHED_CHUNKS ? n_chunks : PL_CACHED_CHUNKS;
      for (uint32_t c = 0; c < n_cached; ++c) {
        const uint32_t p = c * 64u + lane;
        kmers[p] = p < n_slots ? pl_window(seq + p, qual ? qual + p : nullptr, P.mq, P.k) : PL_NO_KMER;
      }
      for (uint32_t j = o0; j < o1; ++j) {
        const uint32_t g = P.gene_ids[j];
        for (uint32_t c = 0; c < n_cached; ++c) {
          const uint32_t p = c * 64u + lane;
          votes[p] = pl_vote(P, g, kmers[p], p, L);
        }
        // rank order: t_cnt descending; an empty entry has t_cnt 0 (a key has at least one vote)
        uint64_t t_key[SHK_MAX_SEGMENTS];
        uint32_t t_cnt[SHK_MAX_SEGMENTS], t_first[SHK_MAX_SEGMENTS], t_last[SHK_MAX_SEGMENTS];
#pragma unroll
        for (int r = 0; r < SHK_MAX_SEGMENTS; ++r) { t_key[r] = 0; t_cnt[r] = 0; t_first[r] = 0; t_last[r] = 0; }
        bool have = false;
        uint64_t cur = 0;
        uint32_t n_keys = 0;
        while (true) {
          uint32_t cnt = 0, first = 0, last = 0;
          uint64_t mn = PL_NO_VOTE;
          for (uint32_t c = 0; c < n_chunks; ++c) {
            const uint32_t p = c * 64u + lane;
            uint64_t v;
            if (c < n_cached) v = votes[p];
            else v = p < n_slots ? pl_vote(P, g, pl_window(seq + p, qual ? qual + p : nullptr, P.mq, P.k), p, L) : PL_NO_VOTE;
            if (have) {
              const uint64_t b = __ballot(v == cur);
              if (b) {
                if (!cnt) first = c * 64u + (uint32_t)__builtin_ctzll(b);
                last = c * 64u + 63u - (uint32_t)__builtin_clzll(b);
                cnt += (uint32_t)__builtin_popcountll(b);
              }
            }
            if (v != PL_NO_VOTE && (!have || v > cur) && v < mn) mn = v;
          }
          mn = uniform_u64(wave_min_u64(mn));
          if (have) {
            // cur goes in front of the first entry it beats, the entries behind move down one, the last one leaves
            ++n_keys;
            bool ins = false;
            uint64_t e_key = cur;
            uint32_t e_cnt = cnt, e_first = first, e_last = last;
#pragma unroll
            for (int r = 0; r < SHK_MAX_SEGMENTS; ++r) {
              ins = ins || e_cnt > t_cnt[r];
              if (ins) {
                const uint64_t xk = t_key[r]; t_key[r] = e_key; e_key = xk;
                const uint32_t xc = t_cnt[r]; t_cnt[r] = e_cnt; e_cnt = xc;
                const uint32_t xf = t_first[r]; t_first[r] = e_first; e_first = xf;
                const uint32_t xl = t_last[r]; t_last[r] = e_last; e_last = xl;
              }
            }
          }
          if (mn == PL_NO_VOTE) break;
          cur = mn;
          have = true;
        }
        // one lane per word of the mate's m entries, and one for their header
        uint32_t val = 0;
#pragma unroll
        for (int r = 0; r < SHK_MAX_SEGMENTS; ++r)
          if (lane_r == (uint32_t)r && t_cnt[r]) {
            val = lane_w == 0 ? (uint32_t)pl_vote_pos(t_key[r])
                : lane_w == 1 ? t_cnt[r]
                : lane_w == 2 ? pl_vote_strand(t_key[r])
                : lane_w == 3 ? t_first[r] : t_last[r];
          }
        const uint64_t e = (uint64_t)j * 2u + m;
        if (lane < P.m * SEG_WORDS) P.entries[e * P.m * SEG_WORDS + lane] = val;
        if (lane == 63u) P.n_keys[e] = n_keys;
      }
    }
  }
}

}  // namespace

int launch_segments_into(Ctx *ctx, const Slot &s, uint32_t m, uint32_t *d_keys, shk_segment *d_entries, uint64_t cap_assoc, hipStream_t stream)
{
  const DeviceIndex &ix = ctx->idx;
  if (!ix.ptab_lg || !ix.ptab || !ix.pdir || !d_keys || !d_entries || !m || m > SHK_MAX_SEGMENTS) {
    ctx->last_error = "segments mode without its table";
    return SHK_ERR_STATE;
  }
  if (s.n == 0) return SHK_OK;
  SegParams P{};
  P.gene_off = s.d_gene_off.p;
  P.gene_ids = s.d_gene_ids.p;
  P.counters = s.d_counters;
  P.n = s.n;
  P.cap = std::min<uint64_t>(std::min<uint64_t>(s.d_gene_ids.cap, cap_assoc), 0xFFFFFFFFull);
  P.seq[0] = s.p.seq1; P.off[0] = s.p.off1; P.qual[0] = s.p.hasq ? s.p.qual1 : nullptr;
  P.seq[1] = s.p.seq2; P.off[1] = s.p.off2; P.qual[1] = s.p.hasq ? s.p.qual2 : nullptr;
  P.mq = s.p.mq;
  P.k = s.p.k;
  P.ptab = ix.ptab;
  P.pdir = ix.pdir;
  P.ptab_lg = ix.ptab_lg;
  P.m = m;
  P.n_keys = d_keys;
  P.entries = reinterpret_cast<uint32_t *>(d_entries);
  // one wave per read up to eight workgroups per CU's worth of them, persistent beyond (launch_placement's bound)
  const uint64_t want = (s.n + PL_WAVES - 1) / PL_WAVES;
  hipLaunchKernelGGL(segments_kernel, dim3((unsigned)std::min<uint64_t>(want, 2048)), dim3(PL_THREADS), 0, stream, P);
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? SHK_OK : set_hip_error(ctx, e, "segments_kernel");
}

int launch_segments(Ctx *ctx, const Slot &s, hipStream_t stream)
{
  return launch_segments_into(ctx, s, s.seg_m, s.rec_seg_keys.d.p, s.rec_seg_entries.d.p, segments_cap(s.rec_seg_keys.d, s.rec_seg_entries.d, s.seg_m), stream);
}

}  // namespace shk
