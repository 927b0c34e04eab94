// placement.hip -- placement mode's kernel (gfx950): per association (read, gene) of a finished batch and per mate the diagonal of
// the gene's record that most of the mate's k-mers lie on (include/shark_hip.h, "placement").
//
// Runs on the batch's compute stream behind the assembly of gene_off / gene_ids (scan, gather, EMIT pass), so it sees the final
// associations whichever kernels produced them, and needs no host round trip: the grid is sized from the batch, its waves are
// persistent, a read without associations costs two loads and a compare.
//
// One wavefront per read with associations.  Per mate the windows' canonical k-mers are computed once (lane l takes slots
// l, l + 64, ...; the first PL_CACHED_CHUNKS x 64 are kept in LDS, each lane reading back only what it wrote, the slots of a
// longer mate are recomputed where they are needed -- any length is served here).  Per association every valid slot is looked up
// in DeviceIndex::ptab -- the directory's two words, then the bucket's 16-byte entries, compared in full -- and becomes a vote
// (strand, pos) packed so that unsigned order is "strand 0 first, then the smaller pos".  The winner is found the way the vote
// walks genes: take the wave-minimum key not yet counted, ballot and popcount its votes, keep it if the count is STRICTLY larger;
// ascending order and the strict > give the tie rule.  A read has one to three distinct keys as a rule.
//
// Cost bound.  The search makes one pass over the mate's chunks per DISTINCT key D, plus one.  For a mate of up to 512 slots a pass
// reads LDS only: (D + 1) x 8 chunk steps, the lookups done once.  Beyond 512 slots a pass recomputes the windows of the slots behind
// the cached ones and looks them up again: (D + 1) x (slots - 512) lookups per association, D <= the mate's unique-k-mer slots.  A
// read along its gene has D = 1 + its indels (the 1 500-base reads of the tests: 2 to 3); D grows only where a long mate hits
// thousands of different diagonals of one record by k-mers UNIQUE in it -- repeats do not do that, their k-mers are ambiguous and do
// not vote -- and then it is one wave that runs long, the others go on.  Nothing is capped: a cap would change the answer.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "placement_common.hpp"
#include "shark_internal.hpp"

namespace shk {

namespace {

struct PlaceParams {
  const uint32_t *gene_off;
  const uint16_t *gene_ids;
  const uint32_t *counters;
  uint64_t n, cap;             // reads; records `out` holds
  const uint8_t *seq[2];
  const uint64_t *off[2];
  const uint8_t *qual[2];      // nullptr: no masking
  int32_t mq;
  uint32_t k;
  const uint4 *ptab;
  const uint32_t *pdir;
  uint32_t ptab_lg;
  shk_placement *out;
};

__global__ __launch_bounds__(PL_THREADS) void placement_kernel(const PlaceParams P)
{
  __shared__ uint64_t s_kmer[PL_WAVES][PL_CACHED_CHUNKS * 64];
  __shared__ uint64_t s_vote[PL_WAVES][PL_CACHED_CHUNKS * 64];
  // (a batch with more associations than gene_ids holds is assembled again by the host's slow path, and comes through here again)
  if (P.counters[CTR_OVERFLOW]) return;
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
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
        bool have = false;
        uint64_t cur = 0, best_key = 0;
        uint32_t best_cnt = 0;
        while (true) {
          uint32_t cnt = 0;
          uint64_t mn = PL_NO_VOTE;
          for (uint32_t c = 0; c < n_chunks; ++c) {
            const uint32_t p = c * 64u + lane;
            uint64_t v;
            if (c < n_cached) v = votes[p];
            else v = p < n_slots ? pl_vote(P, g, pl_window(seq + p, qual ? qual + p : nullptr, P.mq, P.k), p, L) : PL_NO_VOTE;
            if (have) cnt += (uint32_t)__builtin_popcountll(__ballot(v == cur));
            if (v != PL_NO_VOTE && (!have || v > cur) && v < mn) mn = v;
          }
          mn = wave_min_u64(mn);
          if (have && cnt > best_cnt) { best_cnt = cnt; best_key = cur; }
          if (mn == PL_NO_VOTE) break;
          cur = mn;
          have = true;
        }
        if (lane == 0) {
          shk_mate_placement r;
          r.pos = best_cnt ? (int32_t)((uint32_t)best_key ^ 0x80000000u) : 0;
          r.support = best_cnt;
          r.strand = best_cnt ? (uint32_t)(best_key >> 32) : 0u;
          P.out[j].mate[m] = r;
        }
      }
    }
  }
}

}  // namespace

int launch_placement(Ctx *ctx, const Slot &s, hipStream_t stream)
{
  const DeviceIndex &ix = ctx->idx;
  if (!ix.ptab_lg || !ix.ptab || !ix.pdir || !s.rec_place.d.p) { ctx->last_error = "placement mode without its table"; return SHK_ERR_STATE; }
  if (s.n == 0) return SHK_OK;
  PlaceParams P{};
  P.gene_off = s.d_gene_off.p;
  P.gene_ids = s.d_gene_ids.p;
  P.counters = s.d_counters;
  P.n = s.n;
  P.cap = std::min<uint64_t>(std::min<uint64_t>(s.d_gene_ids.cap, s.rec_place.d.cap), 0xFFFFFFFFull);
  P.seq[0] = s.p.seq1; P.off[0] = s.p.off1; P.qual[0] = s.p.hasq ? s.p.qual1 : nullptr;
  P.seq[1] = s.p.seq2; P.off[1] = s.p.off2; P.qual[1] = s.p.hasq ? s.p.qual2 : nullptr;
  P.mq = s.p.mq;
  P.k = s.p.k;
  P.ptab = ix.ptab;
  P.pdir = ix.pdir;
  P.ptab_lg = ix.ptab_lg;
  P.out = s.rec_place.d.p;
  // one wave per read up to eight workgroups per CU's worth of them, persistent beyond
  const uint64_t want = (s.n + PL_WAVES - 1) / PL_WAVES;
  hipLaunchKernelGGL(placement_kernel, dim3((unsigned)std::min<uint64_t>(want, 2048)), dim3(PL_THREADS), 0, stream, P);
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? SHK_OK : set_hip_error(ctx, e, "placement_kernel");
}

}  // namespace shk
