// indels.hip -- indels mode on the device (gfx950): the insertions and deletions that the mates' alignments show, normalised and tabled
// over all counted batches (include/shark_hip.h, "indels").  It reads the 64-byte records align_kernel has just stored,
// directly behind that kernel in the batch's tail.
//
// indel_kernel has spliced_accumulate_kernel's outer shape: one lane per read, whole waves, persistent beyond 2 048 workgroups, the same
// three early returns.  A lane loads the first 16 bytes of its read's records, association by association and mate by mate, and is done with
// a record unless n_blocks >= 2 -- the common case, one 16-byte load per mate.  The lanes that hold a record with a gap are found by ballot;
// the wave takes them one at a time and works each record's gaps together, everything about the record wave-uniform:
//   - an insertion's <= 12 read bases are loaded by its first lanes, one ballot says whether all are bases, an OR over the wave packs them;
//   - left-normalisation runs 64 comparisons per pass: lane t compares record base xa - 1 - d - t with its partner (the record, or for an
//     insertion the inserted bases once the partner lies at or behind xa), one ballot, d grows by the leading agreeing lanes, and the loop
//     goes on while all 64 agree;
//   - lane 0 claims the key as junction_insert does (spliced.hip): a 64-bit compare-and-swap from empty, linear probing for at most
//     `capacity` steps, then one atomic add to fwd or rev.  A key never changes once set and additions commute: the table's CONTENT
//     is independent of scheduling.
// The stats are counted in registers and added with one atomic per wave and counter that is not zero.  No LDS, no inline assembly.
//
// indel_clear_kernel empties the table and zeroes the counters; indel_add_kernel adds a caller's validated entries, one lane each.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "placement_common.hpp"
#include "shark_internal.hpp"

namespace shk {

namespace {

constexpr int ID_THREADS = 256;
enum { ST_MATES = 0, ST_DEL = 1, ST_INS = 2, ST_COMPLEX = 3, ST_LONG = 4, ST_NONBASE = 5, ST_DROPPED = 6 };
static_assert(ST_DROPPED + 1 == INDEL_STATS, "shk_indel_stats' order");

struct IndelParams {
  const uint32_t *gene_off;
  const uint16_t *gene_ids;
  const uint32_t *counters;
  uint64_t n;                      // reads
  uint32_t cap;                    // associations `records` holds (align_kernel's cap)
  uint32_t skip_if_long;
  const uint8_t *seq[2];           // nullptr: the batch has no such mate
  const uint64_t *off[2];
  const uint8_t *qual[2];          // nullptr: no masking
  int32_t mq;
  uint32_t min_intron;
  const uint32_t *records;         // [(j * 2 + mate) * 16 + w]: shk_mate_alignment
  const uint64_t *gene_start;
  const uint8_t *recbase;          // [gene_start[g] + x]: 0 .. 3, every other byte 4
  uint32_t n_genes;                // entries of gene_start - 1
  IndelEntry *tab;
  uint64_t tab_mask;               // capacity - 1 (a power of two)
  unsigned long long *stats;       // INDEL_STATS counters
};

__device__ __forceinline__ uint32_t id_wave_or(uint32_t v)
{
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) v |= (uint32_t)__shfl_xor((int)v, o, 64);
  return v;
}
__device__ __forceinline__ uint32_t id_wave_max(uint32_t v)
{
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) {
    const uint32_t t = (uint32_t)__shfl_xor((int)v, o, 64);
    v = t > v ? t : v;
  }
  return v;
}
__device__ __forceinline__ uint32_t id_wave_sum(uint32_t v)
{
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) v += (uint32_t)__shfl_xor((int)v, o, 64);
  return v;
}

// the entry of `key`, claimed if the table has none; nullptr: the table is full
__device__ __forceinline__ IndelEntry *indel_find(IndelEntry *tab, uint64_t tab_mask, unsigned long long key)
{
  uint64_t h = ((key * 0x9E3779B97F4A7C15ull) >> 20) & tab_mask;
  for (uint64_t step = 0; step <= tab_mask; ++step) {
    IndelEntry *e = tab + h;
    unsigned long long cur = __hip_atomic_load(&e->key, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // (a key is set once: only `empty` can be stale, and the swap settles that)
    if (cur == INDEL_EMPTY) {
      cur = atomicCAS(&e->key, INDEL_EMPTY, key);
      if (cur == INDEL_EMPTY) cur = key;
    }
    if (cur == key) return e;
    h = (h + 1) & tab_mask;
  }
  return nullptr;
}

// the read base of read coordinate q on the record's strand (align.hip's read_base): 0 .. 3, or 4 for a byte that is no base, a masked one
// and a q outside the mate
__device__ __forceinline__ uint32_t id_read_base(const uint8_t *seq, const uint8_t *qual, int32_t mq, uint32_t L, uint32_t strand, int64_t q)
{
  if (q < 0 || q >= (int64_t)L) return 4u;
  const uint32_t idx = strand ? L - 1u - (uint32_t)q : (uint32_t)q;
  uint32_t ch = seq[idx];
  if (qual && (int32_t)(int8_t)qual[idx] < mq) ch = (ch - 64u) & 0xFFu;
  const uint32_t c = base_code(ch);
  return c < 4u ? (strand ? 3u - c : c) : 4u;
}

// The leading lanes that agree: how far this pass moves the event to the left (64: all of them, the next pass goes on)
__device__ __forceinline__ uint32_t leading_agree(bool ok)
{
  const unsigned long long bal = __ballot(ok);
  return bal == ~0ull ? 64u : (uint32_t)__ffsll((long long)~bal) - 1u;
}

__global__ __launch_bounds__(ID_THREADS) void indel_kernel(const IndelParams P)
{
  // the batch will be assembled again and comes through here again; or it will be refused in wait (depth_accumulate_kernel's rule)
  if (P.counters[CTR_OVERFLOW] || (P.skip_if_long && P.counters[CTR_LONG]) || P.counters[CTR_VOUCH_BAD]) return;
  const uint32_t lane = threadIdx.x & 63u;
  const uint64_t stride = (uint64_t)gridDim.x * ID_THREADS;
  uint32_t n_mates = 0;                                            // this lane's
  uint32_t st[INDEL_STATS] = {0u, 0u, 0u, 0u, 0u, 0u, 0u};         // the wave's (the same in every lane)
  for (uint64_t base = (uint64_t)blockIdx.x * ID_THREADS + (threadIdx.x & ~63u); base < P.n; base += stride) {
    const uint64_t i = base + lane;
    uint32_t o0 = 0, cnt = 0;
    if (i < P.n) {
      o0 = P.gene_off[i];
      const uint32_t o1 = P.gene_off[i + 1];
      if (o1 > o0 && o1 <= P.cap) cnt = o1 - o0;
    }
    const uint32_t max_cnt = id_wave_max(cnt);
    for (uint32_t a = 0; a < max_cnt; ++a) {
#pragma unroll
      for (uint32_t m = 0; m < 2; ++m) {
        if (!P.seq[m]) continue;
        uint32_t nb = 0;
        if (a < cnt) nb = reinterpret_cast<const uint4 *>(P.records)[((uint64_t)(o0 + a) * 2u + m) * 4u].x;
        n_mates += nb >= 1u ? 1u : 0u;
        unsigned long long todo = __ballot(nb >= 2u);
        while (todo) {
          const uint32_t src = (uint32_t)__ffsll((long long)todo) - 1u;
          todo &= todo - 1ull;
          // one record with a gap, the whole wave on it
          const uint32_t j = __builtin_amdgcn_readfirstlane(__shfl((int)(o0 + a), (int)src, 64));
          const uint64_t ri = base + src;
          const uint32_t g = P.gene_ids[j];
          if (g >= P.n_genes) continue;
          const uint64_t start = P.gene_start[g];
          const int64_t len_g = (int64_t)(P.gene_start[g + 1] - start);
          const uint8_t *const rec = P.recbase + start;
          const uint32_t *const w = P.records + ((uint64_t)j * 2u + m) * 16u;
          const uint32_t n_blocks = w[0] < SHK_MAX_SEGMENTS ? w[0] : SHK_MAX_SEGMENTS;
          const uint32_t strand = w[1] & 1u;
          const uint64_t ra = P.off[m][ri], rlen = P.off[m][ri + 1] - ra;
          const uint32_t L = rlen > 0x7FFFFFFFull ? 0x7FFFFFFFu : (uint32_t)rlen;   // (segments_kernel's L)
          const uint8_t *const rseq = P.seq[m] + ra;
          const uint8_t *const rqual = P.qual[m] ? P.qual[m] + ra : nullptr;
          for (uint32_t b = 0; b + 1u < n_blocks; ++b) {
            const int64_t xa = (int64_t)w[4u + 3u * b] + w[6u + 3u * b], qa = (int64_t)w[5u + 3u * b] + w[6u + 3u * b];
            const int64_t xb = w[7u + 3u * b], qb = w[8u + 3u * b], lb = w[9u + 3u * b];
            const int64_t R = qb - qa, G = xb - xa;
            // (align_kernel's blocks ascend without overlap inside the record; anything else is not a gap)
            if (R < 0 || G < 0 || lb == 0 || xb + lb > len_g) continue;
            uint32_t kind, len, seq = 0u, d = 0u;
            if (R == 0) {
              if (G < 1 || G >= (int64_t)P.min_intron) continue;
              ++st[ST_DEL];
              kind = 0u;
              len = (uint32_t)G;
              for (;;) {
                const int64_t x = xa - 1 - (int64_t)d - lane;
                bool ok = false;
                if (x >= 0) {
                  const uint32_t r0 = rec[x], r1 = rec[x + G];   // (x + G < xb <= len_g)
                  ok = r0 < 4u && r0 == r1;
                }
                const uint32_t run = leading_agree(ok);
                d += run;
                if (run < 64u) break;
              }
            } else if (G >= 1) {
              ++st[ST_COMPLEX];
              continue;
            } else {
              if (R > SHK_INDEL_MAX_INS) { ++st[ST_LONG]; continue; }
              uint32_t s = 0u;
              if (lane < (uint32_t)R) s = id_read_base(rseq, rqual, P.mq, L, strand, qa + lane);
              if (__ballot(s >= 4u)) { ++st[ST_NONBASE]; continue; }
              ++st[ST_INS];
              kind = 1u;
              len = (uint32_t)R;
              const uint32_t raw = id_wave_or(lane < len ? s << (2u * lane) : 0u);
              // T[j] = r[j] in front of xa, the inserted bases behind: T[x] against T[x + R]
              for (;;) {
                const int64_t x = xa - 1 - (int64_t)d - lane;
                bool ok = false;
                if (x >= 0) {
                  const int64_t y = x + R;
                  const uint32_t r0 = rec[x], r1 = y < xa ? (uint32_t)rec[y] : (raw >> (2u * (uint32_t)(y - xa))) & 3u;
                  ok = r0 < 4u && r0 == r1;
                }
                const uint32_t run = leading_agree(ok);
                d += run;
                if (run < 64u) break;
              }
              uint32_t v = 0u;
              if (lane < len) {
                const int64_t y = xa - (int64_t)d + lane;
                v = (y < xa ? (uint32_t)rec[y] & 3u : (raw >> (2u * (uint32_t)(y - xa))) & 3u) << (2u * lane);
              }
              seq = id_wave_or(v);
            }
            if (lane == 0u) {
              IndelEntry *e = indel_find(P.tab, P.tab_mask, indel_key(start + (uint64_t)(xa - (int64_t)d), kind, len, seq));
              if (e) atomicAdd(strand ? &e->rev : &e->fwd, 1u);
              else atomicAdd(P.stats + ST_DROPPED, 1ull);
            }
          }
        }
      }
    }
  }
  st[ST_MATES] = id_wave_sum(n_mates);
  if (lane == 0u) {
#pragma unroll
    for (uint32_t c = 0; c < ST_DROPPED; ++c)
      if (st[c]) atomicAdd(P.stats + c, (unsigned long long)st[c]);
  }
}

__global__ __launch_bounds__(256) void indel_clear_kernel(IndelEntry *__restrict__ tab, uint64_t capacity, unsigned long long *__restrict__ stats)
{
  const uint64_t tid = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x, nth = (uint64_t)gridDim.x * blockDim.x;
  for (uint64_t i = tid; i < capacity; i += nth) {
    IndelEntry e;
    e.key = INDEL_EMPTY;
    e.fwd = 0u;
    e.rev = 0u;
    tab[i] = e;
  }
  if (tid < INDEL_STATS) stats[tid] = 0ull;
}

// one lane per entry of a caller's table; lane 0 of the grid adds the caller's counters
__global__ __launch_bounds__(256) void indel_add_kernel(IndelEntry *__restrict__ tab, uint64_t tab_mask, unsigned long long *__restrict__ stats,
                                                         const IndelEntry *__restrict__ in, uint64_t n, const unsigned long long *__restrict__ add_stats)
{
  const uint64_t tid = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x, nth = (uint64_t)gridDim.x * blockDim.x;
  for (uint64_t i = tid; i < n; i += nth) {
    const IndelEntry t = in[i];
    IndelEntry *e = indel_find(tab, tab_mask, t.key);
    if (e) {
      if (t.fwd) atomicAdd(&e->fwd, t.fwd);
      if (t.rev) atomicAdd(&e->rev, t.rev);
    } else
      atomicAdd(stats + ST_DROPPED, 1ull);
  }
  if (add_stats && tid < INDEL_STATS && add_stats[tid]) atomicAdd(stats + tid, add_stats[tid]);
}

}  // namespace

int launch_indels(Ctx *ctx, const Slot &s, const shk_mate_alignment *records, uint64_t cap_assoc, bool skip_if_long, hipStream_t stream)
{
  const DeviceIndex &ix = ctx->idx;
  const IndelState &I = ctx->indel;
  if (!ix.gene_start || !ix.recbase || !records || !s.indels || !I.tab.p || !I.stats.p) {
    ctx->last_error = "indels mode without its state";
    return SHK_ERR_STATE;
  }
  if (s.n == 0) return SHK_OK;
  IndelParams P{};
  P.gene_off = s.d_gene_off.p;
  P.gene_ids = s.d_gene_ids.p;
  P.counters = s.d_counters;
  P.n = s.n;
  P.cap = (uint32_t)std::min<uint64_t>(std::min<uint64_t>(s.d_gene_ids.cap, cap_assoc), 0xFFFFFFFFull);   // (launch_alignments')
  P.skip_if_long = skip_if_long ? 1u : 0u;
  P.seq[0] = s.p.seq1; P.off[0] = s.p.off1; P.qual[0] = s.p.hasq ? s.p.qual1 : nullptr;
  P.seq[1] = s.p.seq2; P.off[1] = s.p.off2; P.qual[1] = s.p.hasq ? s.p.qual2 : nullptr;
  P.mq = s.p.mq;
  P.min_intron = s.indels_min_intron;
  P.records = reinterpret_cast<const uint32_t *>(records);
  P.gene_start = ix.gene_start;
  P.recbase = ix.recbase;
  P.n_genes = (uint32_t)(ctx->gene_start.size() - 1);
  P.tab = I.tab.p;
  P.tab_mask = I.tab.cap - 1;
  P.stats = I.stats.p;
  // one lane per read up to 2 048 workgroups, persistent beyond (launch_depth_accumulate's bound)
  const uint64_t want = (s.n + ID_THREADS - 1) / ID_THREADS;
  hipLaunchKernelGGL(indel_kernel, dim3((unsigned)std::min<uint64_t>(want, 2048)), dim3(ID_THREADS), 0, stream, P);
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? SHK_OK : set_hip_error(ctx, e, "indel_kernel");
}

int launch_indel_clear(Ctx *ctx)
{
  const uint64_t cap = ctx->indel.tab.cap, want = (cap + 255) / 256;
  hipLaunchKernelGGL(indel_clear_kernel, dim3((unsigned)std::min<uint64_t>(want, 2048)), dim3(256), 0, ctx->stream, ctx->indel.tab.p, cap, ctx->indel.stats.p);
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? SHK_OK : set_hip_error(ctx, e, "indel_clear_kernel");
}

int launch_indel_add(Ctx *ctx, const IndelEntry *d_in, uint64_t n, const unsigned long long *d_stats)
{
  const uint64_t want = std::max<uint64_t>((n + 255) / 256, 1);
  hipLaunchKernelGGL(indel_add_kernel, dim3((unsigned)std::min<uint64_t>(want, 2048)), dim3(256), 0, ctx->stream, ctx->indel.tab.p, ctx->indel.tab.cap - 1,
                     ctx->indel.stats.p, d_in, n, d_stats);
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? SHK_OK : set_hip_error(ctx, e, "indel_add_kernel");
}

}  // namespace shk
