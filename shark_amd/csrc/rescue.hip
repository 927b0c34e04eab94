// rescue.hip -- rescue mode's kernels (gfx950): a mate without a block is compared base by base with every place beside its placed partner
// at which the pair would be proper, and gets an alignment record of one ungapped block where one place is good enough and clearly the
// best (include/shark_hip.h, "rescue").  The first kernel here that compares sequences densely instead of looking k-mers up.
// It runs directly behind the align_kernel launch that stores the records and changes only the rescued mates' records.
//
// Nearly every association needs no rescue, so no wave is spent per read.  Two launches:
//
// rescue_scan_kernel  pair_kernel's shape: one LANE per read, gene_off coalesced, a loop over the read's associations that the wave
//                     walks together.  It reads the first 16-byte word of either mate's record, writes the state 0 record of an
//                     association that is not attempted and appends (read, association) of an attempted one to a queue: one ballot
//                     and one atomic per wave and trip, the count stays on the device.
// rescue_kernel       a fixed grid of workgroups of four waves; a wave takes queue entries in a stride loop up to the device's count.
//                     Per entry the anchor's ends, I_A and the window are wave-uniform scalar work.  The wave stages into its own LDS
//                     slice the target's codes in the record's orientation (complement, reversal and the -q mask applied once) and the
//                     window's record bytes as aligned dwords, loaded coalesced.  Lane t of pass p prices x = lo + 64 p + t: four
//                     bases per step, four steps per trip -- the record's dword at the lane's byte offset from two aligned LDS dwords
//                     by a byte-align (the second is the next step's first: one LDS load per step), xor against the target's dword
//                     (a broadcast load), a carry fold that leaves one bit per non-zero byte, a popcount.  A target byte that is no
//                     base is 0x80 and a record byte that is none is 4, so the xor of a "neither" is never 0.  A lane leaves the loop
//                     once its cost exceeds cap.
//                     One wave minimum over cost << 12 | tie key per pass and a second one without the winner; best and second best are
//                     carried across passes as scalars.  The winner is counted by step 4 from the staged bytes, its record is stored
//                     by sixteen lanes as one 64-byte line, the rescue record by one 16-byte store.
//
// LDS: 1 284 dwords per wave, 20 KiB per workgroup: seven workgroups per CU.  No inline assembly, no run-time index into registers, no
// scratch memory.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "kmer_device.hpp"
#include "shark_internal.hpp"

namespace shk {

static_assert(sizeof(shk_rescue) == 16, "a rescue record is one 16-byte store");
static_assert(sizeof(shk_mate_alignment) == 64 && SHK_MAX_SEGMENTS == 4, "the record layout the loads below take apart");
static_assert(SHK_RESCUE_MAX_LEN % 4 == 0, "the target's slice is whole dwords");

namespace {

constexpr uint32_t RS_SCAN_THREADS = 256;
constexpr uint32_t RS_SCAN_MAX_BLOCKS = 512;     // pair_kernel's: a larger batch takes the stride loop's next trips
constexpr uint32_t RS_WAVES = 4, RS_THREADS = RS_WAVES * 64;
constexpr uint32_t RS_MAX_BLOCKS = 512;          // 2 048 waves: two workgroups per CU; more queue entries take the stride loop's next trips
constexpr uint32_t RS_MAX_FRAG = 4096;           // shk_rescue_enable's bound, and so n_cand's
constexpr uint32_t RS_TGT_WORDS = SHK_RESCUE_MAX_LEN / 4;
// the window's dwords: the lane of byte offset o = shift + 64 p + t (shift <= 3, 64 p + t < n_cand <= 4 096) reads dwords (o >> 2) + d for
// d = 0 .. ceil(L_T / 4): at most 1 024 + 128
constexpr uint32_t RS_WIN_WORDS = (RS_MAX_FRAG + 3) / 4 + 1 + RS_TGT_WORDS;
constexpr uint32_t RS_WAVE_WORDS = RS_TGT_WORDS + RS_WIN_WORDS + 3;   // 1 284: a multiple of four, so every wave's slice is 16-byte aligned
static_assert(RS_WAVE_WORDS % 4 == 0 && RS_WAVE_WORDS * 4 * RS_WAVES <= 80 * 1024, "at least two workgroups per CU");
constexpr uint32_t RS_NO_BASE = 0x80u;           // a target byte that is no base: its xor against a record byte 0 .. 4 is never 0
constexpr uint32_t RS_TIE_BITS = 12;             // 64 p + t < 4 096

struct RescueParams {
  const uint32_t *gene_off;
  const uint16_t *gene_ids;
  const uint32_t *counters;
  uint64_t n;                      // reads
  const uint8_t *seq[2];
  const uint64_t *off[2];          // off[1] == nullptr: a single-end batch, nothing is attempted
  const uint8_t *qual[2];          // nullptr: no masking
  int32_t mq;
  const uint64_t *gene_start;
  const uint8_t *recbase;
  uint64_t recbase_bytes;          // whole dwords: an aligned dword below it may be loaded
  uint32_t n_genes;
  uint32_t skip_if_long;
  uint32_t cap;                    // associations `align` and `out` hold
  uint4 *align;                    // [(j * 2 + mate) * 4 + v]: shk_mate_alignment as four 16-byte words
  uint4 *out;                      // [j]: shk_rescue
  uint32_t *queue_count;           // cleared in front of the scan
  uint2 *queue;                    // (read, association)
  uint32_t cap_queue;
  uint32_t min_intron, max_frag, max_cost, min_gap;
  uint32_t n_lanes;                // of the scan's launch
  uint32_t n_waves;                // of rescue_kernel's launch
};

__device__ __forceinline__ uint32_t clamp_len(uint64_t len) { return len > 0x7FFFFFFFull ? 0x7FFFFFFFu : (uint32_t)len; }   // (align_kernel's L)

__device__ __forceinline__ uint32_t wave_min_u32(uint32_t v)
{
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) {
    const uint32_t t = (uint32_t)__shfl_xor((int)v, o, 64);
    v = t < v ? t : v;
  }
  return v;
}

__device__ __forceinline__ uint32_t rfl(uint32_t v) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)v); }   // (a wave-uniform value into a scalar register)

// what this wave has written to its LDS slice is what its lanes read from here on
__device__ __forceinline__ void wave_lds_sync()
{
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

__global__ __launch_bounds__(RS_SCAN_THREADS) void rescue_scan_kernel(const RescueParams P)
{
  // align_kernel's three: the batch will be assembled again and comes through here again; or it will be refused in wait
  if (P.counters[CTR_OVERFLOW] || (P.skip_if_long && P.counters[CTR_LONG]) || P.counters[CTR_VOUCH_BAD]) return;
  const uint32_t lane = threadIdx.x & 63u;
  // (every wave makes the same number of trips: the ballots below see whole waves)
  const uint64_t trips = (P.n + P.n_lanes - 1) / P.n_lanes;
  for (uint64_t trip = 0; trip < trips; ++trip) {
    const uint64_t i = trip * P.n_lanes + (uint64_t)blockIdx.x * RS_SCAN_THREADS + threadIdx.x;
    uint32_t o0 = 0, o1 = 0, L0 = 0, L1 = 0;
    if (i < P.n) {
      o0 = P.gene_off[i]; o1 = P.gene_off[i + 1];
      if (o1 <= o0 || o1 > P.cap) o1 = o0;        // (align_kernel's guard for a read whose associations the buffers do not hold)
      else if (P.off[1]) {
        L0 = clamp_len(P.off[0][i + 1] - P.off[0][i]);
        L1 = clamp_len(P.off[1][i + 1] - P.off[1][i]);
      }
    }
    // the wave walks its reads' associations together (almost always one trip): the ballot sees every lane
    for (uint32_t j = o0; __any(j < o1); ++j) {
      bool attempted = false;
      if (j < o1) {
        const uint32_t nb0 = P.align[(uint64_t)j * 8u].x, nb1 = P.align[(uint64_t)j * 8u + 4u].x;
        const uint32_t L_t = nb0 ? L1 : L0;       // (read where exactly one mate has a block: the other's length)
        attempted = (nb0 != 0u) != (nb1 != 0u) && L_t >= SHK_RESCUE_MIN_LEN && L_t <= SHK_RESCUE_MAX_LEN;
        if (!attempted) P.out[j] = make_uint4(0u, 0u, 0u, 0u);
      }
      const uint64_t mask = __ballot(attempted);
      if (mask) {
        const uint32_t leader = (uint32_t)__ffsll((unsigned long long)mask) - 1u;
        uint32_t base = 0;
        if (lane == leader) base = atomicAdd(P.queue_count, (uint32_t)__popcll(mask));
        base = (uint32_t)__shfl((int)base, (int)leader, 64);
        const uint32_t at = base + (uint32_t)__popcll(mask & ((1ull << lane) - 1ull));
        if (attempted && at < P.cap_queue) P.queue[at] = make_uint2((uint32_t)i, j);
      }
    }
  }
}

// the anchor's ends from its record (pairs.hip's mate_ends: the last block by compares against n_blocks, the three gaps at constant places)
struct AnchorEnds {
  int64_t s, e, cl, cr, introns;
  uint32_t strand;
};

// v0 = {n_blocks, strand, matches, mismatches}, v1 = {x0, q0, len0, x1}, v2 = {q1, len1, x2, q2}, v3 = {len2, x3, q3, len3}
__device__ __forceinline__ AnchorEnds anchor_ends(const uint4 v0, const uint4 v1, const uint4 v2, const uint4 v3, uint32_t L, uint32_t min_intron)
{
  AnchorEnds A;
  const uint32_t nb = v0.x;
  A.strand = v0.y ? 1u : 0u;
  const uint32_t lx = nb <= 1u ? v1.x : (nb == 2u ? v1.w : (nb == 3u ? v2.z : v3.y));
  const uint32_t lq = nb <= 1u ? v1.y : (nb == 2u ? v2.x : (nb == 3u ? v2.w : v3.z));
  const uint32_t ll = nb <= 1u ? v1.z : (nb == 2u ? v2.y : (nb == 3u ? v3.x : v3.w));
  A.s = (int32_t)v1.x;
  A.e = (int32_t)(lx + ll);
  A.cl = v1.y;
  A.cr = (int64_t)L - (int64_t)(lq + ll);
  const int32_t lo0 = (int32_t)(v1.x + v1.z), hi0 = (int32_t)v1.w;
  const int32_t lo1 = (int32_t)(v1.w + v2.y), hi1 = (int32_t)v2.z;
  const int32_t lo2 = (int32_t)(v2.z + v3.x), hi2 = (int32_t)v3.y;
  A.introns = 0;
  if (nb >= 2u && hi0 > lo0 && (uint32_t)(hi0 - lo0) >= min_intron) A.introns += hi0 - lo0;
  if (nb >= 3u && hi1 > lo1 && (uint32_t)(hi1 - lo1) >= min_intron) A.introns += hi1 - lo1;
  if (nb >= 4u && hi2 > lo2 && (uint32_t)(hi2 - lo2) >= min_intron) A.introns += hi2 - lo2;
  return A;
}

// one bit (the top one) per non-zero byte of v
__device__ __forceinline__ uint32_t nonzero_bytes(uint32_t v) { return (((v & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | v) & 0x80808080u; }

__global__ __launch_bounds__(RS_THREADS) void rescue_kernel(const RescueParams P)
{
  if (P.counters[CTR_OVERFLOW] || (P.skip_if_long && P.counters[CTR_LONG]) || P.counters[CTR_VOUCH_BAD] || !P.off[1]) return;
  __shared__ __attribute__((aligned(16))) uint32_t lds[RS_WAVES * RS_WAVE_WORDS];
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t wave = rfl(threadIdx.x >> 6);
  uint32_t *const tgt = lds + wave * RS_WAVE_WORDS;          // the target's codes, four per dword, read coordinate 4 w + b in byte b
  uint32_t *const win = tgt + RS_TGT_WORDS;                  // the record's bytes from the aligned address at or below the window's first
  const uint8_t *const win8 = reinterpret_cast<const uint8_t *>(win);
  const uint8_t *const tgt8 = reinterpret_cast<const uint8_t *>(tgt);
  const uint32_t n_queued = std::min(rfl(*P.queue_count), P.cap_queue);
  const uint32_t cap = P.max_cost + P.min_gap, sat = cap + 1u;
  for (uint32_t entry = blockIdx.x * RS_WAVES + wave; entry < n_queued; entry += P.n_waves) {
    const uint2 qe = P.queue[entry];
    const uint64_t i = rfl(qe.x);
    const uint32_t j = rfl(qe.y);
    if (i >= P.n || j >= P.cap) continue;
    uint4 *const rec = P.align + (uint64_t)j * 8u;
    const uint32_t a_is_1 = rfl(rec[0].x) ? 0u : 1u;   // the anchor's mate index; the target is the other
    const uint32_t t_is = 1u - a_is_1;
    const uint4 *const a = rec + a_is_1 * 4u;
    // (selects, not a run-time index into the kernel's arguments)
    const uint64_t *const off_a = a_is_1 ? P.off[1] : P.off[0], *const off_t = a_is_1 ? P.off[0] : P.off[1];
    const uint64_t t_off = off_t[i];
    const uint32_t L_a = clamp_len(off_a[i + 1] - off_a[i]);
    const int32_t L_t = (int32_t)rfl(clamp_len(off_t[i + 1] - t_off));
    AnchorEnds A = anchor_ends(a[0], a[1], a[2], a[3], L_a, P.min_intron);
    A.strand = rfl(A.strand);
    const uint32_t g = P.gene_ids[j];
    // the window (the header's, in signed 64-bit arithmetic)
    int64_t lo = 0, hi = -1;
    uint64_t start = 0;
    if (g < P.n_genes && L_t >= (int32_t)SHK_RESCUE_MIN_LEN && L_t <= (int32_t)SHK_RESCUE_MAX_LEN) {
      start = P.gene_start[g];
      const int64_t len_g = (int64_t)(P.gene_start[g + 1] - start);
      if (!A.strand) {
        lo = std::max<int64_t>(std::max<int64_t>(A.s, A.e - L_t), 0);
        hi = std::min<int64_t>(A.s - A.cl + A.introns + (int64_t)P.max_frag - L_t, len_g - L_t);
      } else {
        lo = std::max<int64_t>(A.e + A.cr - A.introns - (int64_t)P.max_frag, 0);
        hi = std::min<int64_t>(std::min<int64_t>(A.s, A.e - L_t), len_g - L_t);
      }
    }
    // (n_cand <= max_frag by the header's argument; the bound keeps a lane inside the slice whatever the records hold)
    const uint32_t n_cand = rfl(hi >= lo ? (uint32_t)std::min<int64_t>(hi - lo + 1, RS_MAX_FRAG) : 0u);
    uint32_t best = 0xFFFFFFFFu, second = sat;     // the best candidate's key, the smallest cost among the others
    uint32_t shift = 0;
    if (n_cand) {
      const uint32_t t_strand = 1u - A.strand;
      // the target in the record's orientation, behind the -q mask (align_kernel's read_base)
      const uint8_t *const seq = (a_is_1 ? P.seq[0] : P.seq[1]) + t_off;
      const uint8_t *const qual_t = a_is_1 ? P.qual[0] : P.qual[1];
      const uint8_t *const qual = qual_t ? qual_t + t_off : nullptr;
      const uint32_t n_tw = ((uint32_t)L_t + 3u) >> 2;
      for (uint32_t w = lane; w < n_tw; w += 64u) {
        uint32_t v = 0;
#pragma unroll
        for (uint32_t b = 0; b < 4u; ++b) {
          const uint32_t q = 4u * w + b;
          uint32_t code = 0;
          if (q < (uint32_t)L_t) {
            const uint32_t idx = t_strand ? (uint32_t)L_t - 1u - q : q;
            uint32_t ch = seq[idx];
            if (qual && (int32_t)(int8_t)qual[idx] < P.mq) ch = (ch - 64u) & 0xFFu;
            const uint32_t c = base_code(ch);
            code = c < 4u ? (t_strand ? 3u - c : c) : RS_NO_BASE;
          }
          v |= code << (8u * b);
        }
        tgt[w] = v;
      }
      // the window's n_cand + L_T - 1 record bytes as aligned dwords
      const uint64_t first = start + (uint64_t)lo;
      shift = rfl((uint32_t)(first & 3u));
      const uint64_t base = first - shift;
      const uint32_t n_ww = (shift + n_cand + (uint32_t)L_t - 1u + 3u) >> 2;   // (<= RS_WIN_WORDS - 1)
      for (uint32_t w = lane; w < n_ww; w += 64u) {
        const uint64_t at = base + 4ull * w;
        win[w] = at + 4u <= P.recbase_bytes ? *reinterpret_cast<const uint32_t *>(P.recbase + at) : 0x04040404u;
      }
      wave_lds_sync();
      const uint32_t n_full = (uint32_t)L_t >> 2;                              // whole dwords of the target
      const uint32_t tail_mask = (1u << (8u * ((uint32_t)L_t & 3u))) - 1u;       // the bytes of the last, partial one (0: none)
      for (uint32_t o0 = 0; o0 < n_cand; o0 += 64u) {
        const uint32_t o = o0 + lane;
        uint32_t key = 0xFFFFFFFFu;
        if (o < n_cand) {
          const uint32_t byte = shift + o, rot = byte & 3u;
          const uint32_t *const w = win + (byte >> 2);
          uint32_t cost = 0, d = 0;
          uint32_t cur = w[0];
          // sixteen bases per trip while they last -- the four steps' loads are in flight together, the bound is looked at once --, then four
          for (; d + 4u <= n_full && cost <= cap; d += 4u) {
            const uint4 t4 = *reinterpret_cast<const uint4 *>(tgt + d);
            const uint32_t n0 = w[d + 1u], n1 = w[d + 2u], n2 = w[d + 3u], n3 = w[d + 4u];
            cost += (uint32_t)__popc(nonzero_bytes(__builtin_amdgcn_alignbyte(n0, cur, rot) ^ t4.x)) +
                    (uint32_t)__popc(nonzero_bytes(__builtin_amdgcn_alignbyte(n1, n0, rot) ^ t4.y)) +
                    (uint32_t)__popc(nonzero_bytes(__builtin_amdgcn_alignbyte(n2, n1, rot) ^ t4.z)) +
                    (uint32_t)__popc(nonzero_bytes(__builtin_amdgcn_alignbyte(n3, n2, rot) ^ t4.w));
            cur = n3;
          }
          for (; d < n_full && cost <= cap; ++d) {
            const uint32_t next = w[d + 1u];
            cost += (uint32_t)__popc(nonzero_bytes(__builtin_amdgcn_alignbyte(next, cur, rot) ^ tgt[d]));
            cur = next;
          }
          if (d == n_full && tail_mask && cost <= cap) {
            const uint32_t next = w[d + 1u];
            cost += (uint32_t)__popc(nonzero_bytes((__builtin_amdgcn_alignbyte(next, cur, rot) ^ tgt[d]) & tail_mask));
          }
          cost = cost < sat ? cost : sat;
          // ties to the smallest frag: the smallest x beside an anchor on strand 0, the largest beside one on strand 1
          key = (cost << RS_TIE_BITS) | (A.strand ? (RS_MAX_FRAG - 1u) - o : o);
        }
        const uint32_t m1 = rfl(wave_min_u32(key));   // (lane 0 of a pass is a candidate: m1 is one's key)
        const uint32_t m2 = rfl(wave_min_u32(key == m1 ? 0xFFFFFFFFu : key));   // (keys are distinct: only the winner leaves)
        const uint32_t c1 = m1 >> RS_TIE_BITS, c2 = std::min(m2 >> RS_TIE_BITS, sat);
        if (m1 < best) {
          second = std::min(std::min(second, std::min(best >> RS_TIE_BITS, sat)), c2);
          best = m1;
        } else {
          second = std::min(second, c1);
        }
      }
    }
    const uint32_t cost = n_cand ? best >> RS_TIE_BITS : sat;
    uint32_t state = 1u;
    if (n_cand) state = cost > P.max_cost ? 2u : (second - cost < P.min_gap ? 3u : 4u + t_is);
    if (state >= 4u) {
      const uint32_t tie = best & ((1u << RS_TIE_BITS) - 1u);
      const uint32_t o = A.strand ? (RS_MAX_FRAG - 1u) - tie : tie;
      // step 4 over the one block, from the staged bytes
      uint32_t matches = 0, mismatches = 0;
      for (int32_t q0 = 0; q0 < L_t; q0 += 64) {
        const int32_t q = q0 + (int32_t)lane;
        bool is_m = false, is_x = false;
        if (q < L_t) {
          const uint32_t b = tgt8[q], r = win8[shift + o + (uint32_t)q];
          is_m = b == r;                              // (b is 0 .. 3 or 0x80, r is 0 .. 4)
          is_x = b < 4u && r < 4u && b != r;
        }
        matches += (uint32_t)__popcll(__ballot(is_m));
        mismatches += (uint32_t)__popcll(__ballot(is_x));
      }
      const uint32_t x = (uint32_t)(lo + (int64_t)o);
      const uint32_t word = lane == 0u ? 1u : (lane == 1u ? 1u - A.strand : (lane == 2u ? matches : (lane == 3u ? mismatches : (lane == 4u ? x : (lane == 6u ? (uint32_t)L_t : 0u)))));
      if (lane < 16u) reinterpret_cast<uint32_t *>(rec + t_is * 4u)[lane] = word;
    }
    if (lane == 0u) P.out[j] = make_uint4(state, cost, n_cand ? second : sat, n_cand);
    wave_lds_sync();                                  // (the next entry's staging overwrites what this one's lanes have read)
  }
}

}  // namespace

int launch_rescue(Ctx *ctx, const Slot &s, uint64_t cap_assoc, bool skip_if_long, hipStream_t stream)
{
  const DeviceIndex &ix = ctx->idx;
  if (!s.rescue || !s.align || !s.rec_align.d.p || !s.rec_rescue.d.p || !s.d_rescue_queue.p || s.rescue > RS_MAX_FRAG || !ix.gene_start || !ix.recbase) {
    ctx->last_error = "rescue mode without its state";
    return SHK_ERR_STATE;
  }
  if (s.n == 0) return SHK_OK;
  RescueParams P{};
  P.gene_off = s.d_gene_off.p;
  P.gene_ids = s.d_gene_ids.p;
  P.counters = s.d_counters;
  P.n = s.n;
  P.seq[0] = s.p.seq1; P.off[0] = s.p.off1; P.qual[0] = s.p.hasq ? s.p.qual1 : nullptr;
  P.seq[1] = s.p.seq2; P.off[1] = s.p.seq2 ? s.p.off2 : nullptr; P.qual[1] = s.p.hasq ? s.p.qual2 : nullptr;
  P.mq = s.p.mq;
  P.gene_start = ix.gene_start;
  P.recbase = ix.recbase;
  P.recbase_bytes = ix.recbase_bytes & ~3ull;
  P.n_genes = (uint32_t)(ctx->gene_start.size() - 1);
  P.skip_if_long = skip_if_long ? 1u : 0u;
  // (launch_alignments' bound on the associations its records hold, and this mode's own array)
  P.cap = (uint32_t)std::min<uint64_t>(std::min<uint64_t>(std::min<uint64_t>(s.d_gene_ids.cap, cap_assoc), std::min<uint64_t>(s.rec_align.d.cap / 2, s.rec_rescue.d.cap)), 0xFFFFFFFFull);
  P.align = reinterpret_cast<uint4 *>(s.rec_align.d.p);
  P.out = reinterpret_cast<uint4 *>(s.rec_rescue.d.p);
  // the queue's first 16 bytes hold the count
  P.queue_count = reinterpret_cast<uint32_t *>(s.d_rescue_queue.p);
  P.queue = s.d_rescue_queue.p + 2;
  P.cap_queue = (uint32_t)std::min<uint64_t>(s.d_rescue_queue.cap - 2, 0xFFFFFFFFull);
  P.min_intron = s.rescue_min_intron;
  P.max_frag = s.rescue;
  P.max_cost = s.rescue_max_cost;
  P.min_gap = s.rescue_min_gap;
  const unsigned scan_blocks = (unsigned)std::min<uint64_t>((s.n + RS_SCAN_THREADS - 1) / RS_SCAN_THREADS, RS_SCAN_MAX_BLOCKS);
  P.n_lanes = scan_blocks * RS_SCAN_THREADS;
  // (the attempted associations are counted on the device: the grid is sized by the reads, a wave that finds no entry returns at once)
  const unsigned blocks = (unsigned)std::min<uint64_t>((s.n + RS_WAVES - 1) / RS_WAVES, RS_MAX_BLOCKS);
  P.n_waves = blocks * RS_WAVES;
  hipError_t e = hipMemsetAsync(P.queue_count, 0, sizeof(uint32_t), stream);
  if (e != hipSuccess) return set_hip_error(ctx, e, "rescue queue");
  hipLaunchKernelGGL(rescue_scan_kernel, dim3(scan_blocks), dim3(RS_SCAN_THREADS), 0, stream, P);
  if ((e = hipGetLastError()) != hipSuccess) return set_hip_error(ctx, e, "rescue_scan_kernel");
  hipLaunchKernelGGL(rescue_kernel, dim3(blocks), dim3(RS_THREADS), 0, stream, P);
  e = hipGetLastError();
  return e == hipSuccess ? SHK_OK : set_hip_error(ctx, e, "rescue_kernel");
}

}  // namespace shk
