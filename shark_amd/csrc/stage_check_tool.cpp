// shark-stage-check -- stage_bases.hpp's stage8 / stage16 / gather8 on the CPU, against two references: the word-at-a-time
// classify4 / pack4 / gather4 with multiplies as the kernels ran them before (carried here in full, so that a change to the header
// does not change the reference), and a definition byte by byte.  Every byte value at every position of a chunk, in random
// contexts, at every shift of the alignbyte front; both stream words and the validity bits are compared.
//
//   shark-stage-check [contexts per (value, position, shift), default 64] [seed]
//
// prints one JSON line; exit status 1 when anything differs.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "stage_bases.hpp"

namespace ref {
// ---- the word-at-a-time form, as it stood ----
static uint32_t perm(const uint32_t tbl, const uint32_t sel)
{
  uint32_t r = 0;
  for (int i = 0; i < 4; ++i) r |= ((tbl >> (8u * ((sel >> (8 * i)) & 7u))) & 0xFFu) << (8 * i);   // (selectors are 0..3 here)
  return r;
}
static void classify4(uint32_t w, uint32_t &code4, uint32_t &inv4)
{
  const uint32_t t = w & 0xDFDFDFDFu;
  code4 = ((t >> 1) ^ (t >> 2)) & 0x03030303u;
  const uint32_t expect = perm(0x54474341u, code4);
  uint32_t x = expect ^ t;
  x |= x >> 4;
  x |= x >> 2;
  x |= x >> 1;
  inv4 = x & 0x01010101u;
}
static uint32_t pack4(uint32_t code4) { return (code4 * 0x40100401u) >> 24; }
static uint32_t gather4(uint32_t flags4) { return ((flags4 * 0x00204081u) >> 21) & 0xFu; }
static uint32_t lsb_first(uint32_t msb)
{
  uint32_t r = 0;
  for (int i = 0; i < 32; ++i) r |= ((msb >> i) & 1u) << (31 - i);
  return ((r >> 1) & 0x55555555u) | ((r & 0x55555555u) << 1);
}
// ---- byte by byte ----
// valid: one of ACGTacgt, code = to_int - 1 (kmer_utils.hpp:29-41, :68); any other byte is invalid and carries the code the kernels have
// always given it: ((t >> 1) ^ (t >> 2)) & 3 of the byte with bit 5 cleared
static bool byte_valid(const uint8_t c) { return c != 0 && strchr("ACGTacgt", c) != nullptr; }
static uint32_t byte_code(const uint8_t c)
{
  if (byte_valid(c)) return (uint32_t)(strchr("ACGT", c & 0xDF) - "ACGT");
  const uint32_t t = c & 0xDFu;
  return ((t >> 1) ^ (t >> 2)) & 3u;
}
// kmer_device.hpp's base_code: 0..3, or 4 = invalid
static uint32_t base_code(uint32_t c)
{
  const uint32_t t = c & 0xDFu;
  const uint32_t code = ((t >> 1) ^ (t >> 2)) & 3u;
  const uint32_t expect = (0x54474341u >> (8 * code)) & 0xFFu;
  return expect == t ? code : 4u;
}
}  // namespace ref

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint32_t rnd()
{
  rng_state ^= rng_state << 13;
  rng_state ^= rng_state >> 7;
  rng_state ^= rng_state << 17;
  return (uint32_t)(rng_state >> 16);
}
// a context byte: mostly bases (both cases), some N, some anything
static uint8_t context_byte()
{
  const uint32_t r = rnd();
  const uint32_t kind = r & 15u;
  if (kind < 9) return (uint8_t)"ACGT"[(r >> 4) & 3u];
  if (kind < 12) return (uint8_t)"acgt"[(r >> 4) & 3u];
  if (kind < 13) return (uint8_t)'N';
  return (uint8_t)(r >> 8);
}

static uint32_t alignbyte(const uint32_t hi, const uint32_t lo, const uint32_t sh) { return (uint32_t)(((((uint64_t)hi) << 32) | lo) >> (8u * sh)); }

struct Tally { uint64_t chunks16 = 0, chunks8 = 0, diff_mul = 0, diff_bytes = 0, diff_base_code = 0, diff_gather8 = 0, diff_forms = 0; };

// the chunk of N bases (16 or 8) that starts `sh` bytes into buf (N + 4 bytes, as the kernels' dwords hold them)
template <int N>
static void check_chunk(const uint8_t *buf, const uint32_t sh, Tally &t)
{
  uint32_t d[5] = {0u, 0u, 0u, 0u, 0u}, b[4] = {0u, 0u, 0u, 0u};
  memcpy(d, buf, N + 4);
  for (int i = 0; i < N / 4; ++i) b[i] = alignbyte(d[i + 1], d[i], sh);
  uint32_t msb, inv;
  if (N == 16) shk::stage16(b[0], b[1], b[2], b[3], msb, inv);
  else shk::stage8(b[0], b[1], msb, inv);
  const uint32_t lsb = shk::stg_lsb_first(msb);
  // (the header's two forms: the one the kernels get by default, above, and the one they can ask for by name)
  uint32_t msb_f[2], inv_f[2];
  if (N == 16) { shk::stage16<false>(b[0], b[1], b[2], b[3], msb_f[0], inv_f[0]); shk::stage16<true>(b[0], b[1], b[2], b[3], msb_f[1], inv_f[1]); }
  else { shk::stage8<false>(b[0], b[1], msb_f[0], inv_f[0]); shk::stage8<true>(b[0], b[1], msb_f[1], inv_f[1]); }
  if (msb_f[0] != msb || msb_f[1] != msb || inv_f[0] != inv || inv_f[1] != inv) ++t.diff_forms;
  // the word-at-a-time form
  uint32_t msb_m = 0, inv_m = 0;
  for (int i = 0; i < N / 4; ++i) {
    uint32_t c4, i4;
    ref::classify4(b[i], c4, i4);
    msb_m |= ref::pack4(c4) << (8 * (N / 4 - 1 - i));
    inv_m |= ref::gather4(i4) << (4 * i);
  }
  if (msb != msb_m || inv != inv_m || lsb != ref::lsb_first(msb_m)) ++t.diff_mul;
  // byte by byte
  uint32_t msb_b = 0, lsb_b = 0, inv_b = 0;
  for (int i = 0; i < N; ++i) {
    const uint8_t c = buf[sh + i];
    const uint32_t code = ref::byte_code(c);
    msb_b |= code << (2 * (N - 1 - i));
    lsb_b |= code << (2 * i);
    inv_b |= (ref::byte_valid(c) ? 0u : 1u) << i;
  }
  if (N == 8) lsb_b <<= 16;   // (the reversal of a 16-bit word lands in the high half)
  if (msb != msb_b || inv != inv_b || lsb != lsb_b) ++t.diff_bytes;
  (N == 16 ? t.chunks16 : t.chunks8) += 1;
}

template <int N>
static void sweep(const uint32_t contexts, Tally &t)
{
  uint8_t buf[N + 4];
  for (uint32_t sh = 0; sh < 4; ++sh) {
    // every value at every position, in random contexts
    for (uint32_t v = 0; v < 256; ++v)
      for (uint32_t p = 0; p < (uint32_t)N; ++p)
        for (uint32_t c = 0; c < contexts; ++c) {
          for (auto &x : buf) x = context_byte();
          buf[sh + p] = (uint8_t)v;
          check_chunk<N>(buf, sh, t);
        }
    // every value everywhere (all-invalid chunks but for the eight bases' own), all-valid chunks in both cases, mixed case
    for (uint32_t v = 0; v < 256; ++v) {
      memset(buf, (int)v, sizeof(buf));
      check_chunk<N>(buf, sh, t);
    }
    for (uint32_t c = 0; c < 4096; ++c) {
      for (auto &x : buf) x = (uint8_t)"ACGT"[rnd() & 3u];
      check_chunk<N>(buf, sh, t);
      for (auto &x : buf) x = (uint8_t)"acgt"[rnd() & 3u];
      check_chunk<N>(buf, sh, t);
      for (auto &x : buf) x = (uint8_t)"ACGTacgt"[rnd() & 7u];
      check_chunk<N>(buf, sh, t);
      for (auto &x : buf) x = (uint8_t)rnd();
      check_chunk<N>(buf, sh, t);
    }
  }
}

int main(int argc, char **argv)
{
  const uint32_t contexts = argc > 1 ? (uint32_t)strtoul(argv[1], nullptr, 10) : 64u;
  if (argc > 2) rng_state ^= strtoull(argv[2], nullptr, 10) * 0xD1B54A32D192ED03ull;
  Tally t;
  sweep<16>(contexts, t);
  sweep<8>(contexts, t);
  // the byte-by-byte definition and base_code (the index build's classification) agree on every byte
  for (uint32_t v = 0; v < 256; ++v) {
    const uint32_t bc = ref::base_code(v);
    if ((bc != 4u) != ref::byte_valid((uint8_t)v) || (bc != 4u && bc != ref::byte_code((uint8_t)v))) ++t.diff_base_code;
  }
  // gather8 over every pattern of the eight flags
  for (uint32_t m = 0; m < 256; ++m) {
    uint32_t f[2] = {0u, 0u};
    for (uint32_t i = 0; i < 8; ++i) f[i >> 2] |= ((m >> i) & 1u) << (8u * (i & 3u));
    if (shk::gather8(f[0], f[1]) != m || shk::gather8<false>(f[0], f[1]) != m || shk::gather8<true>(f[0], f[1]) != m || (ref::gather4(f[0]) | (ref::gather4(f[1]) << 4)) != m) ++t.diff_gather8;
  }
  printf("{\"stage_mul\": %d, \"contexts\": %u, \"chunks16\": %llu, \"chunks8\": %llu, \"diff_mul\": %llu, \"diff_bytes\": %llu, \"diff_base_code\": %llu, "
         "\"diff_gather8\": %llu, \"diff_forms\": %llu}\n",
         (int)SHK_STAGE_MUL, contexts, (unsigned long long)t.chunks16, (unsigned long long)t.chunks8, (unsigned long long)t.diff_mul,
         (unsigned long long)t.diff_bytes, (unsigned long long)t.diff_base_code, (unsigned long long)t.diff_gather8, (unsigned long long)t.diff_forms);
  return (t.diff_mul | t.diff_bytes | t.diff_base_code | t.diff_gather8 | t.diff_forms) ? 1 : 0;
}
