// stage_bases.hpp -- ASCII bases -> 2-bit codes + validity bits, 8 or 16 bases at a time (plain C++ that compiles for the host as
// well: kmer_device.hpp includes it for the kernels, the host-only tool shark-stage-check checks every byte value without a GPU).
//
// The result must agree with to_int (kmer_utils.hpp:29-41): A/a C/c G/g T/t are valid with codes 0..3 (= to_int-1,
// kmer_utils.hpp:68), every other byte -- including bytes >= 128, which are undefined behaviour in the reference -- is invalid.
// An invalid byte has a code too (it lands in the code streams, which the tests compare): ((t >> 1) ^ (t >> 2)) & 3 of the byte
// folded to upper case, whatever the byte is.
//
// Two forms of the same arithmetic:
//   * stage8 / stage16 / gather8: no 32-bit multiply.  Four codes are packed by one v_dot4_u32_u8 (weights 64, 16, 4, 1), "byte is
//     not zero" is a carry into bit 7, and the flags of two words share one word before ONE dot product (weights 1, 2, 4, 8) turns
//     them into eight validity bits.
//   * classify4 / pack4 / gather4: a word at a time, one v_mul_lo_u32 (a quarter-rate instruction) per pack and per gather.
//     stage8<true> / stage16<true> / gather8<true> run on these; -DSHK_STAGE_MUL=1 makes that the default, so that the two can be
//     timed by turns.  The kernels that are held at 80 VGPRs and spill a few of them as it is (the table modes' one-pair
//     instantiations, process_read) ask for this form by name: they wait on memory, not on instructions, and the other form's
//     schedule moved their spills both ways (profiles/README.md).
#pragma once
#include <stdint.h>

#ifndef SHK_STAGE_MUL
#define SHK_STAGE_MUL 0
#endif

#if defined(__HIPCC__)
#define SHK_STG_FN __host__ __device__ __forceinline__
#else
#define SHK_STG_FN inline
#endif

namespace shk {

// byte i of the result = byte sel_i of `tbl`, sel_i = byte i of `sel` (< 4): v_perm_b32 with a zero upper source
SHK_STG_FN uint32_t stg_perm(const uint32_t tbl, const uint32_t sel)
{
#if defined(__HIP_DEVICE_COMPILE__)
  return __builtin_amdgcn_perm(0u, tbl, sel);
#else
  uint32_t r = 0;
  for (int i = 0; i < 4; ++i) r |= ((tbl >> (8u * ((sel >> (8 * i)) & 3u))) & 0xFFu) << (8 * i);
  return r;
#endif
}

// sum over the four bytes of a_i * b_i: v_dot4_u32_u8
SHK_STG_FN uint32_t stg_dot4(const uint32_t a, const uint32_t b)
{
#if defined(__HIP_DEVICE_COMPILE__)
  return __builtin_amdgcn_udot4(a, b, 0u, false);
#else
  uint32_t r = 0;
  for (int i = 0; i < 4; ++i) r += ((a >> (8 * i)) & 0xFFu) * ((b >> (8 * i)) & 0xFFu);
  return r;
#endif
}

SHK_STG_FN uint32_t stg_bitrev(uint32_t x)
{
#if defined(__HIP_DEVICE_COMPILE__)
  return __builtin_bitreverse32(x);
#else
  x = ((x >> 1) & 0x55555555u) | ((x & 0x55555555u) << 1);
  x = ((x >> 2) & 0x33333333u) | ((x & 0x33333333u) << 2);
  x = ((x >> 4) & 0x0F0F0F0Fu) | ((x & 0x0F0F0F0Fu) << 4);
  x = ((x >> 8) & 0x00FF00FFu) | ((x & 0x00FF00FFu) << 8);
  return (x >> 16) | (x << 16);
#endif
}

// ---------------------------------------------------------------------------
// One word at a time, with multiplies.
//   code4 : 2-bit code in the low bits of each byte
//   inv4  : bit 0 of each byte set when that byte is NOT one of ACGTacgt
// ---------------------------------------------------------------------------
SHK_STG_FN void classify4(uint32_t w, uint32_t &code4, uint32_t &inv4)
{
  const uint32_t t = w & 0xDFDFDFDFu;                       // fold lower case onto upper case
  code4 = ((t >> 1) ^ (t >> 2)) & 0x03030303u;              // A->0 C->1 G->2 T->3
  const uint32_t expect = stg_perm(0x54474341u /* "ACGT" */, code4);
  uint32_t x = expect ^ t;                                  // zero byte <=> valid base
  x |= x >> 4;
  x |= x >> 2;
  x |= x >> 1;
  inv4 = x & 0x01010101u;
}

// 4 x 2-bit codes (one per byte, first character in the LOW byte) -> 8 bits,
// first character most significant (kmer_utils.hpp:67-69 packs MSB first).
SHK_STG_FN uint32_t pack4(uint32_t code4) { return (code4 * 0x40100401u) >> 24; }

// bit 0 of each byte -> 4 contiguous bits, byte 0 -> bit 0
SHK_STG_FN uint32_t gather4(uint32_t flags4) { return ((flags4 * 0x00204081u) >> 21) & 0xFu; }

// ---------------------------------------------------------------------------
// Without multiplies.
// ---------------------------------------------------------------------------
// code4 as classify4 gives it; bad4: BIT 7 of each byte set when that byte is not one of ACGTacgt (the other bits are whatever the
// sum left there).  x = "ACGT"[code] ^ t is zero for a base; (x & 0x7F) + 0x7F carries into bit 7 when one of the low seven bits is
// set -- at most 0xFE, so no carry leaves the byte -- and `| x` brings in bit 7 itself.
SHK_STG_FN void stg_codes4(const uint32_t w, uint32_t &code4, uint32_t &bad4)
{
  const uint32_t t = w & 0xDFDFDFDFu;
  code4 = ((t >> 1) ^ (t >> 2)) & 0x03030303u;
  const uint32_t x = stg_perm(0x54474341u, code4) ^ t;
  bad4 = ((x & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | x;
}

// bit 0 of each byte of two words -> 8 contiguous bits, byte 0 of f_lo -> bit 0, byte 0 of f_hi -> bit 4 (the words hold nothing
// but those bits): byte j of the merged word is f_lo_j + 16 f_hi_j, and the weights 1, 2, 4, 8 shift it by j
template <bool MUL = (SHK_STAGE_MUL != 0)>
SHK_STG_FN uint32_t gather8(const uint32_t f_lo, const uint32_t f_hi)
{
  if constexpr (MUL) return gather4(f_lo) | (gather4(f_hi) << 4);
  else return stg_dot4(f_lo | (f_hi << 4), 0x08040201u);
}
// the same from bit 7 of each byte, whatever the other bits hold (stg_codes4's bad4)
SHK_STG_FN uint32_t stg_gather8_bit7(const uint32_t b_lo, const uint32_t b_hi)
{
  return stg_dot4(((b_lo >> 7) & 0x01010101u) | ((b_hi >> 3) & 0x10101010u), 0x08040201u);
}

// Eight bases, `lo` the first four (first base in the LOW byte).
//   msb16 : their codes, first base in bits 15:14
//   inv8  : bit i set when base i is not one of ACGTacgt
template <bool MUL = (SHK_STAGE_MUL != 0)>
SHK_STG_FN void stage8(const uint32_t lo, const uint32_t hi, uint32_t &msb16, uint32_t &inv8)
{
  if constexpr (MUL) {
    uint32_t c_lo, c_hi, i_lo, i_hi;
    classify4(lo, c_lo, i_lo);
    classify4(hi, c_hi, i_hi);
    msb16 = (pack4(c_lo) << 8) | pack4(c_hi);
    inv8 = gather4(i_lo) | (gather4(i_hi) << 4);
  } else {
    uint32_t c_lo, c_hi, b_lo, b_hi;
    stg_codes4(lo, c_lo, b_lo);
    stg_codes4(hi, c_hi, b_hi);
    msb16 = (stg_dot4(c_lo, 0x01041040u) << 8) | stg_dot4(c_hi, 0x01041040u);
    inv8 = stg_gather8_bit7(b_lo, b_hi);
  }
}

// Sixteen bases, b0 the first four.
//   msb32 : their codes, first base in bits 31:30
//   inv16 : bit i set when base i is not one of ACGTacgt
template <bool MUL = (SHK_STAGE_MUL != 0)>
SHK_STG_FN void stage16(const uint32_t b0, const uint32_t b1, const uint32_t b2, const uint32_t b3, uint32_t &msb32, uint32_t &inv16)
{
  if constexpr (MUL) {
    uint32_t c0, c1, c2, c3, i0, i1, i2, i3;
    classify4(b0, c0, i0);
    classify4(b1, c1, i1);
    classify4(b2, c2, i2);
    classify4(b3, c3, i3);
    msb32 = (pack4(c0) << 24) | (pack4(c1) << 16) | (pack4(c2) << 8) | pack4(c3);
    inv16 = gather4(i0) | (gather4(i1) << 4) | (gather4(i2) << 8) | (gather4(i3) << 12);
  } else {
    uint32_t c0, c1, c2, c3, x0, x1, x2, x3;
    stg_codes4(b0, c0, x0);
    stg_codes4(b1, c1, x1);
    stg_codes4(b2, c2, x2);
    stg_codes4(b3, c3, x3);
    msb32 = (((((stg_dot4(c0, 0x01041040u) << 8) | stg_dot4(c1, 0x01041040u)) << 8) | stg_dot4(c2, 0x01041040u)) << 8) | stg_dot4(c3, 0x01041040u);
    inv16 = (stg_gather8_bit7(x2, x3) << 8) | stg_gather8_bit7(x0, x1);
  }
}

// the same codes with the first base in the LOW bits: reverse the 32 bits, swap the two bits of every base back (a 16-bit msb16
// lands in the high half)
SHK_STG_FN uint32_t stg_lsb_first(const uint32_t msb)
{
  const uint32_t r = stg_bitrev(msb);
  return ((r >> 1) & 0x55555555u) | ((r & 0x55555555u) << 1);
}

}  // namespace shk
