// indel_host.hpp -- the parts of indels mode that need no device: the table's key, the validation of a caller's entry (shk_indels_add)
// and the text form of an entry (`shark --indels`).  Plain C++ over include/shark_hip.h, shared by libsharkhip, the command and
// indel_host_check_tool.cpp, which runs them on their own.
#pragma once
#include <stdint.h>

#include <string>

#include "../../include/shark_hip.h"

#if defined(__HIPCC__)
#define SHK_INDEL_HD __host__ __device__
#else
#define SHK_INDEL_HD
#endif

namespace shk {

// The key of a tabled event at base gx = gene_start[g] + x of the reference: a deletion carries its length in the low 16 bits, an insertion
// bit 31, its length in bits 24 .. 27 and its bases in the low 24.  Key order is (gene, x, kind, len, seq) order; all ones is no key
SHK_INDEL_HD inline unsigned long long indel_key(uint64_t gx, uint32_t kind, uint32_t len, uint32_t seq)
{
  return (unsigned long long)gx << 32 | (kind ? 0x80000000u | len << 24 | seq : len);
}

// the event's half of a key back into kind, len and seq
inline void indel_key_event(uint32_t ev, shk_indel &out)
{
  out.kind = ev >> 31;
  out.len = out.kind ? (ev >> 24) & 0x7Fu : ev & 0xFFFFu;
  out.seq = out.kind ? ev & 0xFFFFFFu : 0u;
}

// An entry of shk_indels_add as the table keys it: 0 = valid (*key set), else the rule it breaks (INDEL_ENTRY_RULES).  gs: the genes'
// starts, n_genes + 1 entries
inline int indel_entry_key(const shk_indel &t, const uint64_t *gs, uint64_t n_genes, unsigned long long *key)
{
  if (t.gene >= n_genes) return 1;
  if (t.kind > 1 || t.reserved != 0) return 2;
  if (t.kind == 0 ? (t.len < 1 || t.len > 65535 || t.seq != 0) : (t.len < 1 || t.len > SHK_INDEL_MAX_INS || (t.seq >> (2 * t.len)) != 0)) return 3;
  const uint64_t len_g = gs[t.gene + 1] - gs[t.gene];
  if (t.x >= len_g || (uint64_t)t.x + (t.kind == 0 ? t.len : 0u) > len_g) return 4;
  *key = indel_key(gs[t.gene] + t.x, t.kind, t.len, t.seq);
  return 0;
}
static const char *const INDEL_ENTRY_RULES[] = {"", "names no record (gene < n_records)", "has a kind other than 0 or 1, or reserved != 0",
                                                "has len or seq outside its kind's bounds", "lies outside its record"};

// one line of `shark --indels`: <gene> <x> <I|D> <len> <seq> <fwd> <rev>, seq as letters on the record's strand, * for a deletion
inline void indel_line(const shk_indel &e, const std::string &gene, std::string &text)
{
  text += gene;
  text += ' '; text += std::to_string(e.x);
  text += ' '; text += e.kind ? 'I' : 'D';
  text += ' '; text += std::to_string(e.len);
  text += ' ';
  if (e.kind)
    for (uint32_t t = 0; t < e.len && t < SHK_INDEL_MAX_INS; ++t) text += "ACGT"[(e.seq >> (2u * t)) & 3u];
  else text += '*';
  text += ' '; text += std::to_string(e.fwd);
  text += ' '; text += std::to_string(e.rev);
  text += '\n';
}

}  // namespace shk
