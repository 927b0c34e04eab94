// indel_host_check_tool.cpp -- the host-only parts of indels mode (indel_host.hpp) run on their own: the entry validation of
// shk_indels_add and the line writer of `shark --indels` over every boundary of their rules.  No device, no library: built and run under
// -fsanitize=address,undefined by tools/indel_host_check.sh.  Exit status 0 and "indel host check ok" when every expectation holds.
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "indel_host.hpp"

static int failures = 0;
#define EXPECT(cond)                                                       \
  do {                                                                     \
    if (!(cond)) { std::fprintf(stderr, "line %d: %s\n", __LINE__, #cond); ++failures; } \
  } while (0)

int main()
{
  using namespace shk;
  // three genes of 100, 0 and 50 bases, the arrays sized exactly: a read past either end is the sanitizer's to find
  std::vector<uint64_t> gs{0, 100, 100, 150};
  const uint64_t n_genes = gs.size() - 1;
  unsigned long long key = 0;
  auto rule = [&](uint32_t gene, uint32_t x, uint32_t kind, uint32_t len, uint32_t seq, uint32_t reserved = 0) {
    const shk_indel e{gene, x, kind, len, seq, 1, 2, reserved};
    return indel_entry_key(e, gs.data(), n_genes, &key);
  };
  EXPECT(rule(0, 0, 0, 1, 0) == 0 && key == indel_key(0, 0, 1, 0));
  EXPECT(rule(0, 99, 0, 1, 0) == 0);
  EXPECT(rule(0, 35, 0, 65, 0) == 0);
  EXPECT(rule(0, 36, 0, 65, 0) == 4);
  EXPECT(rule(0, 100, 1, 1, 0) == 4);
  EXPECT(rule(0, 99, 1, 12, 0xFFFFFFu) == 0 && key == (99ull << 32 | 0x80000000u | 12u << 24 | 0xFFFFFFu));
  EXPECT(rule(1, 0, 1, 1, 0) == 4);                       // a gene without a base holds no event
  EXPECT(rule(2, 49, 1, 1, 3) == 0 && (key >> 32) == 149);
  EXPECT(rule(3, 0, 0, 1, 0) == 1);
  EXPECT(rule(0xFFFFFFFFu, 0, 0, 1, 0) == 1);
  EXPECT(rule(0, 0, 2, 1, 0) == 2);
  EXPECT(rule(0, 0, 0, 1, 0, 1) == 2);
  EXPECT(rule(0, 0, 0, 0, 0) == 3);
  EXPECT(rule(0, 0, 0, 65536, 0) == 3);
  EXPECT(rule(0, 0, 0, 1, 1) == 3);
  EXPECT(rule(0, 0, 1, 0, 0) == 3);
  EXPECT(rule(0, 0, 1, 13, 0) == 3);
  EXPECT(rule(0, 0, 1, 0xFFFFFFFFu, 0) == 3);             // (no shift by 2 * len is taken: the length is refused first)
  EXPECT(rule(0, 0, 1, 2, 16) == 3);
  EXPECT(rule(0, 0xFFFFFFFFu, 0, 65535, 0) == 4);         // (x + len does not wrap)
  for (int r = 1; r <= 4; ++r) EXPECT(INDEL_ENTRY_RULES[r][0] != 0);
  // keys ascend with (gene, x, kind, len, seq), and the event's half reads back
  const unsigned long long order[] = {indel_key(5, 0, 1, 0), indel_key(5, 0, 65535, 0), indel_key(5, 1, 1, 0), indel_key(5, 1, 1, 3), indel_key(5, 1, 12, 0),
                                      indel_key(6, 0, 1, 0)};
  for (size_t i = 0; i + 1 < sizeof(order) / sizeof(order[0]); ++i) EXPECT(order[i] < order[i + 1]);
  EXPECT(indel_key(0xFFFFFFFEull, 1, 12, 0xFFFFFFu) != ~0ull);
  shk_indel back{};
  indel_key_event((uint32_t)indel_key(7, 1, 12, 0xABCDEFu), back);
  EXPECT(back.kind == 1 && back.len == 12 && back.seq == 0xABCDEFu);
  indel_key_event((uint32_t)indel_key(7, 0, 65535, 0), back);
  EXPECT(back.kind == 0 && back.len == 65535 && back.seq == 0);
  // the line writer
  std::string text;
  const uint32_t gattaca = 2u | 0u << 2 | 3u << 4 | 3u << 6 | 0u << 8 | 1u << 10 | 0u << 12;
  indel_line(shk_indel{0, 550, 1, 7, gattaca, 8, 9, 0}, "geneA", text);
  indel_line(shk_indel{1, 400, 0, 3, 0, 10, 0, 0}, "", text);
  indel_line(shk_indel{2, 0xFFFFFFFFu, 0, 65535, 0, 0xFFFFFFFFu, 0xFFFFFFFFu, 0}, "g", text);
  indel_line(shk_indel{2, 0, 1, 12, 0xFFFFFFu, 1, 1, 0}, "g", text);
  EXPECT(text == "geneA 550 I 7 GATTACA 8 9\n 400 D 3 * 10 0\ng 4294967295 D 65535 * 4294967295 4294967295\ng 0 I 12 TTTTTTTTTTTT 1 1\n");
  if (failures) return EXIT_FAILURE;
  std::puts("indel host check ok");
  return EXIT_SUCCESS;
}
