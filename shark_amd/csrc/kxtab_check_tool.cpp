// shark-kxtab-check -- host-only check of the k-mer keyed exact table (kmer_table.hpp): builds the image for a key set and verifies,
// with the lookup rule the kernel uses, that every key is found, that M random 34-bit values are answered exactly as a std::set of
// the keys answers them, and that the adversarial non-keys of every key are not found: the key with any one of its 34 bits
// flipped, and the other values that share its slot before the displacement and its group (they differ in the tag's bits above the
// group, land on the key's own slot and have to be told apart by the stored tag alone).  `candidate_non_keys` counts the non-keys among
// all these probes that pass the first of the lookup's two stages (kxtab_candidate: the tag's low 16 bits) and are turned down by the
// second; `two_stage_diff` the probes, keys included, for which the two stages and the one-call rule disagree (none).
// usage: shark-kxtab-check KIND N SEED [M [SHUFFLE]]   -> one JSON object
//   KIND random: N distinct random 34-bit keys;  polya / repeat: the canonical 17-mers of N + 16 bases of poly-A / of an AC repeat
//   with a substitution every few dozen bases (low complexity: few distinct keys, close to one another)
//   SHUFFLE != 0: the keys are handed to the builder in an order shuffled with that seed (the image must not depend on it)
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <set>
#include <string>

#include "kmer_table.hpp"

// the inverse of kxtab_mix: the key with this tag and this slot before the displacement
static uint64_t unmix(uint32_t tag, uint32_t base, uint32_t m1, uint32_t m2)
{
  const uint32_t a = (base ^ ((tag * (m2 & 0xFFFFFFu)) >> 16)) & 0xFFFFu;
  const uint32_t b = tag ^ ((((a + 1u) * (m1 & 0xFFFFFFu)) >> 6) & shk::KXTAB_TAG_MASK);
  return ((uint64_t)b << 16) | a;
}

int main(int argc, char **argv)
{
  if (argc < 4) { fprintf(stderr, "usage: %s random|polya|repeat N SEED [M [SHUFFLE]]\n", argv[0]); return 2; }
  const std::string kind(argv[1]);
  const uint32_t n = (uint32_t)atoi(argv[2]);
  const uint64_t seed = strtoull(argv[3], nullptr, 10), m = argc > 4 ? strtoull(argv[4], nullptr, 10) : 1000000ull;
  const uint64_t shuffle = argc > 5 ? strtoull(argv[5], nullptr, 10) : 0ull;
  const uint64_t mask = (1ull << shk::KXTAB_KEY_BITS) - 1ull;
  std::mt19937_64 rng(seed);
  std::set<uint64_t> set;
  if (kind == "random") {
    while (set.size() < n) set.insert(rng() & mask);
  } else if (kind == "polya" || kind == "repeat") {
    const uint32_t k = 17;
    std::vector<uint32_t> seq(n + k - 1);
    for (size_t i = 0; i < seq.size(); ++i) seq[i] = kind == "polya" ? 0u : (uint32_t)(i & 1u);
    for (size_t i = rng() % 40; i < seq.size(); i += 20 + rng() % 40) seq[i] = (uint32_t)(rng() & 3u);
    for (size_t s = 0; s + k <= seq.size(); ++s) {
      uint64_t fwd = 0, rc = 0;
      for (uint32_t j = 0; j < k; ++j) { fwd = (fwd << 2) | seq[s + j]; rc |= (uint64_t)(3u - seq[s + j]) << (2u * j); }
      set.insert(fwd < rc ? fwd : rc);
    }
  } else { fprintf(stderr, "unknown kind %s\n", kind.c_str()); return 2; }
  std::vector<uint64_t> keys(set.begin(), set.end());
  if (shuffle) { std::mt19937_64 r2(shuffle); std::shuffle(keys.begin(), keys.end(), r2); }
  std::vector<uint8_t> img;
  uint32_t m1 = 0, m2 = 0, attempts = 0;
  const auto t0 = std::chrono::steady_clock::now();
  const bool built = shk::kxtab_build(keys, img, &m1, &m2, &attempts);
  const double build_us = std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count();
  unsigned long long missing = 0, false_pos = 0, false_neg = 0, used = 0, flip_fp = 0, flip_probes = 0, slot_fp = 0, slot_probes = 0, cand_non_keys = 0, two_stage_diff = 0, hash = 1469598103934665603ull;
  // (the two stages against the one-call rule, for every probe; a non-key: did it pass the candidate stage?)
  auto lookup = [&](const uint64_t v, const bool is_key) -> bool {
    uint32_t tag, s2;
    const bool cand = shk::kxtab_candidate(img.data(), m1, m2, v, tag, s2), got = shk::kxtab_lookup(img.data(), m1, m2, v);
    if (!is_key && cand) ++cand_non_keys;
    if ((cand && shk::kxtab_confirm(img.data(), tag, s2)) != got) ++two_stage_diff;
    return got;
  };
  if (built) {
    for (uint32_t s = 0; s < shk::KXTAB_SLOTS; ++s) {
      uint16_t t16;
      memcpy(&t16, img.data() + 2u * s, 2);
      used += (t16 | ((img[shk::KXTAB_T2_OFF + (s >> 2)] >> (2u * (s & 3u))) & 3u)) != 0u;   // (an entry equal to the empty encoding would not count)
    }
    for (const uint8_t b : img) hash = (hash ^ b) * 1099511628211ull;
    for (const uint64_t c : keys) {
      if (!lookup(c, true)) ++missing;
      for (uint32_t bit = 0; bit < shk::KXTAB_KEY_BITS; ++bit) {
        const uint64_t v = c ^ (1ull << bit);
        if (set.count(v)) continue;
        ++flip_probes;
        flip_fp += lookup(v, false);
      }
      uint32_t tag, base;
      shk::kxtab_mix(c, m1, m2, tag, base);
      for (uint32_t h = 1; h < (1u << (shk::KXTAB_TAG_BITS - shk::KXTAB_GROUP_LG)); ++h) {
        const uint64_t v = unmix(tag ^ (h << shk::KXTAB_GROUP_LG), base, m1, m2);
        if (set.count(v)) continue;
        ++slot_probes;
        slot_fp += lookup(v, false);
      }
    }
    for (uint64_t i = 0; i < m; ++i) {
      const uint64_t v = rng() & mask;
      const bool want = set.count(v) != 0, got = lookup(v, want);
      false_pos += got && !want;
      false_neg += !got && want;
    }
  }
  printf("{\"built\": %s, \"m1\": %u, \"m2\": %u, \"attempts\": %u, \"keys\": %zu, \"capacity\": %u, \"bytes\": %u, \"slots_used\": %llu, \"missing\": %llu, "
         "\"false_pos\": %llu, \"false_neg\": %llu, \"probes\": %llu, \"flip_false_pos\": %llu, \"flip_probes\": %llu, \"slot_false_pos\": %llu, "
         "\"slot_probes\": %llu, \"candidate_non_keys\": %llu, \"two_stage_diff\": %llu, \"image_hash\": \"%016llx\", \"build_us\": %.0f}\n",
         built ? "true" : "false", m1, m2, attempts, keys.size(), shk::KXTAB_MAX_KEYS, shk::KXTAB_BYTES, used, missing, false_pos, false_neg,
         (unsigned long long)m, flip_fp, flip_probes, slot_fp, slot_probes, cand_non_keys, two_stage_diff, built ? hash : 0ull, build_us);
  return 0;
}
