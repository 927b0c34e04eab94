/*
 * sdsl_standin_check.cpp -- C exports over the sdsl stand-in (oracle/sdsl_standin)
 * so that tests can check its rank and select against numpy.
 */
#include <cstdint>

#include <sdsl/bit_vectors.hpp>
#include <sdsl/util.hpp>

extern "C" {

/* bits: n bytes of 0/1.  rank_out: n + 1 values, rank(i) for i = 0..n.
 * select_out: one value per one, select(j) for j = 1..ones.  Returns the number of ones. */
uint64_t standin_rank_select(const uint8_t *bits, uint64_t n, uint64_t *rank_out, uint64_t *select_out)
{
  sdsl::bit_vector bv(n, 0);
  for (uint64_t i = 0; i < n; ++i)
    if (bits[i]) bv[i] = 1;
  const sdsl::bit_vector &cbv = bv;
  for (uint64_t i = 0; i < n; ++i)
    if (cbv[i] != (bits[i] != 0)) return UINT64_MAX;
  sdsl::bit_vector::rank_1_type r;
  sdsl::util::init_support(r, &bv);
  for (uint64_t i = 0; i <= n; ++i) rank_out[i] = r(i);
  const uint64_t ones = r(bv.size());
  sdsl::bit_vector::select_1_type s;
  sdsl::util::init_support(s, &bv);
  for (uint64_t j = 1; j <= ones; ++j) select_out[j - 1] = s(j);
  return ones;
}

} /* extern "C" */
