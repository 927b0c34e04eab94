/*
 * sdsl_standin/sdsl/util.hpp -- util::init_support of the sdsl stand-in
 * (see bit_vectors.hpp): (re)binds a rank or select support to a bit vector.
 */
#ifndef SHARK_SDSL_STANDIN_UTIL_HPP
#define SHARK_SDSL_STANDIN_UTIL_HPP

namespace sdsl {
namespace util {

template <class Support, class BitVector>
void init_support(Support &s, const BitVector *v)
{
  s.set_vector(v);
}

} // namespace util
} // namespace sdsl

#endif
