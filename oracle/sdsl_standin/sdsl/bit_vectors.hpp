/*
 * sdsl_standin/sdsl/bit_vectors.hpp -- a small stand-in for the part of
 * sdsl-lite's bit vector API that the reference's bloomfilter.h uses, so that
 * the reference CLI can be compiled in place (test infrastructure only).
 *
 * Semantics follow sdsl's documentation:
 *   bit_vector(n, v)   n bits, all set to v
 *   bv[i]              assignable proxy; const read gives bool
 *   rank_1_type r(i)   number of ones in [0, i), valid for 0 <= i <= size()
 *   select_1_type s(j) position of the j-th one, j >= 1
 * The rank directory keeps one 64-bit count per 512 bits (1/8 bit per bit), so
 * that a 2^33-bit filter costs 128 MiB of directory rather than another GiB.
 *
 * sdsl's headers pull in standard headers that the reference relies on without
 * including them itself (<map> in ReadAnalyzer.hpp; <mutex>, <chrono>, <array>
 * in main.cpp); they are included here for the same reason.
 */
#ifndef SHARK_SDSL_STANDIN_BIT_VECTORS_HPP
#define SHARK_SDSL_STANDIN_BIT_VECTORS_HPP

#include <array>
#include <chrono>
#include <cstddef>
#include <cstdint>
#include <map>
#include <mutex>
#include <vector>

namespace sdsl {

class rank_support_v5;
class select_support_scan;

class bit_vector {
public:
  typedef uint64_t size_type;
  typedef rank_support_v5 rank_1_type;
  typedef select_support_scan select_1_type;

  class reference {
  public:
    reference(uint64_t *w, unsigned b) : w_(w), b_(b) {}
    reference &operator=(bool v)
    {
      if (v) *w_ |= uint64_t(1) << b_;
      else *w_ &= ~(uint64_t(1) << b_);
      return *this;
    }
    reference &operator=(const reference &o) { return *this = bool(o); }
    operator bool() const { return (*w_ >> b_) & 1; }

  private:
    uint64_t *w_;
    unsigned b_;
  };

  bit_vector() {}
  explicit bit_vector(size_type n, bool v = false) : n_(n), w_((n + 63) / 64, v ? ~uint64_t(0) : 0)
  {
    if (v && (n & 63)) w_.back() &= (uint64_t(1) << (n & 63)) - 1;  /* bits past size() stay zero */
  }

  reference operator[](size_type i) { return reference(&w_[i >> 6], unsigned(i & 63)); }
  bool operator[](size_type i) const { return (w_[i >> 6] >> (i & 63)) & 1; }
  size_type size() const { return n_; }
  const uint64_t *data() const { return w_.data(); }
  size_type words() const { return w_.size(); }

private:
  size_type n_ = 0;
  std::vector<uint64_t> w_;
};

/* rank of ones: block counts every 8 words, popcounts inside the block */
class rank_support_v5 {
public:
  rank_support_v5() {}
  explicit rank_support_v5(const bit_vector *v) { set_vector(v); }
  void set_vector(const bit_vector *v)
  {
    v_ = v;
    blocks_.clear();
    if (!v) return;
    const uint64_t *w = v->data();
    const uint64_t nw = v->words();
    blocks_.assign(nw / 8 + 1, 0);
    uint64_t acc = 0;
    for (uint64_t i = 0; i < nw; ++i) {
      if ((i & 7) == 0) blocks_[i / 8] = acc;
      acc += __builtin_popcountll(w[i]);
    }
    if ((nw & 7) == 0) blocks_[nw / 8] = acc;
  }
  uint64_t rank(uint64_t i) const
  {
    const uint64_t *w = v_->data();
    const uint64_t wi = i >> 6;
    uint64_t r = blocks_[wi >> 3];
    for (uint64_t j = wi & ~uint64_t(7); j < wi; ++j) r += __builtin_popcountll(w[j]);
    if (i & 63) r += __builtin_popcountll(w[wi] & ((uint64_t(1) << (i & 63)) - 1));
    return r;
  }
  uint64_t operator()(uint64_t i) const { return rank(i); }

private:
  const bit_vector *v_ = nullptr;
  std::vector<uint64_t> blocks_;
};

/* select of ones: the position of every 64th one is sampled, then words are scanned */
class select_support_scan {
public:
  select_support_scan() {}
  explicit select_support_scan(const bit_vector *v) { set_vector(v); }
  void set_vector(const bit_vector *v)
  {
    v_ = v;
    samples_.clear();
    if (!v) return;
    const uint64_t *w = v->data();
    uint64_t seen = 0;
    for (uint64_t i = 0; i < v->words(); ++i) {
      uint64_t x = w[i];
      while (x) {
        if ((seen & 63) == 0) samples_.push_back(i * 64 + __builtin_ctzll(x));
        ++seen;
        x &= x - 1;
      }
    }
  }
  uint64_t select(uint64_t j) const
  {
    const uint64_t s = (j - 1) >> 6;
    uint64_t pos = samples_[s];
    uint64_t left = (j - 1) & 63;           /* ones still to pass after the sampled one */
    const uint64_t *w = v_->data();
    uint64_t wi = pos >> 6;
    uint64_t x = w[wi] & (~uint64_t(0) << (pos & 63));
    for (;;) {
      const uint64_t c = __builtin_popcountll(x);
      if (left < c) break;
      left -= c;
      x = w[++wi];
    }
    while (left--) x &= x - 1;
    return wi * 64 + __builtin_ctzll(x);
  }
  uint64_t operator()(uint64_t j) const { return select(j); }

private:
  const bit_vector *v_ = nullptr;
  std::vector<uint64_t> samples_;
};

} // namespace sdsl

#endif
