// shark-ktab-check -- host-only print-out of ktab_home (kmer_device.hpp): where the minimiser-bucketed table keeps a k-mer and the
// word its slot is compared with, computed by the very function the build and classify kernels call (it is __host__ __device__;
// this file is compiled as HIP for that reason and needs no device at run time).  tests/test_ktab_audit.py pins the Python
// restatement of the layout (tests/ktab_audit.py: ktab_home_model) to it.
// usage: shark-ktab-check < input   with input = "K W LINE_LG" followed by k-mers as decimal numbers (first base most
//   significant, either strand) -> one line "bucket want" per k-mer
#include <cstdio>
#include <cstdlib>

#include "kmer_device.hpp"

int main()
{
  unsigned k = 0, w = 0, line_lg = 0;
  if (scanf("%u %u %u", &k, &w, &line_lg) != 3 || k < 3 || k > 17 || w < 1 || w > 15 || w > k || k - w > 3 || line_lg < 1 || line_lg > 28) {
    fprintf(stderr, "usage: shark-ktab-check < input   (input: K W LINE_LG, then k-mers; 3 <= K <= 17, K - 3 <= W <= min(K, 15), 1 <= LINE_LG <= 28)\n");
    return 2;
  }
  unsigned long long x;
  while (scanf("%llu", &x) == 1) {
    if (x >> (2u * k)) { fprintf(stderr, "%llu is not a %u-mer\n", x, k); return 2; }
    uint64_t rc = 0, t = ~(uint64_t)x;
    for (unsigned i = 0; i < k; ++i) { rc = (rc << 2) | (t & 3u); t >>= 2; }
    uint32_t bucket = 0, want = 0;
    shk::ktab_home((uint64_t)x, rc, k, w, line_lg, bucket, want);
    printf("%u %u\n", bucket, want);
  }
  return 0;
}
