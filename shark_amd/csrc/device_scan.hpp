// device_scan.hpp -- exclusive prefix sum of uint32 arrays on gfx950.
//
// Three launches (tile sums -> scan of the tile sums in one workgroup -> per-tile scan with the
// tile's offset); 16 contiguous items per thread as four 16-byte accesses, wave64 shuffles inside
// a workgroup.  Streaming, bandwidth-bound: 2 reads + 1 write of the array (10 M items: 30 + 10 +
// 45 us; the first version -- 8 items per thread, dword accesses, 64-bit shuffles -- took 290).  Used by the rank
// directory (bloomfilter.h:121 init_support(_brank)), the gene-list CSR
// (bloomfilter.h:142-167) and the result offsets of classify.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace shk {

constexpr int SCAN_THREADS = 256;
constexpr int SCAN_ITEMS = 16;                     // per thread
constexpr int SCAN_TILE = SCAN_THREADS * SCAN_ITEMS;  // 4096

// temp: (ntiles + 1) uint64_t; the grand total lands in temp[ntiles].
inline uint64_t scan_temp_words(uint64_t n) { return (n + SCAN_TILE - 1) / SCAN_TILE + 1; }

// exclusive scan in -> out (may alias); returns the device pointer holding the 64-bit total
const uint64_t *exclusive_scan_u32(const uint32_t *in, uint32_t *out, uint64_t n, uint64_t *temp, hipStream_t stream);

// The result of a batch against an index of ONE record without wrap, assembled by the scan itself (shark_hip.hip, enqueue_tail): a
// read's list there is {} or {0}, so gene_ids[0 .. total) is `total` copies of id 0 and gene 0 was assigned `total` reads.  The same
// three launches as exclusive_scan_u32 over count[0 .. n) -> gene_off[0 .. n) (n >= 1, no aliasing, temp as above), with
//   * an epilogue in the tile-offsets kernel: the thread that writes the total also writes counters[CTR_ASSOC_LO / _HI], sets
//     counters[CTR_OVERFLOW] = total > gene_ids_cap (finalize_total_kernel's job) and adds the total to gene_counts[0] exactly when
//     gene_hist_kernel would have counted the batch: count_genes, no overflow, and not (skip_if_long and counters[CTR_LONG] != 0);
//   * a fill in the apply kernel: workgroup b writes id 0 to gene_ids[tile_offs[b] .. tile_offs[b] + its tile's sum), coalesced (16-byte
//     stores between a head and a tail of fewer than 8 ids); nothing at or beyond gene_ids_cap, nothing at all on overflow.
// Returns the device pointer holding the 64-bit total.
struct OneRecordResult {
  uint16_t *gene_ids;
  uint64_t gene_ids_cap;
  uint32_t *counters;                   // the batch's counter block (shark_internal.hpp, CTR_*)
  unsigned long long *gene_counts;      // the context's per-gene counters (only [0] is touched); may be null when !count_genes
  bool count_genes, skip_if_long;
  // a speculated batch (shark_hip.hip, enqueue_classify): uniform_check_kernel's words {verdict, L1, L2}, final before this scan starts,
  // and the lengths its classify launch assumed.  Anything but "uniform, of these lengths": the epilogue sets counters[CTR_SPEC_MISS]
  // and adds nothing to gene_counts.  nullptr: not speculated
  const uint32_t *spec_verdict = nullptr;
  uint32_t spec_L1 = 0, spec_L2 = 0;
};
const uint64_t *exclusive_scan_assemble_one(const uint32_t *count, uint32_t *gene_off, uint64_t n, uint64_t *temp, const OneRecordResult &r,
                                            hipStream_t stream);

}  // namespace shk
