// debug_primitives.hip -- test-only entry points that run exclusive_scan_u32 and radix_sort_u64 on caller-supplied data
// (shk_debug_scan_u32, shk_debug_sort_u64; documented in shark_internal.hpp next to shk_debug_index_array).  Exported from the
// library, not declared in include/shark_hip.h, used by no classify or build path.  shk_debug_assemble_one runs the scan's one-record
// form (device_scan.hpp, exclusive_scan_assemble_one) the same way; that one is declared in include/shark_hip.h.
//
// Every device buffer handed down sits between two guard bands inside its own allocation: at least DBG_GUARD words of
// DBG_PATTERN in front of it and behind it.  After the run the whole allocation comes back to the host and the guard words that
// no longer hold the pattern are counted per band -- a write outside [0, n) or a helper array sized too small shows up as a
// non-zero count, and nothing ever leaves an allocation for it.
#include <vector>

#include "device_scan.hpp"
#include "device_sort.hpp"
#include "shark_internal.hpp"

namespace shk {
namespace {

constexpr uint64_t DBG_GUARD = 64;                        // words per band (a misaligned buffer's front band has up to 3 more)
constexpr uint64_t DBG_PATTERN = 0xC3A5F00DC3A5F00Dull;   // every guard word (truncated for 32-bit words)
constexpr uint64_t DBG_FILL = 0x3C5A0FF23C5A0FF2ull;      // what a payload the caller does not supply starts as
static_assert((uint16_t)DBG_FILL == SHK_DEBUG_FILL16 && SHK_DEBUG_COUNTER_WORDS == COUNTER_BLOCK_WORDS && SHK_DEBUG_CTR_LONG == CTR_LONG &&
                  SHK_DEBUG_CTR_OVERFLOW == CTR_OVERFLOW && SHK_DEBUG_CTR_ASSOC_LO == CTR_ASSOC_LO && SHK_DEBUG_CTR_ASSOC_HI == CTR_ASSOC_HI,
              "what include/shark_hip.h says of shk_debug_assemble_one");

// one device allocation [front guard | n payload words | back guard] with its host image
template <typename T>
struct Guarded {
  T *base = nullptr;
  uint64_t front = 0, n = 0;
  std::vector<T> img;
  Guarded() = default;
  Guarded(const Guarded &) = delete;
  Guarded &operator=(const Guarded &) = delete;
  ~Guarded() { if (base) (void)hipFree(base); }
  T *dev() const { return base + front; }
  // the payload starts `off` words behind a 256-byte aligned address (hipMalloc's alignment; DBG_GUARD words keep it)
  hipError_t alloc(uint64_t n_words, uint64_t off, const T *payload, hipStream_t stream)
  {
    static_assert((DBG_GUARD * sizeof(T)) % 16 == 0, "the front band keeps the payload's alignment");
    front = DBG_GUARD + off;
    n = n_words;
    img.assign(front + n + DBG_GUARD, (T)DBG_PATTERN);
    for (uint64_t i = 0; i < n; ++i) img[front + i] = payload ? payload[i] : (T)DBG_FILL;
    hipError_t e = hipMalloc((void **)&base, img.size() * sizeof(T));
    if (e != hipSuccess) { base = nullptr; return e; }
    return hipMemcpyAsync(base, img.data(), img.size() * sizeof(T), hipMemcpyHostToDevice, stream);
  }
  hipError_t fetch(hipStream_t stream) { return hipMemcpyAsync(img.data(), base, img.size() * sizeof(T), hipMemcpyDeviceToHost, stream); }
  const T *payload() const { return img.data() + front; }
  // changed[0] = guard words in front that lost the pattern, changed[1] = behind
  void count(uint32_t *changed) const
  {
    changed[0] = changed[1] = 0;
    for (uint64_t i = 0; i < front; ++i) changed[0] += img[i] != (T)DBG_PATTERN;
    for (uint64_t i = front + n; i < img.size(); ++i) changed[1] += img[i] != (T)DBG_PATTERN;
  }
};

}  // namespace
}  // namespace shk

using namespace shk;

extern "C" {

int shk_debug_scan_u32(shk_ctx *ctx, const uint32_t *in, uint64_t n, uint32_t in_off, uint32_t out_off, int in_place, uint32_t *out,
                       uint32_t *in_after, uint64_t *total, uint32_t *guard_changed)
{
  if (!ctx || !total || !guard_changed || in_off > 3 || out_off > 3) return SHK_ERR_ARG;
  if (n && (!in || !out || !in_after)) return SHK_ERR_ARG;
  if (in_place && in_off != out_off) return SHK_ERR_ARG;
  SHK_HIP(ctx, hipSetDevice(ctx->prm.device));
  try {
    Guarded<uint32_t> gin, gout;
    Guarded<uint64_t> gtemp;
    SHK_HIP(ctx, gin.alloc(n, in_off, in, ctx->stream));
    if (!in_place) SHK_HIP(ctx, gout.alloc(n, out_off, nullptr, ctx->stream));
    SHK_HIP(ctx, gtemp.alloc(scan_temp_words(n), 0, nullptr, ctx->stream));
    Guarded<uint32_t> &go = in_place ? gin : gout;
    const uint64_t *d_total = exclusive_scan_u32(gin.dev(), go.dev(), n, gtemp.dev(), ctx->stream);
    SHK_HIP(ctx, hipGetLastError());
    if (d_total < gtemp.dev() || d_total >= gtemp.dev() + gtemp.n) return SHK_ERR_HIP;   // (the total lies inside temp by contract)
    const uint64_t total_at = (uint64_t)(d_total - gtemp.dev());
    // (the input's image is taken before the output's so that in place both are the one buffer as it stands afterwards)
    SHK_HIP(ctx, gin.fetch(ctx->stream));
    if (!in_place) SHK_HIP(ctx, gout.fetch(ctx->stream));
    SHK_HIP(ctx, gtemp.fetch(ctx->stream));
    SHK_HIP(ctx, hipStreamSynchronize(ctx->stream));
    for (uint64_t i = 0; i < n; ++i) { in_after[i] = gin.payload()[i]; out[i] = go.payload()[i]; }
    *total = gtemp.payload()[total_at];
    gin.count(guard_changed);
    go.count(guard_changed + 2);
    gtemp.count(guard_changed + 4);
  } catch (...) {
    return SHK_ERR_NOMEM;
  }
  return SHK_OK;
}

int shk_debug_sort_u64(shk_ctx *ctx, const uint64_t *keys, uint64_t n, uint32_t end_bit, uint64_t *out, int *which, uint32_t *guard_changed)
{
  if (!ctx || !which || !guard_changed || end_bit > 64 || n >= (1ull << 32)) return SHK_ERR_ARG;
  if (n && (!keys || !out)) return SHK_ERR_ARG;
  SHK_HIP(ctx, hipSetDevice(ctx->prm.device));
  try {
    Guarded<uint64_t> ga, gb, gtmp;
    Guarded<uint32_t> ghist;
    const uint64_t hist_words = radix_sort_hist_words(n);
    SHK_HIP(ctx, ga.alloc(n, 0, keys, ctx->stream));
    SHK_HIP(ctx, gb.alloc(n, 0, nullptr, ctx->stream));
    SHK_HIP(ctx, ghist.alloc(hist_words, 0, nullptr, ctx->stream));
    SHK_HIP(ctx, gtmp.alloc(scan_temp_words(hist_words), 0, nullptr, ctx->stream));
    const uint64_t *res = radix_sort_u64(ga.dev(), gb.dev(), n, end_bit, ghist.dev(), gtmp.dev(), ctx->stream);
    SHK_HIP(ctx, hipGetLastError());
    if (res != ga.dev() && res != gb.dev()) return SHK_ERR_HIP;   // (nullptr: a launch failed)
    *which = res == gb.dev() ? 1 : 0;
    SHK_HIP(ctx, ga.fetch(ctx->stream));
    SHK_HIP(ctx, gb.fetch(ctx->stream));
    SHK_HIP(ctx, ghist.fetch(ctx->stream));
    SHK_HIP(ctx, gtmp.fetch(ctx->stream));
    SHK_HIP(ctx, hipStreamSynchronize(ctx->stream));
    const uint64_t *sorted = *which ? gb.payload() : ga.payload();
    for (uint64_t i = 0; i < n; ++i) out[i] = sorted[i];
    ga.count(guard_changed);
    gb.count(guard_changed + 2);
    ghist.count(guard_changed + 4);
    gtmp.count(guard_changed + 6);
  } catch (...) {
    return SHK_ERR_NOMEM;
  }
  return SHK_OK;
}

int shk_debug_assemble_one(shk_ctx *ctx, const uint32_t *count, uint64_t n, uint32_t count_off, uint32_t off_off, uint64_t gene_ids_cap, uint32_t ctr_long,
                           int skip_if_long, int count_genes, uint32_t *gene_off, uint16_t *gene_ids, uint32_t *counters, uint64_t *gene0_added,
                           uint32_t *guard_changed)
{
  if (!ctx || !count || !gene_off || !counters || !gene0_added || !guard_changed || n == 0 || count_off > 3 || off_off > 3) return SHK_ERR_ARG;
  if (gene_ids_cap && !gene_ids) return SHK_ERR_ARG;
  SHK_HIP(ctx, hipSetDevice(ctx->prm.device));
  try {
    Guarded<uint32_t> gcount, goff, gctr;
    Guarded<uint64_t> gtemp, ggene;
    Guarded<uint16_t> gids;
    std::vector<uint32_t> ctr0(COUNTER_BLOCK_WORDS, 0u);
    ctr0[CTR_LONG] = ctr_long;
    const uint64_t gene0 = 0;
    SHK_HIP(ctx, gcount.alloc(n, count_off, count, ctx->stream));
    SHK_HIP(ctx, goff.alloc(n, off_off, nullptr, ctx->stream));
    SHK_HIP(ctx, gtemp.alloc(scan_temp_words(n), 0, nullptr, ctx->stream));
    SHK_HIP(ctx, gids.alloc(gene_ids_cap, 0, nullptr, ctx->stream));
    SHK_HIP(ctx, gctr.alloc(COUNTER_BLOCK_WORDS, 0, ctr0.data(), ctx->stream));
    SHK_HIP(ctx, ggene.alloc(1, 0, &gene0, ctx->stream));
    const OneRecordResult r{gids.dev(), gene_ids_cap, gctr.dev(), reinterpret_cast<unsigned long long *>(ggene.dev()), count_genes != 0, skip_if_long != 0};
    const uint64_t *d_total = exclusive_scan_assemble_one(gcount.dev(), goff.dev(), n, gtemp.dev(), r, ctx->stream);
    SHK_HIP(ctx, hipGetLastError());
    if (d_total < gtemp.dev() || d_total >= gtemp.dev() + gtemp.n) return SHK_ERR_HIP;   // (the total lies inside temp by contract)
    SHK_HIP(ctx, gcount.fetch(ctx->stream));
    SHK_HIP(ctx, goff.fetch(ctx->stream));
    SHK_HIP(ctx, gtemp.fetch(ctx->stream));
    SHK_HIP(ctx, gids.fetch(ctx->stream));
    SHK_HIP(ctx, gctr.fetch(ctx->stream));
    SHK_HIP(ctx, ggene.fetch(ctx->stream));
    SHK_HIP(ctx, hipStreamSynchronize(ctx->stream));
    for (uint64_t i = 0; i < n; ++i) gene_off[i] = goff.payload()[i];
    for (uint64_t i = 0; i < gene_ids_cap; ++i) gene_ids[i] = gids.payload()[i];
    for (uint32_t i = 0; i < COUNTER_BLOCK_WORDS; ++i) counters[i] = gctr.payload()[i];
    *gene0_added = ggene.payload()[0];
    // (the scan's own total must be what the epilogue put into the counters: both are handed out, the second through them)
    if (gtemp.payload()[d_total - gtemp.dev()] != (((uint64_t)counters[CTR_ASSOC_HI] << 32) | counters[CTR_ASSOC_LO])) return SHK_ERR_HIP;
    gcount.count(guard_changed);
    goff.count(guard_changed + 2);
    gtemp.count(guard_changed + 4);
    gids.count(guard_changed + 6);
    gctr.count(guard_changed + 8);
    ggene.count(guard_changed + 10);
    // (the counts are an input: a changed word of theirs counts as a guard word behind them)
    for (uint64_t i = 0; i < n; ++i) guard_changed[1] += gcount.payload()[i] != count[i];
  } catch (...) {
    return SHK_ERR_NOMEM;
  }
  return SHK_OK;
}

}  // extern "C"
