/*
 * shark_hip.h -- C ABI of libsharkhip: the MI355X (gfx950) implementation of
 * shark's k-mer classification hot path.
 *
 * shark (AlgoLab/shark) has no plugin/FFI interface; the seam this library
 * replaces is the group of functor calls inside the two worker loops of
 * main.cpp plus the BF methods they use.  Each entry point below cites the
 * reference interface it stands in for (file:line relative to the reference
 * tree).  Plain pointers and sizes only; no C++/torch types; every function
 * returns 0 (SHK_OK) or a negative error code and never throws.
 *
 * Mode machine (bloomfilter.h:104-110): shk_ref_add* -> shk_ref_finalize ->
 * shk_classify*; going backwards returns SHK_ERR_STATE.
 *
 * There is NO CPU fallback: without a HIP device every call that computes
 * fails with SHK_ERR_HIP / SHK_ERR_NO_DEVICE.
 *
 * Threading: a context serialises nothing by itself -- use one context per
 * host thread (and per GPU); different contexts may be used concurrently.  The
 * reference's ReadAnalyzer is const over a frozen index (ReadAnalyzer.hpp:39,
 * main.cpp:193); here every context owns a replica of that index.
 */
#ifndef SHARK_HIP_H
#define SHARK_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SHK_OK                    0
#define SHK_ERR_ARG              -1  /* bad argument (k outside [1,31], c outside [0,1], NULL, ...) */
#define SHK_ERR_STATE            -2  /* call not allowed in the current mode */
#define SHK_ERR_HIP              -3  /* HIP runtime error; text via shk_last_error */
#define SHK_ERR_NOMEM            -4
#define SHK_ERR_TOO_MANY_GENES   -5  /* >= 2^31 FASTA records (more than 65 536 genes are handled as the reference handles them:
                                        ids wrap to uint16_t, small_vector.hpp:46, and are not de-duplicated, bloomfilter.h:72) */
#define SHK_ERR_INDEX_TOO_LARGE  -6  /* >= 2^31 set bits or list entries (int in bloomfilter.h:70,:130) */
#define SHK_ERR_NO_DEVICE        -7

#define SHK_INLINE_IDS 4             /* gene ids stored inline per read in the device result */

typedef struct shk_ctx shk_ctx;

/* argument_parser.hpp:49-63 (namespace opt) */
typedef struct shk_params {
  uint32_t k;            /* -k, default 17, range [1,31]      (:56, :112-121) */
  double   c;            /* -c, default 0.6, range [0,1]      (:57, :122-129) */
  uint64_t bf_bits;      /* filter size in BITS; -b N => N<<33 (:58, :130-134) */
  int32_t  min_quality;  /* -q, 0 = no masking; any value >= 0: stored as the reference's `char`
                            (:59, :135-145), so -q > 94 wraps exactly as it does there          */
  int32_t  single;       /* -s                                 (:60, :146-148) */
  int32_t  device;       /* HIP device ordinal */
} shk_params;

/* BF::BF(size) bloomfilter.h:48-53 + ReadAnalyzer ctor ReadAnalyzer.hpp:36-37 */
int  shk_create(const shk_params *params, shk_ctx **out);
void shk_destroy(shk_ctx *ctx);
const char *shk_strerror(int code);
const char *shk_last_error(const shk_ctx *ctx);

/* ---- index build -------------------------------------------------------- */
/* One FASTA record, in FILE ORDER, including records shorter than k and
 * records without any valid k-mer (the library reproduces main.cpp:162-186's
 * gene numbering, quirk included).  Stands in for
 *   FastaSplitter::operator()   FastaSplitter.hpp:42-54  (record order = legend order)
 *   KmerBuilder::operator()     KmerBuilder.hpp:40-72
 *   BloomfilterFiller::operator() BloomfilterFiller.hpp:38-46 / BF::add_at bloomfilter.h:57-59
 *   pass 2 + BF::add_to_kmer    main.cpp:154-189, bloomfilter.h:61-75
 * The sequence bytes are only buffered here; all k-mer work happens on the
 * device in shk_ref_finalize. */
int shk_ref_add(shk_ctx *ctx, const char *seq, uint64_t len);

/* BF::switch_mode(1) + switch_mode(2)  bloomfilter.h:111-188, main.cpp:148,:193.
 * Runs on the device: canonical k-mers -> XXH64 -> bit set; rank directory;
 * (set bit -> ascending unique gene id list) CSR. */
int shk_ref_finalize(shk_ctx *ctx);

/* THE K-MER KEYED TABLE of a one-gene index (k <= 17).  The reference's answer for a k-mer depends only on its
 * filter position, so the canonical k-mers whose position is a set bit -- the gene's own and the ones that collide with them in the
 * filter -- decide every probe exactly.  shk_ref_finalize enumerates them on the device (all 4^k / 2 canonical k-mers against the
 * index's exact table: tens of milliseconds at k = 17) and builds a second exact table keyed by the k-mer itself, which the
 * classify kernels then probe without XXH64: the same results, a sixth less kernel time.  On by default; shk_ref_kmer_table(ctx, 0)
 * before shk_ref_finalize (SHK_ERR_STATE afterwards) or SHK_NO_KMER_TABLE=1 in the environment leaves it out -- for a context that
 * classifies fewer pairs than repay the enumeration.  Where it does not apply (several genes, k > 17, more keys than the table
 * holds: beyond one gene of about 21 kb at k = 17 and 2^33 bits) nothing is built and nothing changes.  New: no counterpart. */
int shk_ref_kmer_table(shk_ctx *ctx, int on);

typedef struct shk_index_info {
  uint64_t n_records;    /* FASTA records added (= legend_ID.size(), FastaSplitter.hpp:48) */
  uint64_t nidx;         /* final gene counter (main.cpp:191) */
  uint64_t bf_bits;
  uint64_t n_set_bits;   /* num_kmer, bloomfilter.h:122 */
  uint64_t tot_idx;      /* _index_kmer.size(), bloomfilter.h:130-133 */
  uint64_t n_ref_kmers;  /* valid reference k-mer occurrences hashed */
} shk_index_info;
int shk_index_info_get(const shk_ctx *ctx, shk_index_info *info);
/* How the classify kernels look a k-mer's filter position up on this index:
 * "bitvector-mod", "bitvector", "summary+bitvector", "table", "summary+table",
 * "lds-summary+table", "lds-table" (tiny indices: the exact table is held
 * in LDS for batches of one read length; other batches of such an index take
 * lds-summary+table), and for filter sizes that are not a power of two
 * "table-mod", "lds-summary+table-mod"
 * (every mode returns exactly the filter's bit).  Environment
 * SHK_PROBE=bitvector at finalize time disables the table, SHK_TAB_DENSE=1
 * builds it at up to 0.8 load (long probe paths), SHK_NO_LDS_TABLE=1 leaves
 * the LDS-resident table out; all three are for the tests. */
const char *shk_probe_mode(const shk_ctx *ctx);
/* The classify kernel instantiation the LAST batch's main launch ran, as rocprofv3 names it (e.g.
 * "classify_uni_kernel<5, 5, false, 21, true>"; the last argument reads "device" when uniform_check_kernel decided on the
 * device which of the two launched instantiations did the work).  On a panel-sized index the choice depends on the batch
 * before (shk_probe_mode names the index's chains, this names what ran), so a timing or a profile can say what it measured.
 * New: the reference has no counterpart.  The environment's test switches (SHK_FORCE_GENERIC, SHK_BIG_LDS_ALWAYS) are read
 * once, by shk_create.  classify_fast_kernel and classify_general_kernel are named here without their last template argument
 * (evidence mode: "false" in a profile for the ordinary instantiations, which this call leaves out as it always has, "true" for
 * the evidence ones, which this call spells "evidence"): "classify_fast_kernel<5, 3, false>" here is
 * "classify_fast_kernel<5, 3, false, false>" in rocprofv3, "classify_fast_kernel<5, 3, false, evidence>" is "<5, 3, false, true>".
 * Candidates mode (below) added one more trailing template argument the same way: a profile shows the ordinary instantiation as
 * "classify_fast_kernel<5, 3, false, false, false>", the evidence one as "<5, 3, false, true, false>" and the candidates one, which
 * this call spells "classify_fast_kernel<5, 3, false, candidates>" (and "classify_general_kernel<wrap, candidates>"), as
 * "<5, 3, false, true, true>": it computes the evidence record as well. */
const char *shk_last_kernel(const shk_ctx *ctx);

/* Parity introspection: copy the device-resident index to host buffers.
 * words: (bf_bits+63)/64 uint64_t in sdsl::bit_vector layout, bit i =
 * (words[i>>6] >> (i&63)) & 1 (bloomfilter.h:51,:58,:89).
 * offsets[n_set_bits+1] / ids[tot_idx]: list r (the r-th set bit, r = rank)
 * is ids[offsets[r]..offsets[r+1]) -- the explicit form of _bv/_select_bv/
 * _index_kmer (bloomfilter.h:142-167). */
int shk_index_copy_bf(const shk_ctx *ctx, uint64_t *words, uint64_t n_words);
int shk_index_copy_lists(const shk_ctx *ctx, uint32_t *offsets, uint16_t *ids);

/* ---- classification ------------------------------------------------------ */
/* A batch of reads as structure-of-arrays.  Mate 1 of read i is
 * seq1[off1[i] .. off1[i+1]); seq2/off2 NULL => single-end.  qual1/qual2 use
 * the same offsets and may be NULL when min_quality == 0.  The mate join
 * ("N", FastqSplitter.hpp:63) and the quality mask (FastqSplitter.hpp:70,
 * :104-109) are applied ON THE DEVICE; the caller passes raw FASTQ fields. */
typedef struct shk_batch {
  uint64_t        n;
  const char     *seq1;
  const uint64_t *off1;   /* n+1 */
  const char     *seq2;
  const uint64_t *off2;   /* n+1 */
  const char     *qual1;
  const char     *qual2;
} shk_batch;

/* Associations per read: read i belongs to genes
 * gene_ids[gene_off[i] .. gene_off[i+1]) (ascending), the indices the
 * reference passes to legend_ID[] at ReadAnalyzer.hpp:106.  Buffers are owned
 * by the context and stay valid until the next shk_classify* call on it. */
typedef struct shk_result {
  uint64_t        n;
  const uint32_t *gene_off;  /* n+1 */
  const uint16_t *gene_ids;  /* gene_off[n] */
  uint64_t        n_assoc;
} shk_result;

/* ReadAnalyzer::operator()(const vector<elem_t>&, vector<assoc_t>&) const
 * ReadAnalyzer.hpp:39-110 over host buffers (H2D, kernels, D2H): submit + wait of one batch. */
int shk_classify(shk_ctx *ctx, const shk_batch *batch, shk_result *result);

/* The same as a pipeline, for callers that stream batches -- the reference overlaps split / analyze /
 * output across its worker threads (main.cpp:66-77, :219-223); here up to SHK_PIPE_DEPTH batches are in
 * flight per context: while the caller waits for batch i, the H2D copies of batches i+1.. overlap the
 * kernels of batch i on separate HIP streams, and no step in between waits for the host.
 *   submit: reads `batch` (host buffers; pinned memory from shk_alloc_pinned makes the copies truly
 *           asynchronous), enqueues everything and returns a ticket.  The host buffers must stay
 *           untouched until the ticket has been waited for.  SHK_ERR_STATE when SHK_PIPE_DEPTH
 *           tickets are outstanding.
 *   wait  : blocks until that batch is classified and returns its associations in pinned host
 *           buffers owned by the context; they stay valid until SHK_PIPE_DEPTH further submits.
 *           (A ticket of shk_classify_device_submit: device pointers instead.)
 * Tickets must be waited for in the order they were submitted. */
#define SHK_PIPE_DEPTH 3
int shk_classify_submit(shk_ctx *ctx, const shk_batch *batch, uint64_t *ticket);
int shk_classify_wait(shk_ctx *ctx, uint64_t ticket, shk_result *result);

/* Same, for inputs ALREADY RESIDENT IN HBM: every pointer in `batch` is a
 * device pointer; the result pointers returned in `result` are DEVICE
 * pointers owned by the context.  max_read_len is an upper bound on the
 * longest mate (0 = unknown); it only selects the kernel specialisation --
 * reads that do not fit are routed to the general kernel, never dropped.
 * Work is enqueued on the context's stream and the call returns after the
 * stream has drained (one host synchronisation per call when max_read_len is given). */
int shk_classify_device(shk_ctx *ctx, const shk_batch *batch, uint32_t max_read_len, shk_result *result);

/* ... and as a pipeline: the device-resident entry point WITHOUT its host synchronisation (the reference's analyzer threads never
 * wait for the output stage either, main.cpp:66-77).  Everything is enqueued on the context's stream and the call returns a
 * ticket; shk_classify_wait(ticket) then returns DEVICE pointers (as shk_classify_device does), valid until SHK_PIPE_DEPTH
 * further submits.  Tickets of this call and of shk_classify_submit share the context's SHK_PIPE_DEPTH slots and are waited for
 * in submission order.
 *   max_read_len   an upper bound on the longest mate, REQUIRED here (> 0): without one the device would have to be asked
 *                  between two kernels; SHK_ERR_ARG when 0.  A bound that does not hold is noticed and repaired in wait.
 *   uniform_len1/2 when the caller KNOWS that every mate 1 (mate 2) has exactly this length and off1[i] = i * uniform_len1
 *                  (off2 likewise) -- a sequencer's output, generated or copied to the device by the caller itself -- it says so
 *                  here, as the host entry points find out by scanning the offsets: the kernel then never reads an offset and
 *                  the pass that would verify them on the device (61 us per 10 M pairs) is not made.  0, 0: unknown, the
 *                  device looks (as shk_classify_device always does).  The caller vouches for what it states; one thread on
 *                  the device compares three offsets per mate (first, middle, last) with r * length, and shk_classify_wait
 *                  returns SHK_ERR_ARG for a batch whose caller vouched wrongly (no results are handed out). */
int shk_classify_device_submit(shk_ctx *ctx, const shk_batch *batch, uint32_t max_read_len, uint32_t uniform_len1, uint32_t uniform_len2,
                               uint64_t *ticket);

/* ---- evidence: the three numbers a read's decision is made from ------------ */
/* The reference computes, per read, the best gene's coverage `max`, its k-mer count `maxk` and the number of valid characters
 * `len` of the joined and masked string, keeps the genes that reach (max, maxk) if max >= c * len (and, with --single, only a
 * lone one), and throws the three numbers away (ReadAnalyzer.hpp:90-104).  In evidence mode they leave the device with the
 * associations, one record per read (pair) of the batch:
 *   cov, nk   the maximum over ALL genes in the reference's order of comparison (coverage first, then k-mer count), whether or
 *             not it then passes c * len or --single; 0, 0 for a read shorter than k, without a valid k-mer, or without a hit
 *   len       valid characters of the joined string (the joiner 'N', invalid characters and bases masked by -q do not count)
 * so a read has associations at confidence c iff nk > 0 and (double)cov >= c * (double)len (without --single): one run at c = 0
 * answers for every c.  New: the reference has no counterpart beyond the lines named above.
 *
 * The mode has a price: the kernels that are fast because they never compute a read's final coverage (the table kernels' bound
 * cut and early decision, the base-for-base verdict) are not used (how much slower that is: DESIGN.md 6), every k-mer of every read is probed
 * (shk_last_kernel then names the evidence instantiation: "classify_fast_kernel<5, 3, false, evidence>", "classify_general_kernel<wrap, evidence>").  gene_off, gene_ids, n_assoc
 * and shk_gene_counts are the same with the mode on and off; with it off nothing changes at all. */
typedef struct shk_read_evidence { uint32_t cov, nk, len; } shk_read_evidence;
typedef struct shk_evidence {
  uint64_t                 n;       /* records = reads of that batch */
  const shk_read_evidence *reads;
} shk_evidence;
/* Switches evidence mode on (enable != 0) or off for the batches submitted AFTERWARDS, through any of the four families
 * (shk_classify, shk_classify_submit / _wait, shk_classify_device, shk_classify_device_submit).  SHK_ERR_STATE while tickets are
 * outstanding: the batches in flight of one context are all of one kind. */
int shk_evidence_enable(shk_ctx *ctx, int enable);
/* The evidence of the batch whose result was handed out LAST by shk_classify, shk_classify_device or shk_classify_wait: the same
 * lifetime as that result and the same memory space -- pinned host memory owned by the context for host batches, DEVICE memory
 * for resident ones.  (shk_count_work hands out none: SHK_ERR_STATE behind it.)  SHK_ERR_STATE if that batch was submitted with the mode off, if its wait returned an error, or if no batch
 * has been waited for yet. */
int shk_evidence_last(const shk_ctx *ctx, shk_evidence *out);

/* ---- candidates: a read's best genes in the reference's ranking, with their numbers ---- */
/* The reference holds, per read, a map gene -> (coverage, k-mer count) over every gene with at least one hit
 * (ReadAnalyzer.hpp:64-88), picks the entries that reach the maximum (coverage first, then k-mer count; the map's ascending gene
 * order among equals: ReadAnalyzer.hpp:90-102) and throws the rest away.  In candidates mode the first m entries of that map in
 * the order in which :90-102 would pick them if each winner were removed in turn -- cov descending, then nk descending, then gene
 * id ascending -- leave the device with the associations, whether or not the read then passes c * len or --single:
 *   reads[i].len       valid characters of the joined string (ReadAnalyzer.hpp:46-49), as shk_read_evidence.len
 *   reads[i].n_genes   size of the read's map: distinct gene ids with a hit (0 for a read shorter than k, without a valid k-mer or
 *                      without a hit); may exceed m
 *   entries[i*m + r]   the gene of rank r with its coverage and k-mer count; entry 0 is evidence mode's (cov, nk); the leading
 *                      entries that share entry 0's (cov, nk) are, in order, the genes the ordinary result holds when the read
 *                      passes; slots behind the last candidate are empty (all three 0: a candidate has nk >= 1)
 * On an index of more than 65 536 records the entries are the reference's map entries: ids wrapped to 16 bits, cov and nk with the
 * multiplicities of ReadAnalyzer.hpp:56-62, :79-86.  New: the reference has no counterpart beyond the lines named above.
 *
 * The price is evidence mode's (the full-probe kernels run: shk_last_kernel names "classify_fast_kernel<5, 3, false, candidates>",
 * "classify_general_kernel<wrap, candidates>") plus 8 + 12 m bytes stored per read.  gene_off, gene_ids, n_assoc and
 * shk_gene_counts are the same with the mode on and off; with it off nothing changes at all. */
#define SHK_MAX_CANDIDATES 8
typedef struct shk_candidate { uint32_t gene, cov, nk; } shk_candidate;          /* nk == 0: empty slot (all three 0) */
typedef struct shk_read_candidates { uint32_t len, n_genes; } shk_read_candidates;
typedef struct shk_candidates {
  uint64_t                   n;        /* reads of that batch */
  uint32_t                   m;        /* entries per read */
  const shk_read_candidates *reads;    /* n */
  const shk_candidate       *entries;  /* n * m, read i at entries[i*m .. i*m+m), rank order, empty slots last */
} shk_candidates;
/* Switches candidates mode on with m entries per read (1 .. SHK_MAX_CANDIDATES) or off (m = 0) for the batches submitted
 * AFTERWARDS, through any of the four families; SHK_ERR_ARG for m > SHK_MAX_CANDIDATES, SHK_ERR_STATE while tickets are
 * outstanding.  Independent of evidence mode: both may be on, then both _last calls answer and agree.  New: no counterpart. */
int shk_candidates_enable(shk_ctx *ctx, uint32_t m);
/* The candidates of the batch whose result was handed out LAST, with shk_evidence_last's rules: that result's lifetime and memory
 * space (pinned host memory for host batches, DEVICE memory for resident ones); SHK_ERR_STATE if that batch was submitted with the
 * mode off, if its wait returned an error, behind shk_count_work, or if no batch has been waited for yet.  New: no counterpart. */
int shk_candidates_last(const shk_ctx *ctx, shk_candidates *out);

/* ---- placement: where in its gene, and on which strand, an assigned read lies ---- */
/* Per ASSOCIATION (read, gene g) and per mate: the diagonal of g's record that most of the mate's k-mers lie on.  Defined from
 * sequences alone, never through the filter.  The record of g is the FASTA record whose k-mers pass 2 added under id g
 * (main.cpp:160-187, numbering quirk included: at most one record per id); positions are 0-based offsets into its bytes.  A mate
 * is the mate as the classifier sees it -- raw bytes behind the -q mask (FastqSplitter.hpp:70,:104-109), length L counting all
 * bytes, the joiner 'N' belonging to neither mate.  A window of k characters is valid iff all are bases under to_int
 * (kmer_utils.hpp:29-41); f is its k-mer, r the reverse complement (kmer_utils.hpp:47-55), min(f, r) its canonical k-mer and
 * f <= r its orientation bit; a window with f == r takes no part, in the read or in the record.
 *   votes    slot p of the mate (0 <= p <= L - k) votes iff its canonical k-mer is the canonical k-mer of EXACTLY ONE valid window x
 *            of the record (k-mers compared in full; none: no vote; two or more: ambiguous, no vote).  The vote is (strand, pos):
 *            strand = xor of the two orientation bits (0: same direction); pos = x - p for strand 0, x + p + k - L for strand 1 --
 *            either way the record coordinate of the leftmost record base the whole mate would lie on along that diagonal.  pos may
 *            be negative, and pos + L may pass the record's end.
 *   result   the key with the most votes; ties go to strand 0, then to the smaller pos.  support = its votes.  No votes: (0, 0, 0);
 *            mate 2 of a single-end batch: (0, 0, 0).  A read that reached g through filter false positives alone has support 0.
 * Not an alignment: nothing is extended across an indel, which shows as lowered support.  New: the reference has no counterpart.
 *
 * The mode needs a table of its own, (gene, canonical k-mer) -> the unique x and its orientation, or "ambiguous", built on the
 * device by shk_ref_finalize when shk_ref_keep_positions was called before (16 bytes per distinct (gene, k-mer) plus a directory
 * of 4 bytes per bucket).  The classify kernels run unchanged; placement_kernel runs behind them over the reads
 * that received associations.  gene_off, gene_ids, n_assoc, shk_last_kernel and shk_gene_counts are the same with the mode on
 * and off; with it off nothing changes at all, and without shk_ref_keep_positions finalize does exactly what it always did. */
typedef struct shk_mate_placement { int32_t pos; uint32_t support; uint32_t strand; } shk_mate_placement;
typedef struct shk_placement { shk_mate_placement mate[2]; } shk_placement;   /* one per ASSOCIATION, parallel to gene_ids */
typedef struct shk_placements {
  uint64_t             n_assoc;   /* = that result's n_assoc */
  const shk_placement *entries;   /* entries[j] belongs to gene_ids[j] */
} shk_placements;
/* Asks shk_ref_finalize to build the placement table as well.  Before shk_ref_finalize only; SHK_ERR_STATE afterwards.  Finalize
 * then returns SHK_ERR_INDEX_TOO_LARGE for what the table cannot represent: a record of >= 2^31 bases, a reference of >= 2^32
 * bases in all, or more than 2^30 distinct (gene, canonical k-mer) pairs.  New: no counterpart. */
int shk_ref_keep_positions(shk_ctx *ctx);
/* Switches placement mode on (enable != 0) or off for the batches submitted AFTERWARDS, through any of the four families.
 * Switching it on returns SHK_ERR_STATE before shk_ref_finalize, on an index finalized without shk_ref_keep_positions, on an index
 * of more than 65 536 records (ids wrap there and name several records) and, either way, while tickets are outstanding.
 * Independent of evidence and candidates mode: all three may be on at once.  New: no counterpart. */
int shk_placement_enable(shk_ctx *ctx, int enable);
/* The placements of the batch whose result was handed out LAST, with shk_evidence_last's rules: that result's lifetime and memory
 * space (pinned host memory for host batches, DEVICE memory for resident ones); computed from the final gene_off / gene_ids,
 * whichever path produced them (batches repaired in shk_classify_wait included).  SHK_ERR_STATE if that batch was submitted with
 * the mode off, if its wait returned an error, behind shk_count_work, or if no batch has been waited for yet.  New: no counterpart. */
int shk_placement_last(const shk_ctx *ctx, shk_placements *out);

/* ---- segments: the several diagonals of its gene's record a mate lies on, and the slots that say so ---- */
/* The references are gene loci -- genomic sequence, introns included -- and the reads are RNA-Seq: a mate that crosses an exon
 * junction lies on two or more diagonals of its gene's record, an intron apart.  Placement (above) keeps the diagonal with the
 * most votes; segments mode hands out the best m of them.  It rests on placement's definitions, unchanged: mate, L, window, vote
 * and key (strand, pos).
 *
 * Per ASSOCIATION (read, gene g) and per mate let K be the set of distinct keys that received at least one vote.  Per key:
 *   support   its votes
 *   first     the smallest slot p that voted for it
 *   last      the largest slot p that voted for it (first <= last <= L - k; votes need not be contiguous in between)
 * The keys are ranked by support descending, then strand 0 first, then the smaller pos -- placement's tie rule, so rank 0 is
 * exactly the mate's shk_mate_placement.  With m entries per mate (1 <= m <= SHK_MAX_SEGMENTS) the first m ranks leave the device
 * together with n_keys = |K|, which may exceed m.  Slots behind the last key are empty (all five words 0: a segment has
 * support >= 1).  No votes, a mate shorter than k, mate 2 of a single-end batch: n_keys = 0 and m empty slots.  Nothing is
 * filtered on the device by strand or by a support floor: that is the consumer's choice.  Integers, no tolerance anywhere.
 *
 * Junctions are a pure function of the segments, computed by the consumer (shark --junctions, shark_amd.capi.junctions).  The
 * record span [lo, hi) of a segment is the union of the record windows its first and last voting slots lie on:
 *   strand 0: lo = pos + first,         hi = pos + last + k
 *   strand 1: lo = pos + L - k - last,  hi = pos + L - first
 * For one mate and a support floor s_min:
 *   1. take its reported segments with support >= s_min and rank 0's strand (rank 0 itself included only if it reaches s_min);
 *   2. sort them by (lo, hi);
 *   3. every consecutive pair (A, B) with pos_B > pos_A is a junction
 *        (g, donor = hi_A, acceptor = lo_B, intron = pos_B - pos_A, overlap = hi_A + intron - lo_B).
 * overlap is signed: positive, read bases that both sides explain (microhomology at the junction: the breakpoint lies anywhere in
 * it); negative, read bases that neither side explains (a substitution within k of the junction silences the windows over it).
 * A table of junctions over many mates is keyed by (g, donor, acceptor) and counts the mates that show each; where mates disagree on
 * the intron of one key (an indel in a read next to the junction moves its second diagonal) the key carries the smallest intron.
 * Example (L = 100, k = 17): strand 1, pos 9653, slots 26..83 and strand 1, pos 10843, slots 0..14 give spans [9653, 9727) and
 * [10912, 10943): donor 9727, acceptor 10912, intron 1190, overlap 5.
 *
 * The mode needs placement's table (shk_ref_keep_positions) and nothing else of placement mode: segments_kernel runs behind the
 * classify kernels over the reads that received associations, from the final gene_off / gene_ids whichever path produced them
 * (batches repaired in shk_classify_wait included), and stores 8 + 40 m bytes per association.  Independent of evidence,
 * candidates, placement and depth mode: all may be on at once, then entry 0 equals shk_placement_last's record.  gene_off,
 * gene_ids, n_assoc, shk_last_kernel, shk_gene_counts and the other modes' records are the same with the mode on and off; with it
 * off no launch and no allocation is added.  New: the reference has no counterpart. */
#define SHK_MAX_SEGMENTS 4
typedef struct shk_segment { int32_t pos; uint32_t support, strand, first, last; } shk_segment;   /* support == 0: empty slot (all five 0) */
typedef struct shk_segments {
  uint64_t           n_assoc;  /* = that result's n_assoc */
  uint32_t           m;        /* entries per mate */
  const uint32_t    *n_keys;   /* n_assoc * 2:     [j*2 + mate],          j parallel to gene_ids */
  const shk_segment *entries;  /* n_assoc * 2 * m: [(j*2 + mate)*m + r],  rank order, empty slots last */
} shk_segments;
/* Switches segments mode on with m entries per mate (1 .. SHK_MAX_SEGMENTS) or off (m = 0) for the batches submitted AFTERWARDS,
 * through any of the four families.  SHK_ERR_ARG for m > SHK_MAX_SEGMENTS.  Switching it on returns SHK_ERR_STATE where
 * shk_placement_enable(ctx, 1) does: before shk_ref_finalize, on an index finalized without shk_ref_keep_positions, on an index of
 * more than 65 536 records; either way while tickets are outstanding.  New: no counterpart. */
int shk_segments_enable(shk_ctx *ctx, uint32_t m);
/* The segments of the batch whose result was handed out LAST, with shk_placement_last's rules: that result's lifetime and memory
 * space (pinned host memory for host batches, DEVICE memory for resident ones).  SHK_ERR_STATE if that batch was submitted with
 * the mode off, if its wait returned an error, behind shk_count_work, or if no batch has been waited for yet.  New: no counterpart. */
int shk_segments_last(const shk_ctx *ctx, shk_segments *out);

/* ---- depth: per-base read depth along each gene, accumulated on the device over all batches ---- */
/* Rests on placement (above) and inherits its definitions of mate, L, pos, strand and support.  For every association j = (read i,
 * gene g) of a COUNTED batch and for each mate m of it whose placement has support >= min_support (min_support >= 1), the mate
 * covers the record coordinates [pos, pos + L) n [0, len_g): L the mate's length in bytes, every byte counting; len_g the length
 * in bytes of the FASTA record that pass 2 numbered g (main.cpp:160-187; an id without a record -- the numbering quirk -- has
 * len_g = 0).  The strand plays no part: pos is the leftmost record base on either strand.
 *   depth[g][x] = the number of such (association, mate) intervals that contain x, summed over all batches counted since the
 *                 last shk_depth_reset.
 * So: a pair whose mates overlap counts 2 on the overlap (depth counts mates, not fragments); a read tied over several genes
 * counts in each of them; a mate with support 0 never counts (a placement reached through filter false positives alone, mate 2
 * of a single-end batch, a mate shorter than k); an interval that clips to nothing counts nowhere (with support >= 1 at least k
 * bases of the mate lie inside the record, so this does not arise).  Integer arithmetic, no tolerance anywhere.
 *
 * A batch is counted exactly once.  depth_accumulate_kernel runs in the batch's tail behind placement_kernel and skips itself
 * under the conditions under which the per-gene counters (shk_gene_counts) skip: more associations than the result buffer holds,
 * or reads beyond a length bound that was taken on trust -- the batch is then counted when shk_classify_wait / shk_classify_device
 * runs the tail again.  A batch refused in wait is never counted: more than 2^32-1 associations (SHK_ERR_ARG), and a batch of
 * shk_classify_device_submit whose caller vouched wrongly for its read lengths (the accumulation looks at the device's own verdict
 * on the vouched lengths and returns; that path itself is unchanged, the per-gene counters of such a batch are what they always
 * were).  shk_count_work is a measurement: its batch is not counted.
 *
 * The state is a difference array on the device, 4 bytes per base of the records that carry an id plus one entry (two atomic adds
 * per counted mate: +1 at the interval's start, -1 at its end), and a 64-bit counter of counted mates; a read-out scans it into a
 * second array of that size (allocated by the first read-out) and leaves the state as it is, so accumulation can go on.  Counters
 * are 32 bits wide and wrap: once more than 2^31-1 mates have been counted since the last reset, every read-out returns
 * SHK_ERR_INDEX_TOO_LARGE until shk_depth_reset (shk_depth_mates still stores the number).  New: the reference has no counterpart. */
/* Switches depth mode on with this min_support (>= 1), or off (0), for the batches submitted AFTERWARDS, through any of the four
 * families.  Switching it on returns SHK_ERR_STATE where shk_placement_enable(ctx, 1) does: before shk_ref_finalize, on an index
 * finalized without shk_ref_keep_positions, on an index of more than 65 536 records; either way while tickets are outstanding.  The
 * first enable allocates and clears the state; switching off keeps what has been accumulated, switching on again goes on from it.
 * Independent of placement, evidence and candidates mode: with depth on and placement off placement_kernel runs all the same (depth
 * needs its records), shk_placement_last answers SHK_ERR_STATE and no placement is published to pinned memory.  With the mode off
 * no launch and no allocation is added.  New: no counterpart. */
int shk_depth_enable(shk_ctx *ctx, uint32_t min_support);
typedef struct shk_gene_depth {
  uint32_t len;      /* len_g */
  uint32_t covered;  /* number of x with depth >= 1 */
  uint32_t max;      /* the largest depth in the gene */
  uint32_t pad;
  uint64_t sum;      /* sum of depth over the gene = the clipped bases of all counted mates */
} shk_gene_depth;
/* gene_start[0 .. n_genes] (n_genes + 1 entries, n_genes <= nidx of shk_index_info): the depth of gene g lies at
 * [gene_start[g], gene_start[g+1]) of the full array, gene_start[g+1] - gene_start[g] = len_g.  A property of the index, not of
 * the accumulated state: available from shk_ref_finalize on wherever shk_depth_enable can be switched on (SHK_ERR_STATE elsewhere),
 * tickets outstanding or not.  New: no counterpart. */
int shk_depth_layout(const shk_ctx *ctx, uint64_t *gene_start, uint32_t n_genes);
/* The read-outs.  All return SHK_ERR_STATE if the mode was never enabled on this context or while tickets are outstanding, and
 * SHK_ERR_INDEX_TOO_LARGE behind the overflow guard above; otherwise they run on the context's stream behind everything enqueued
 * so far and leave the accumulated state untouched.  The scan is kept until a batch adds to the state or the state is reset: read-outs
 * in a row (gene after gene, or get_all and then the summary) pay for one scan.  New: no counterpart.
 *   shk_depth_get      depth[0 .. len_g) of one gene (gene < nidx) into host memory; cap (entries) must be at least len_g
 *   shk_depth_get_all  the whole array, gene_start[nidx] entries (cap at least that): device == 0: `depth` is a host pointer;
 *                      device != 0: a DEVICE pointer, the copy stays on the device
 *   shk_depth_summary  out[g] for g < n_genes (n_genes <= nidx), host memory
 *   shk_depth_mates    the number of counted mates since the last reset */
int shk_depth_get(shk_ctx *ctx, uint32_t gene, uint32_t *depth, uint64_t cap);
int shk_depth_get_all(shk_ctx *ctx, uint32_t *depth, uint64_t cap, int device);
int shk_depth_summary(shk_ctx *ctx, shk_gene_depth *out, uint32_t n_genes);
int shk_depth_mates(const shk_ctx *ctx, uint64_t *n_mates);
/* Clears the accumulated depth and the mate counter (the mode stays as it is); the read-outs' state rules.  New: no counterpart. */
int shk_depth_reset(shk_ctx *ctx);

/* ---- spliced depth and the junction table: the two consumers of segments mode, on the device ---- */
/* Both rest on the segments section's definitions, unchanged: mate, L, key, support, first, last and the record span [lo, hi) of a
 * segment.  Both consume one thing:
 *
 * KEPT SPANS of a mate at floor s_min (>= 1).  Take the mate's first SHK_MAX_SEGMENTS (4) ranked segments; keep those with
 * support >= s_min and rank 0's strand (rank 0 itself only if it reaches s_min: ranks descend in support, so a rank 0 below the
 * floor keeps nothing); sort the kept ones by (lo, hi), equal spans in rank order.  Steps 1 and 2 of the junction rule above at
 * m = 4, whatever m segments mode itself runs at.  The result may be empty: the mate then contributes nothing anywhere.
 *
 * SPLICED DEPTH.  Depth mode (above) paints [pos, pos + L) along the mate's best diagonal -- straight over the intron of a mate
 * that crosses a junction.  Here a counted mate covers the UNION of its kept spans, clipped to [0, len_g):
 *   - a base counts once per mate, however many of its spans contain it (spans of one mate can overlap in record coordinates:
 *     behind a short deletion, at an insertion in the read, over the microhomology of a junction);
 *   - only explained bases count: nothing is extended to the mate's ends.  An overhang shorter than k past a junction holds no
 *     whole window and cannot vote, so nothing says on which side of the intron it lies; extending the span by it would paint
 *     it into the intron, the very error this mode removes.  A mate's ends behind its outermost voting windows are left out
 *     for the same reason (a substitution there silences up to k windows): spliced depth is a lower bound base by base;
 *   - depth[g][x], the counting of batches and every rule of depth mode are otherwise unchanged: mates are counted, not fragments;
 *     a read tied over several genes counts in each; integers only; a batch is counted exactly once (a batch with more
 *     associations than the result buffer holds or with reads beyond a length bound taken on trust is counted when the tail
 *     runs again; a batch vouched for wrongly and a shk_count_work batch are not counted);
 *   - a mate counts in shk_depth_mates iff it added at least one interval.
 *
 * JUNCTION TABLE.  For every counted mate, every consecutive pair (A, B) of its kept spans with pos_B > pos_A is one OBSERVATION
 * of the key (g, donor = hi_A, acceptor = lo_B) -- step 3 of the junction rule.  Per key the table holds
 *   mates    the observations since the last reset
 *   intron   the smallest pos_B - pos_A among them
 * which is `shark --junctions`' table, accumulated on the device over all counted batches (the same batches as depth's).
 * Example (segments section): the mate with spans [9653, 9727) and [10912, 10943) covers those 74 + 31 bases and none of the 1185
 * between them, and is one observation of (g, 9727, 10912) with intron 1190.
 *
 * State: spliced depth uses depth mode's state.  The table is an open-addressing array of `capacity` 16-byte entries on the device.
 * New: the reference has no counterpart. */
/* As shk_depth_enable, but the intervals of the batches submitted AFTERWARDS are the unions of kept spans at s_min = min_support.
 * The state, its layout and every shk_depth_* read-out and reset are shared with plain depth, and one state holds one kind:
 * switching between plain and spliced (either way) returns SHK_ERR_STATE if a depth batch of the other kind was submitted since
 * the first enable or the last shk_depth_reset (the host keeps a flag; the device is not asked).  shk_depth_enable(ctx, 0) and
 * shk_depth_enable_spliced(ctx, 0) switch either kind off.  placement_kernel does not run for spliced depth (unless placement
 * mode asks for it); segments_kernel does, see below.  New: no counterpart. */
int shk_depth_enable_spliced(shk_ctx *ctx, uint32_t min_support);
/* Switches the junction table on with this min_support (>= 1) or off (0) for the batches submitted AFTERWARDS, through any of the
 * four families.  capacity: table entries, rounded up to a power of two of at least 64; 16 bytes each; the table must hold every
 * distinct key (keep it at most half full for short probe chains).  The first enable allocates and clears the table; a later
 * enable with another capacity returns SHK_ERR_ARG unless no batch was submitted with the mode on since the first enable or the
 * last shk_junctions_reset (the table is then allocated anew).  Switching off (capacity is ignored) keeps the table.  State rules
 * are shk_segments_enable's: switching on returns SHK_ERR_STATE before shk_ref_finalize, without shk_ref_keep_positions, on an
 * index of more than 65 536 records; either way while tickets are outstanding.  New: no counterpart.
 *
 * Both modes are independent of every other mode and of each other.  shk_segments_last hands out exactly what it does without
 * them, at the caller's m.  With segments mode on at m = SHK_MAX_SEGMENTS its one segments_kernel launch serves them too;
 * otherwise segments_kernel runs (once more) at m = 4 into arrays of the context's own, allocated with the first such batch and
 * never handed out.  spliced_accumulate_kernel follows it.  With both off no launch and no allocation is added. */
int shk_junctions_enable(shk_ctx *ctx, uint32_t min_support, uint64_t capacity);
typedef struct shk_junction { uint32_t gene, donor, acceptor, intron; uint64_t mates; } shk_junction;
/* The read-outs, with depth's rules: SHK_ERR_STATE if the mode was never enabled on this context or while tickets are
 * outstanding; stream-ordered behind everything enqueued so far; the table is left untouched.  If any observation found the table
 * full, every read-out returns SHK_ERR_INDEX_TOO_LARGE until shk_junctions_reset (nothing partial is handed out).
 *   shk_junctions_get    *n = the number of distinct keys; out != NULL: the keys sorted by (gene, donor, acceptor) into out[0 .. *n)
 *                        (host memory; SHK_ERR_ARG if cap < *n, *n is set all the same).  out == NULL: only *n
 *   shk_junctions_reset  empties the table (the mode and the capacity stay as they are) */
int shk_junctions_get(shk_ctx *ctx, shk_junction *out, uint64_t cap, uint64_t *n);
int shk_junctions_reset(shk_ctx *ctx);

/* ---- pileup: per record base, how many counted mates show A, C, G or T there -- the third consumer of segments mode ---- */
/* Placement, depth, segments, spliced depth and the junction table say WHERE a mate lies; pileup says what it READS there.  It
 * rests on definitions this header already has, unchanged: the mate as the classifier sees it (its raw bytes behind the -q mask:
 * a byte whose quality is below min_quality is the byte minus 64), L, segment, record span [lo, hi), and the KEPT SPANS of a mate
 * at floor s_min (the first four ranked segments with support >= s_min on rank 0's strand, sorted by (lo, hi), equal spans in
 * rank order).
 *
 * OWNERSHIP.  For every association (read, gene g) of a COUNTED batch and each mate of it, walk the kept spans in sorted order
 * with spliced depth's `reach`, 0 at first:
 *     span r owns the record coordinates [max(lo_r, reach), min(hi_r, len_g));   then reach = max(reach, hi_r).
 * A record base is therefore owned by at most one span of a mate -- the earliest in sorted order that contains it --, and the owned
 * pieces are exactly the pieces spliced depth adds.
 *
 * OBSERVATION.  An owned coordinate x on the diagonal (strand, pos) of its span reads one byte of the mate, at index
 *     strand 0: i = x - pos;        strand 1: i = pos + L - 1 - x.
 * A span lies inside [pos, pos + L) (first <= last <= L - k), so 0 <= i < L: every owned coordinate has its byte.  Let
 * c = to_int[byte] (kmer_utils.hpp:29-41: A, C, G, T and their lower case are 1 .. 4, every other byte 0).
 *     c == 0 (an N, any other non-base, a byte masked by -q): the base makes NO observation;
 *     otherwise the observed base ON THE RECORD'S STRAND is b = c - 1 on strand 0 and b = 3 - (c - 1) on strand 1: with the codes
 *     A, C, G, T = 0 .. 3 that is the complement (the fact reverse_char states).
 *   counts[g][x][b] = the number of observations of b at x, summed over all batches counted since the last shk_pileup_reset.
 * A mate is a PILEUP MATE iff it owned at least one coordinate (spliced depth's rule for shk_depth_mates), whatever its bytes there.
 * Example (segments section): the mate with spans [9653, 9727) and [10912, 10943) on strand 1 makes 74 + 31 observations (if all
 * its bytes there are bases) and none at the 1185 bases between them.
 *
 * Consequences:
 *   - a base counts at most once per mate, so every counter is at most the number of pileup mates; a 64-bit device counter of
 *     pileup mates guards the 32-bit counters: beyond 2^32 - 1 pileup mates since the last reset every read-out returns
 *     SHK_ERR_INDEX_TOO_LARGE until shk_pileup_reset (shk_pileup_mates still stores the number);
 *   - with the same s_min over the same batches,
 *         sum_b counts[g][x][b] + (observations lost to c == 0 at x) == spliced depth[g][x]:
 *     equality where no read byte is a non-base, and never more;
 *   - nothing is compared with the reference sequence and the device does not keep it: the caller holds the FASTA, the reference
 *     allele is the caller's to look up (unless shk_ref_keep_bases was asked for: the variants section below);
 *   - a read tied over several genes counts in each of them; mates are counted, not fragments;
 *   - a batch is counted exactly once, by depth mode's rules word for word: a batch with more associations than the result buffer
 *     holds, or with reads beyond a length bound taken on trust, is counted when the tail runs again (shk_classify_wait /
 *     shk_classify_device); a batch vouched for wrongly and a shk_count_work batch are never counted;
 *   - integers only, no tolerance anywhere.
 *
 * State: uint32 counts[gene_start[nidx]][4] on the device, interleaved -- entry [x * 4 + b] of gene g at (gene_start[g] + x) * 4 + b,
 * shk_depth_layout's gene_start, which answers wherever this mode can be switched on --, 16 bytes per record base (four times
 * depth's), and the 64-bit counter.  The counters are the answer: a read-out is one copy, no scan.
 *
 * Independent of every other mode: gene_off, gene_ids, n_assoc, shk_last_kernel, shk_gene_counts and every other mode's records
 * and state are the same with the mode on and off.  With segments mode on at m = SHK_MAX_SEGMENTS its one segments_kernel launch
 * serves pileup too; otherwise segments_kernel runs at m = 4 into the arrays of the context's own that spliced depth and the
 * junction table use (one launch serves all three).  pileup_kernel follows.  With the mode off no launch and no allocation is
 * added.  New: the reference has no counterpart. */
/* Switches pileup mode on with s_min = min_support (>= 1) or off (0) for the batches submitted AFTERWARDS, through any of the four
 * families.  State rules are shk_junctions_enable's: switching on returns SHK_ERR_STATE before shk_ref_finalize, without
 * shk_ref_keep_positions, on an index of more than 65 536 records; either way while tickets are outstanding.  The first enable
 * allocates and clears the state (SHK_ERR_NOMEM if it cannot: the mode is left off); switching off keeps what has been accumulated,
 * switching on again goes on from it.  New: no counterpart. */
int shk_pileup_enable(shk_ctx *ctx, uint32_t min_support);
/* ALIGNED PILEUP: as shk_pileup_enable, but the batches submitted AFTERWARDS count what alignments mode shows instead of the owned
 * pieces.  With s_min = min_support, every base of every FINAL BLOCK of the alignments section -- after trimming, gap closure and,
 * at the context's current shk_alignments_extend parameters, end extension -- makes one observation at its record coordinate under
 * the OBSERVATION rule above: read base q + t of block {x, q, len} at x + t; c == 0 makes none; the base is complemented on strand
 * 1.  A mate is a pileup mate iff n_blocks >= 1.  Blocks are disjoint in the read, so a read base is observed at most once (owned
 * pileup observes the microhomology of a junction twice and the bases gap closure places not at all), and sum_b counts over the
 * state equals the number of base-bearing block bases.  The record base is not consulted: an observation needs no r < 4.
 * The state, its layout, the read-outs, shk_pileup_add, shk_variants_* and the mate guard are pileup's own, and ONE STATE HOLDS ONE
 * KIND: switching between owned and aligned (either way) returns SHK_ERR_STATE if a pileup batch of the other kind was submitted
 * since the first enable or the last shk_pileup_reset (the host keeps a flag; the device is not asked).  shk_pileup_enable(ctx, 0)
 * and shk_pileup_enable_aligned(ctx, 0) switch either kind off.  Switching on additionally returns SHK_ERR_STATE on an index
 * finalized without shk_ref_keep_bases (the walk is alignments mode's and closes gaps against the record).  A batch is counted
 * exactly once by pileup's rules word for word.  pileup_kernel does not run: align_kernel's accumulating instantiation does, with
 * alignments mode off too (no records are stored or allocated then); with alignments mode on at the same floor one launch does
 * both, at another floor each has its own.  New: no counterpart. */
int shk_pileup_enable_aligned(shk_ctx *ctx, uint32_t min_support);
/* The read-outs, with depth's rules: SHK_ERR_STATE if the mode was never enabled on this context or while tickets are outstanding,
 * SHK_ERR_INDEX_TOO_LARGE behind the guard above; otherwise they run on the context's stream behind everything enqueued so far and
 * leave the state untouched.  New: no counterpart.
 *   shk_pileup_get      the 4 * len_g entries [x * 4 + b] of one gene (gene < nidx) into host memory; cap (entries) at least that
 *   shk_pileup_get_all  all 4 * gene_start[nidx] entries (cap at least that): device == 0: `counts` is a host pointer; device != 0:
 *                       a DEVICE pointer, the copy stays on the device
 *   shk_pileup_mates    the pileup mates since the last reset
 *   shk_pileup_reset    clears the counters and the mate counter (the mode stays as it is) */
int shk_pileup_get(shk_ctx *ctx, uint32_t gene, uint32_t *counts, uint64_t cap);
int shk_pileup_get_all(shk_ctx *ctx, uint32_t *counts, uint64_t cap, int device);
int shk_pileup_mates(const shk_ctx *ctx, uint64_t *n);
int shk_pileup_reset(shk_ctx *ctx);
/* Adds an array in the pileup layout, element by element (modulo 2^32), to the context's pileup state and `mates` to the 64-bit
 * counter of pileup mates: what sums the states of N workers or N ranks (a variant call, below, is not linear in the counters, so
 * the states are summed BEFORE the call), and what loads a hand-made state.  device == 0: `counts` is a host pointer; device != 0: a
 * DEVICE pointer, 16-byte aligned.  n_entries must be 4 * gene_start[nidx] (SHK_ERR_ARG otherwise; SHK_ERR_ARG for counts == NULL
 * with entries to add and for a device pointer that is not aligned).  The caller vouches that no counter in `counts` exceeds `mates` -- true of every state this library accumulated --; it is
 * not checked, and with it the guard of the mate counter (2^32 - 1) keeps guarding the 32-bit counters behind the call.
 * shk_pileup_reset's state rules: SHK_ERR_STATE if the mode was never enabled on this context or while tickets are outstanding; the
 * mode may be on or off.  Runs on the context's stream behind everything enqueued so far and returns when it is done.  New: no
 * counterpart. */
int shk_pileup_add(shk_ctx *ctx, const uint32_t *counts, uint64_t n_entries, uint64_t mates, int device);

/* ---- variants: the record positions where the pileup shows another base than the record -- pileup's read-out against the reference ---- */
/* Pileup (above) counts what the mates read at every record base; variants mode holds that against the record itself, on the
 * device, and hands out the positions that differ.  It adds nothing to a batch: the state is pileup's, the call is a read-out.
 *
 * RECORD BASES.  shk_ref_keep_bases asks shk_ref_finalize to keep the records' bases on the device: one byte per record base in
 * shk_depth_layout's order -- base x of gene g at gene_start[g] + x, the records that carry an id and no others -- holding
 * r = to_int[byte] - 1 (kmer_utils.hpp:29-41): A, C, G, T and their lower case are 0 .. 3, every other byte is 4.
 *
 * THE CALL.  For record base x of gene g let n[b] = counts[g][x][b] (b = 0 .. 3 = A, C, G, T), T = n[0] + n[1] + n[2] + n[3] as a
 * 64-bit sum, and r the record's base there.
 *   - a position with r == 4 takes no part in anything below: it is no site and adds to no sum;
 *   - otherwise alt is the b != r with the largest n[b]; ties go to the smallest b;
 *   - x is a SITE iff all three hold:
 *         T >= min_depth,     n[alt] >= min_alt,     (uint64) n[alt] * frac_den >= (uint64) frac_num * T
 *     (the allele fraction n[alt] / T is at least frac_num / frac_den, compared without a division).
 * Parameters: min_depth >= 1, min_alt >= 1, 1 <= frac_den <= 65535, frac_num <= frac_den; anything else is SHK_ERR_ARG.  Within
 * these bounds both products stay below 2^51.  Integers only, no tolerance anywhere.
 * Per gene, over its positions with r < 4:
 *   observed     sum of T
 *   mismatches   sum of (T - n[r]): the observations that differ from the record
 *   covered      the number of x with T >= min_depth
 *   sites        the number of sites
 * mismatches / observed is the gene's error rate: what a site's allele fraction is held against to tell a variant from noise.  (The
 * two sums are 64 bits wide and wrap; a state this library accumulated stays far below that.)
 * Example: r = A, n = (12, 0, 5, 0), defaults of the command (depth 8, alt 3, frac 1/5): T = 17, alt = G, 5 * 5 >= 1 * 17: a site
 * {ref 0, alt 2}.  With n = (14, 0, 3, 0): 3 * 5 = 15 < 17: none.
 *
 * Kernels (variants.hip): two streaming passes over the state (16 bytes per base) and the record bases (1 byte per base) -- count
 * the sites per wavefront, scan the counts, write the records at their final places, so the order is (gene, x) without a sort --
 * and one pass for the summary.  Scratch memory is allocated by the first call, kept, and only grows.  New: no counterpart. */
/* Asks shk_ref_finalize to keep the record bases as well.  Implies shk_ref_keep_positions (the array only exists where gene_start
 * does).  Before shk_ref_finalize only; SHK_ERR_STATE afterwards.  Costs one byte per record base; without the call finalize does
 * exactly what it did: no allocation, no launch.  New: no counterpart. */
int shk_ref_keep_bases(shk_ctx *ctx);
typedef struct shk_variant_params { uint32_t min_depth, min_alt, frac_num, frac_den; } shk_variant_params;
typedef struct shk_variant { uint32_t gene, x, ref, alt, n[4]; } shk_variant;            /* 32 bytes; ref, alt: 0 .. 3 = A, C, G, T */
typedef struct shk_gene_variants { uint64_t observed, mismatches; uint32_t covered, sites; } shk_gene_variants;
/* The read-outs.  SHK_ERR_STATE if pileup mode was never enabled on this context, if the index was finalized without
 * shk_ref_keep_bases, or while tickets are outstanding; SHK_ERR_INDEX_TOO_LARGE behind pileup's mate guard; SHK_ERR_ARG for
 * parameters outside the bounds above.  Both run on the context's stream behind everything enqueued so far and leave the pileup
 * state untouched, so accumulation can go on.
 *   shk_variants_get      *n = the number of sites; out != NULL: the sites sorted by (gene, x) into out[0 .. *n) (host memory;
 *                         SHK_ERR_ARG if cap < *n, *n is set all the same).  out == NULL: only *n (shk_junctions_get's conventions)
 *   shk_variants_summary  out[g] for g < n_genes (n_genes <= nidx), host memory */
int shk_variants_get(shk_ctx *ctx, const shk_variant_params *p, shk_variant *out, uint64_t cap, uint64_t *n);
int shk_variants_summary(shk_ctx *ctx, const shk_variant_params *p, shk_gene_variants *out, uint32_t n_genes);

/* ---- alignments: each placed mate's gapped alignment to its gene's record -- the per-read product, the fourth consumer of segments mode ---- */
/* Depth, the junction table, pileup and variants hand out aggregates; alignments mode hands out, per ASSOCIATION (read, gene g) and per
 * mate, where the mate's bases lie on g's record: at most SHK_MAX_SEGMENTS gap-free BLOCKS, and how many of their bases agree with the
 * record.  It rests on definitions this header already has, unchanged: mate, L, the -q mask, to_int, segment, record span [lo, hi), the
 * KEPT SPANS of a mate at floor s_min, pileup's OWNERSHIP walk with `reach`, len_g, and the record's code r of shk_ref_keep_bases
 * (0 .. 3, every other byte 4).  Everything below is per association and per mate.
 *
 * READ COORDINATE.  q = x - pos is the index of the read base under record coordinate x on the diagonal (strand, pos), counted in the
 * record's orientation on either strand: on strand 0 the mate's byte q, on strand 1 its byte L - 1 - q, complemented (pileup's two
 * index formulas read as one).  A block {x, q, len} says: read bases q .. q + len - 1 lie on record bases x .. x + len - 1.
 *
 * 1. PIECES.  Pileup's owned pieces [a_r, b_r) = [max(lo_r, reach), min(hi_r, len_g)) of the kept spans in sorted order, word for
 *    word; empty ones are dropped.  They ascend and are disjoint in x.
 * 2. TRIMMING.  Consecutive pieces can overlap in the READ (microhomology at a junction: overlap > 0).  Walk the pieces with a read
 *    cursor c, 0 at first:  t = max(0, c - (a_r - pos_r)),  a' = a_r + t.  If a' >= b_r the piece yields no block (and c stays);
 *    otherwise it yields the block {x = a', q = a' - pos_r, len = b_r - a'} and c = q + len.  The left side keeps the shared read
 *    bases.  The blocks ascend and are disjoint in both x and q; the first piece always yields a block.
 * 3. GAP CLOSURE.  Between consecutive blocks A and B let R = q_B - (q_A + len_A), the read bases neither explains, and
 *    G = x_B - (x_A + len_A).  Closure applies iff 1 <= R <= 64 and G >= R (typically a substitution within k of a junction, which
 *    silenced the windows over it).  For every split s in 0 .. R the read bases q_A + len_A + t with t < s go on A's diagonal, at
 *    record x_A + len_A + t, and the remaining R - s on B's diagonal, at the record bases directly left of x_B (read base
 *    q_A + len_A + t at x_B - R + t).  cost(s) = the number of those R bases that are NOT A MATCH (step 4).  Take the s of smallest
 *    cost, ties to the LARGEST s; then  len_A += s;  x_B -= R - s;  q_B -= R - s;  len_B += R - s.  G >= R keeps the record
 *    intervals disjoint and inside [0, len_g).  A gap consumes only its own bases, so the gaps are independent of each other.  Every
 *    other gap stays open: R > 64, or G < R (an insertion in the read).
 * 3a. END EXTENSION (shk_alignments_extend; off by default), after gap closure, on a mate with n_blocks >= 1, with mismatch penalty
 *    P (1 .. 15) and end bonus B (0 .. 15).  K-mers are blind outside the outermost voting windows: a substitution at read index
 *    i < k or i >= L - k silences every window on its outer side, and the span, the owned piece and the block all stop short of it.
 *    This step compares the overhang with the record base by base, with step 4's kinds: a match scores +1, a mismatch -P, a base that
 *    is neither 0.
 *      RIGHT END.  The last block ends at (xe, qe) = (x + len, q + len); H = min(L - qe, len_g - xe).  Overhang base t = 0 .. H - 1 is
 *      read base qe + t on record base xe + t.  score(e) = the sum over t < e, plus B iff qe + e == L and e >= 1 (the extension
 *      reaches the mate's end, not merely the record's).  Take the e in 0 .. H of largest score, ties to the SMALLEST e; len += e.
 *      LEFT END.  The mirror image on block 0 = {x0, q0, len}: H = min(q0, x0), base t is read base q0 - 1 - t on record base
 *      x0 - 1 - t, the bonus applies iff e == q0 and e >= 1; then x0 -= e, q0 -= e, len += e.
 *    With one block the left end is done first and then the right; the two are independent.  Interior gaps are untouched, step 4
 *    counts over the extended blocks, and the record stays consistent (blocks inside [0, len_g) and [0, L), ascending, disjoint):
 *    shk_alignment_cigar takes it as it is.  Consequences:
 *      - an isolated substitution at distance d (counted from 0) from the block in an overhang of h bases that otherwise matches up
 *        to the mate's end is extended through iff the whole overhang scores more than its first d bases: h - 1 - P + B > d (at
 *        d = 0, next to the block: h - 1 - P + B > 0).  With the command's P = 4, B = 5 that always holds (h - 1 - 4 + 5 = h > d);
 *      - an overhang into unrelated sequence (an intron behind a junction) keeps only its matching prefix: the expected score per
 *        base is 0.25 - 0.75 P < 0, and no bonus waits at the record's end;
 *      - trailing bases that are neither are not taken (ties go to the smallest e) unless the bonus carries the extension to the end;
 *      - with P = 0 the step is off and the records are bit-identical to those without it.
 * 3b. SPLICED ENDS (shk_splice_sites_set, shk_alignments_splice; off by default), after gap closure and BEFORE step 3a, on a mate with
 *    n_blocks >= 1, with the context's list of SITES and min_overhang (1 .. SHK_SPLICE_MAX_OVERHANG), max_cost and min_gap (0 .. 64).
 *    A site (d, a) of gene g says: record bases [d, a) of g are an intron.  A side of a junction becomes a kept span only where it
 *    holds s_min unique k-mers, at least k + s_min - 1 read bases; a shorter overhang past a junction is silent and stays outside
 *    every block.  This step tries such an end across every listed intron it could have crossed and keeps the placement where it is
 *    good and clearly the best.  "Not a match" is step 4's kind, as in a split's cost: a read byte that is no base or is masked, and
 *    a record code 4, are not a match.
 *      RIGHT END.  The last block is A = {x, q, len}; (xe, qe) = (x + len, q + len), h = L - qe.  The end is ATTEMPTED iff
 *      min_overhang <= h <= SHK_SPLICE_MAX_OVERHANG and the mate has at most 3 blocks at that moment.  B = min(SHK_SPLICE_BACK,
 *      len - 1).  The EVALUATED read bases are p = qe - B .. L - 1 (B + h <= 64 of them); on A's diagonal base p lies on record base
 *      xA(p) = xe + (p - qe).  A site (d, a) of the gene is a CANDIDATE iff
 *          xe - B <= d <= xe + h - 1      (A keeps at least one base and at least one base crosses),
 *          a + (xe + h - d) <= len_g      (the far side lies inside the record),
 *      and d < a, which every listed site satisfies.  Under the candidate base p lies on xA(p) if xA(p) < d, else on xA(p) + (a - d);
 *      cost(d, a) = the number of evaluated bases that are not a match there.  The NULL candidate leaves every evaluated base on
 *      xA(p) (a coordinate at or beyond len_g is not a match); its shift is 0, a site's SHIFT is a - d >= 1.
 *        best   the candidate of smallest cost, ties to the LARGEST d, then the largest a (the left block keeps the shared bases,
 *               as trimming and closure rule);
 *        cost2  the smallest cost over the null candidate and all candidates whose shift differs from best's.  (Two sites of one
 *               shift describe the same placement up to where the bases between their donors lie -- the junction table produces
 *               such pairs from mates with an error next to a junction --, and they must not make each other ambiguous.)
 *      The end is PLACED iff a candidate exists, cost(best) <= max_cost and cost2 - cost(best) >= min_gap (as signed numbers).
 *      Placing:  len_A += d - xe (which may be negative), and the block {a, qe + (d - xe), h - (d - xe)} is added behind A: it ends
 *      at the mate's last base.
 *      LEFT END.  The mirror image on block 0 = {x0, q0, len}: h = q0 under the same bounds, B = min(SHK_SPLICE_BACK, len - 1), the
 *      evaluated bases are p = 0 .. q0 + B - 1 with xB(p) = x0 + (p - q0).  A site is a candidate iff
 *          x0 - h + 1 <= a <= x0 + B,     d - (q0 - x0 + a) >= 0      (the new block starts inside the record).
 *      Base p lies on xB(p) if xB(p) >= a, else on xB(p) - (a - d).  Null candidate, tie rule (largest d, then largest a), cost2 and
 *      the three conditions are the right end's.  Placing adds the block {d - n, 0, n} with n = q0 - x0 + a in front of block 0, and
 *      block 0 becomes {a, n, len - (a - x0)}.
 *    The left end is done first, then the right; the right end's B and its count of blocks are those after the left.  A mate ends
 *    with at most SHK_MAX_SEGMENTS blocks.  Step 3a runs afterwards: it finds H = 0 at a placed end and treats an unplaced end as
 *    before; step 4 counts over the final blocks.  Example (k = 17, exons [0, 80) and [140, 220), site (80, 140)): the mate
 *    s[20:80] + s[140:150] has the block {20, 0, 60} and h = 10; with the site it becomes {20, 0, 60}, {140, 60, 10}: 60M60N10M.
 *    What the step does NOT do: an overhang that itself holds a second junction; an overhang longer than SHK_SPLICE_MAX_OVERHANG
 *    bases; a mate with no block; sites learned within the run.  Depth, spliced depth and the junction table accumulate from the
 *    spans in front of align_kernel and do not see a placed overhang.
 * 4. COUNTING, over the final blocks.  For the read byte's c = to_int[byte behind the -q mask] and the record's code r at a block base:
 *    c == 0 or r == 4: neither a match nor a mismatch; otherwise b = c - 1 on strand 0 and 3 - (c - 1) on strand 1, and b == r is a
 *    match, anything else a mismatch.  (For a split's cost a base that is neither counts as not a match.)
 * 5. RECORD.  shk_mate_alignment, 64 bytes per mate, 128 per association, parallel to gene_ids: n_blocks, strand (rank 0's), matches,
 *    mismatches, and the blocks in ascending order; unused blocks are zero.  A mate without a block -- no kept span: support below
 *    s_min, a mate shorter than k, mate 2 of a single-end batch -- is all zero.
 * Example (segments section; L = 100, k = 17): strand 1, spans [9653, 9727) at pos 9653 and [10912, 10943) at pos 10843.  Blocks
 * {9653, 0, 74} and, trimmed by the overlap of 5, {10917, 74, 26}: R = 0, nothing is clipped, and the gap is G = 1190 record bases;
 * at min_intron <= 1190 the text form is 74M1190N26M.
 *
 * What the mode does NOT do:
 *   - by default the mate's ends outside its outermost blocks are not extended: they become soft clips (step 3a extends them base
 *     by base where shk_alignments_extend asks for it; an overhang past a junction stays a clip unless step 3b places it across a
 *     LISTED junction: the mode does not discover the other side of an intron by itself);
 *   - the records themselves make no pair-level claim and carry no mapping quality: orientation, template length, the proper-pair
 *     flag and MAPQ are pairs mode's (the next section), which reads these records and changes none of them.
 *
 * Independent of every other mode: gene_off, gene_ids, n_assoc, shk_last_kernel, shk_gene_counts and every other mode's records and
 * state are the same with the mode on and off.  It reads segments_kernel's records at m = SHK_MAX_SEGMENTS as spliced depth, the
 * junction table and pileup do (one launch of that kernel serves all four); align_kernel follows pileup_kernel in the batch's tail,
 * from the final gene_off / gene_ids whichever path produced them (batches repaired in shk_classify_wait included).  With the mode
 * off no launch and no allocation is added.  Integers only, no tolerance anywhere.  New: the reference has no counterpart. */
typedef struct shk_mate_alignment {
  uint32_t n_blocks, strand, matches, mismatches;
  struct { uint32_t x, q, len; } block[4];     /* SHK_MAX_SEGMENTS of them */
} shk_mate_alignment;                          /* 64 bytes */
typedef struct shk_alignments {
  uint64_t                  n_assoc;           /* = that result's n_assoc */
  const shk_mate_alignment *entries;           /* n_assoc * 2: [j*2 + mate], j parallel to gene_ids */
} shk_alignments;
/* Switches alignments mode on with s_min = min_support (>= 1) or off (0) for the batches submitted AFTERWARDS, through any of the four
 * families.  State rules are shk_pileup_enable's: switching on returns SHK_ERR_STATE before shk_ref_finalize, without
 * shk_ref_keep_positions, on an index of more than 65 536 records; either way while tickets are outstanding.  Switching on also
 * returns SHK_ERR_STATE on an index finalized without shk_ref_keep_bases.  New: no counterpart. */
int shk_alignments_enable(shk_ctx *ctx, uint32_t min_support);
/* Step 3a's parameters for the batches submitted AFTERWARDS: mismatch_penalty P = 0 switches the step off (the default), 1 .. 15
 * on; end_bonus B = 0 .. 15; anything else is SHK_ERR_ARG.  SHK_ERR_STATE while tickets are outstanding.  Needs no index and may
 * be called before shk_ref_finalize; it takes effect only where alignments mode or aligned pileup (shk_pileup_enable_aligned) runs.
 * The command's --extend-ends is P = 4, B = 5: the familiar match 1 / mismatch 4 / clip 5.  With P = 0 the kernel launched is the
 * one that ran before this call existed.  New: no counterpart. */
int shk_alignments_extend(shk_ctx *ctx, uint32_t mismatch_penalty, uint32_t end_bonus);
/* Step 3b's site list: copies sites[0 .. n) to the device (the caller's array is free afterwards) and replaces an earlier list; n == 0
 * drops the list and switches the step off.  The intron of a site is record bases [donor, acceptor) of gene.  SHK_ERR_STATE before
 * shk_ref_finalize, without shk_ref_keep_positions, on an index of more than 65 536 records, and while tickets are outstanding;
 * SHK_ERR_ARG unless n < 2^31 and the list is strictly ascending in (gene, donor, acceptor) with gene < n_records and
 * 1 <= donor < acceptor <= len_g - 1.  On the device: one offset per gene, the sites in (donor, acceptor) order (the right end searches
 * by donor) and the same sites in (acceptor, donor) order (the left end searches by acceptor), both built on the host: 16 bytes per
 * site and 4 per gene.  The host's own copy is freed with the context.  New: no counterpart. */
#define SHK_SPLICE_MAX_OVERHANG 48
#define SHK_SPLICE_BACK         16
typedef struct shk_splice_site { uint32_t gene, donor, acceptor; } shk_splice_site;
int shk_splice_sites_set(shk_ctx *ctx, const shk_splice_site *sites, uint64_t n);
/* Step 3b's parameters for the batches submitted AFTERWARDS: min_overhang = 0 switches the step off (the default),
 * 1 .. SHK_SPLICE_MAX_OVERHANG on; max_cost and min_gap 0 .. 64; anything else is SHK_ERR_ARG.  SHK_ERR_STATE while tickets are
 * outstanding, and when switching on without a site list.  It takes effect only where alignments mode or aligned pileup runs
 * (shk_alignments_extend's rule).  The command's defaults are 3, 2, 2.  With the step off the kernel launched and every record are
 * those from before this call existed.  New: no counterpart. */
int shk_alignments_splice(shk_ctx *ctx, uint32_t min_overhang, uint32_t max_cost, uint32_t min_gap);
/* The alignments of the batch whose result was handed out LAST, with shk_segments_last's rules: that result's lifetime and memory
 * space (pinned host memory for host batches, DEVICE memory for resident ones).  SHK_ERR_STATE if that batch was submitted with
 * the mode off, if its wait returned an error, behind shk_count_work, or if no batch has been waited for yet.  New: no counterpart. */
int shk_alignments_last(const shk_ctx *ctx, shk_alignments *out);
/* The text form of one record: its CIGAR string (NUL-terminated) into buf[0 .. cap) and the edit distance into *nm (nm may be NULL).
 * A pure host function -- no context, no device -- and the single definition of the text form.  L: the mate's length in bytes.  Walk:
 * q_0 as S; per block its len as M; between consecutive blocks R as I if R > 0, then G as N if G >= min_intron, else G as D if G > 0;
 * finally L - (q + len) of the last block as S.  Operations of length 0 are left out, adjacent equal operations are merged.
 *     *nm = mismatches + sum of R + sum of G over the gaps written as D.
 * n_blocks == 0 gives "*" and nm 0.  SHK_ERR_ARG if buf is NULL or too small (the text and its NUL must fit), or if the record is
 * inconsistent: more than 4 blocks, a block of length 0, blocks that do not ascend without overlap in x and in q, a block that ends
 * behind L.  New: no counterpart. */
int shk_alignment_cigar(const shk_mate_alignment *a, uint32_t L, uint32_t min_intron, char *buf, size_t cap, uint32_t *nm);

/* ---- indels: the insertions and deletions the mates' alignments show, tabled on the device over all batches ---- */
/* Variants mode reports where the sample differs from the record by one base; the CIGAR of a mate's alignment spells an inserted or
 * deleted stretch as I or D, one text line per mate.  Indels mode aggregates those gaps: one table entry per distinct event, with the
 * number of mates that show it on either strand.  It rests on the alignments section's definitions, unchanged: FINAL BLOCKS (those
 * after trimming, closure and, at the context's current parameters, steps 3b and 3a), read coordinate q, the read base on the record's
 * strand (0 .. 3; 4 for a byte that is no base or is masked by -q) and the record's code r (0 .. 3, else 4).
 *
 * GAP.  For each association, each mate of it with n_blocks >= 2 and each consecutive pair of its blocks (A, B):
 *   xa = x_A + len_A,  qa = q_A + len_A,  R = q_B - qa,  G = x_B - xa.
 *     R == 0 and 1 <= G < min_intron    DELETION of record bases [xa, xa + G)                               counted as `deletions`
 *     G == 0 and R >= 1                 INSERTION of the R read bases s[t] = read base qa + t, t < R,
 *                                       in front of record base xa                                         counted as `insertions`
 *     R >= 1 and G >= 1                 COMPLEX (closure left it open: G < R or R > 64), not tabled        counted as `complex_gaps`
 *     R == 0 and (G == 0 or G >= min_intron)   nothing (blocks that touch; an intron)
 *   min_intron is 1 .. 65535, so a tabled deletion's length fits 16 bits.
 * TABLED.  A deletion always is.  An insertion is iff R <= SHK_INDEL_MAX_INS and every s[t] < 4; otherwise it counts, in place of
 *   `insertions`, under `long_insertions` (R > SHK_INDEL_MAX_INS) or `nonbase_insertions` (R <= SHK_INDEL_MAX_INS and some s[t] == 4: an
 *   N, another byte, a base masked by -q).  So deletions + insertions = the tabled events, `dropped` ones included.
 * LEFT-NORMALISATION of a tabled event, over g's record [0, len_g):
 *   deletion   d = the largest number such that for every i in [xa - d, xa): r[i] < 4 and r[i] == r[i + G].  The event is the deletion of
 *              [xa - d, xa - d + G): x = xa - d, len = G.
 *   insertion  T[j] = r[j] for j < xa and T[xa + t] = s[t] for t < R.  d = the largest number such that for every i in [xa - d, xa):
 *              r[i] < 4 and T[i] == T[i + R].  The event is at x = xa - d with the bases s'[t] = T[xa - d + t], t < R: len = R.
 *   d is bounded only by x = 0 and by a record code of 4.  Alignments mode gives bases that two blocks could both hold to the LEFT block, so a
 *   raw event sits at the right end of its repeat; the same haplotype gets the same key whichever equivalent placement a mate's blocks took.
 * KEY.  (gene, x, kind, len, seq): kind 0 = deletion (seq = 0), kind 1 = insertion (seq = sum of s'[t] << 2 t).  Per key the table holds
 *   fwd and rev: the observations from mates whose record has strand 0 and 1, since the last reset, over the counted batches -- depth's
 *   rules word for word: mates are counted, not fragments; a read tied over several genes counts in each; integers only; a batch is counted
 *   exactly once (a batch with more associations than the result buffer holds or with reads beyond a length bound taken on trust is counted
 *   when its tail runs again; a batch vouched for wrongly and a shk_count_work batch are not counted).
 * STATS.  Seven 64-bit counters since the last reset: mates (records with n_blocks >= 1 that were examined), deletions, insertions,
 *   complex_gaps, long_insertions, nonbase_insertions, and dropped (a tabled event that found no entry: the table was full).
 * Example (k = 17): one A more in the record's run A x 8 at [200, 208) comes out of align_kernel as blocks that end and start at 208 with
 *   R = 1; d = 8, the key is (g, 200, 1, 1, A).  One CAG less in CAG x 4 at [400, 412): xa = 409 .. 412 by the mate's errors, G = 3, the key
 *   (g, 400, 0, 3, 0).
 *
 * What the mode does NOT do: allele fractions (shk_depth_get and shk_pileup_get give the denominators); insertions above
 * SHK_INDEL_MAX_INS bases; complex gaps; realigning mates around a called event.  Closure, trimming and the junction table are unchanged.
 *
 * Independent of every other mode: gene_off, gene_ids, n_assoc, shk_last_kernel, shk_gene_counts and every other mode's records and state
 * are the same with the mode on and off.  indel_kernel reads align_kernel's 64-byte records directly behind that kernel (in front of
 * rescue mode: a rescued mate's one block is no gap): with alignments mode on at the same floor one align_kernel launch serves both;
 * otherwise its storing instantiation runs once more, at this mode's floor, into an array of the context's own, allocated with the first
 * such batch and never handed out.  With the mode off no launch and no allocation is added.  New: the reference has no counterpart. */
#define SHK_INDEL_MAX_INS 12
typedef struct shk_indel { uint32_t gene, x, kind, len, seq, fwd, rev, reserved; } shk_indel;   /* 32 bytes */
typedef struct shk_indel_stats { uint64_t mates, deletions, insertions, complex_gaps, long_insertions, nonbase_insertions, dropped; } shk_indel_stats;
/* Switches the mode on with s_min = min_support (>= 1) or off (0; the other arguments are ignored, the table is kept) for the batches
 * submitted AFTERWARDS, through any of the four families.  min_intron 1 .. 65535, else SHK_ERR_ARG.  State rules are
 * shk_alignments_enable's: switching on returns SHK_ERR_STATE before shk_ref_finalize, without shk_ref_keep_positions, on an index of more
 * than 65 536 records, without shk_ref_keep_bases; either way while tickets are outstanding.  Capacity rules are shk_junctions_enable's:
 * table entries, rounded up to a power of two of at least 64, 16 bytes each {key, fwd, rev}; the first enable allocates and clears the
 * table; a later enable with another capacity or another min_intron returns SHK_ERR_ARG unless the table is clean (no batch submitted
 * with the mode on and nothing added since the first enable or the last shk_indels_reset). */
int shk_indels_enable(shk_ctx *ctx, uint32_t min_support, uint32_t min_intron, uint64_t capacity);
/* The read-outs, with shk_junctions_get's rules: SHK_ERR_STATE if the mode was never enabled on this context or while tickets are
 * outstanding; stream-ordered behind everything enqueued so far; the table is left untouched.  While `dropped` is not 0 shk_indels_get
 * returns SHK_ERR_INDEX_TOO_LARGE until shk_indels_reset (nothing partial is handed out).
 *   shk_indels_get     *n = the number of keys with fwd + rev >= min_mates; out != NULL: those keys sorted by (gene, x, kind, len, seq)
 *                      into out[0 .. *n) (host memory; SHK_ERR_ARG if cap < *n, *n is set all the same).  out == NULL: only *n
 *   shk_indels_stats   the seven counters
 *   shk_indels_add     adds in[0 .. n) (host memory) to the table -- fwd to fwd, rev to rev, a new key where the table has none -- and,
 *                      with stats != NULL, its counters to the table's: how N workers' tables become one.  SHK_ERR_ARG unless every entry
 *                      has gene < n_records, kind 0 with 1 <= len <= 65535 and seq == 0 or kind 1 with 1 <= len <= SHK_INDEL_MAX_INS and
 *                      no bit of seq at or above 2 len, x + (kind 0 ? len : 0) <= len_g, x < len_g, and reserved == 0 (nothing is added
 *                      then).  Stream-ordered; returns when done
 *   shk_indels_reset   empties the table and zeroes the counters (the mode, the capacity and min_intron stay as they are) */
int shk_indels_get(shk_ctx *ctx, uint32_t min_mates, shk_indel *out, uint64_t cap, uint64_t *n);
int shk_indels_stats(shk_ctx *ctx, shk_indel_stats *out);
int shk_indels_add(shk_ctx *ctx, const shk_indel *in, uint64_t n, const shk_indel_stats *stats /* may be NULL */);
int shk_indels_reset(shk_ctx *ctx);

/* ---- pairs: what the two mates of an association say together -- orientation, template, proper pair, MAPQ, fragment sizes ---- */
/* Alignments mode stops at the mate.  Pairs mode reads the two 64-byte records of an association side by side, the mates' lengths and
 * the read's number of associations, and hands out one 32-byte record per ASSOCIATION plus one aggregate over the sample: the
 * fragment-size histogram.  It rests on the alignments section's definitions, unchanged: block {x, q, len}, read coordinate (q counts
 * in the RECORD'S orientation on either strand), strand, and G = x_B - (x_A + len_A) between consecutive blocks A, B.  It changes no
 * alignment record.  Parameters: min_intron >= 1, max_frag, n_bins (2 .. 4096).  Integers only, no tolerance anywhere; a consistent
 * alignment record (blocks ascending and disjoint inside [0, len_g) and [0, L)) makes no difference below negative.
 *
 * PER MATE.  For an association (read i, gene g) take each mate m (0: mate 1, 1: mate 2) whose record has n_blocks >= 1; `last` is
 * block[n_blocks - 1]; L_m is the mate's length in bytes as align_kernel takes it, min(length, 2^31 - 1):
 *     s_m  = block[0].x                      the first record base under the mate
 *     e_m  = last.x + last.len               one behind the last
 *     cl_m = block[0].q                      read bases clipped on the record's LEFT
 *     cr_m = L_m - (last.q + last.len)       read bases clipped on the record's RIGHT
 *     intron intervals  [x_A + len_A, x_B)  for consecutive blocks A, B of the mate with G >= min_intron: exactly the gaps
 *                       shk_alignment_cigar writes as N at that min_intron (at most three per mate, six per association).
 * The mate on strand 0 reads along the record, so its 5' end is on the left and cl is what it lacks there; the mate on strand 1
 * reads against it, so its 5' end is on the right and cr is what it lacks there.
 *
 * PER ASSOCIATION: shk_pair.
 *   cls      0  no mate has a block.  Every other field but mapq is 0.
 *            1  only mate 1 has a block.           2  only mate 2 has a block.
 *            both have blocks, on different strands; F is the mate on strand 0, R the mate on strand 1:
 *            3  (inward)   s_F <= s_R and e_F <= e_R        4  (outward)  otherwise
 *            5  (tandem)   both have blocks on the same strand.
 *            (Mates that dovetail -- s_F <= s_R but e_F > e_R -- and an F that contains R are therefore outward, not inward.)
 *   left     the mate (0 or 1) with the smaller s; ties go to the smaller e, then to mate 0.  cls 1: 0; cls 2: 1.
 *   tstart   the smallest s, tend the largest e, over the mates with blocks.
 *   introns  the length of the UNION of both mates' intron intervals: two mates that cross the same intron count it once, two
 *            introns that overlap in part count every record base once.
 *   frag     cls 3 only, else 0:   (tend - tstart) - introns + cl_F + cr_R
 *            the template from one mate's 5' end to the other's: the span on the record, with the introns either mate SHOWS taken
 *            out and the clipped outer ends put back.  An intron that lies wholly inside the unsequenced insert between the mates
 *            is invisible to both and stays in: there frag is an UPPER BOUND of the fragment's length, not the length.
 *   proper   1 iff cls == 3 and frag <= max_frag, else 0.
 *   mapq     from the read's number of associations n = gene_off[i + 1] - gene_off[i] alone, the STAR scale with 60 for a unique
 *            read:  n = 1: 60;  n = 2: 3;  n = 3 or 4: 1;  n >= 5: 0.  Set on every association of the read, cls 0 included.
 * A single-end batch has no mate 2 record with a block: cls 0 or 1 only.
 * Example: L = 60 both; mate 1 on strand 0 with blocks {100, 2, 58}; mate 2 on strand 1 with blocks {300, 0, 20}, {1400, 20, 37}
 * (3 bases clipped on the right), min_intron = 20: s = 100, 300; e = 158, 1437; cls 3, left 0, tstart 100, tend 1437, introns 1080
 * ([320, 1400)), frag = 1337 - 1080 + 2 + 3 = 262.
 *
 * FRAGMENTS STATE, on the device, accumulated over all COUNTED batches under depth's, pileup's and the junction table's rule word for
 * word: a batch is counted exactly once (a batch with more associations than the result buffer holds, or with reads beyond a length
 * bound taken on trust, is counted when the tail runs again; a batch vouched for wrongly and a shk_count_work batch are never
 * counted -- the latter still gets its records).
 *   classes[6]    uint64: every association adds 1 to classes[cls];
 *   hist[n_bins]  uint64: an association with cls == 3 of a read with EXACTLY ONE association adds 1 to hist[min(frag, n_bins - 1)].
 *                 The last bin is the overflow bin: every frag >= n_bins - 1.
 *
 * Kernel (pairs.hip): pair_kernel directly behind the align_kernel launch that stores the records, one lane per read; a workgroup keeps
 * the histogram in LDS and flushes its non-zero bins once.  Independent of every other mode: gene_off, gene_ids, n_assoc,
 * shk_last_kernel, shk_gene_counts, the alignment records and every other mode's records and state are the same with the mode on and
 * off.  With the mode off no launch and no allocation is added.  New: the reference has no counterpart. */
typedef struct shk_pair {
  uint32_t cls, left, proper, mapq;
  int32_t  tstart, tend;
  uint32_t introns, frag;
} shk_pair;                                    /* 32 bytes */
typedef struct shk_pairs {
  uint64_t        n_assoc;                     /* = that result's n_assoc */
  const shk_pair *entries;                     /* n_assoc records, parallel to gene_ids */
} shk_pairs;
/* Switches pairs mode on (n_bins in 2 .. 4096, min_intron >= 1; anything else is SHK_ERR_ARG) or off (n_bins == 0; the other two are
 * ignored) for the batches submitted AFTERWARDS, through any of the four families.  State rules are shk_alignments_enable's; switching
 * on also returns SHK_ERR_STATE while alignments mode is off.  A batch gets pair records (and is counted) only if it was submitted
 * with alignments mode on as well: switching alignments mode off later leaves pairs mode set and idle.  The first enable allocates
 * and clears the fragments state; a later enable with another n_bins returns SHK_ERR_ARG unless no batch was submitted with the mode
 * on since the first enable or the last shk_fragments_reset (the state is then allocated anew) -- shk_junctions_enable's rule for its
 * capacity.  Switching off keeps the state.  New: no counterpart. */
int shk_pairs_enable(shk_ctx *ctx, uint32_t min_intron, uint32_t max_frag, uint32_t n_bins);
/* The pair records of the batch whose result was handed out LAST, with shk_alignments_last's rules: that result's lifetime and memory
 * space (pinned host memory for host batches, DEVICE memory for resident ones).  SHK_ERR_STATE if that batch was submitted without
 * pairs mode (or without alignments mode), if its wait returned an error, behind shk_count_work, or if no batch has been waited for
 * yet.  New: no counterpart. */
int shk_pairs_last(const shk_ctx *ctx, shk_pairs *out);
/* The fragments state's read-out and reset, with depth's rules: SHK_ERR_STATE if pairs mode was never enabled on this context or
 * while tickets are outstanding; stream-ordered behind everything enqueued so far; the read-out leaves the state untouched.
 *   shk_fragments_get    hist[0 .. n_bins) and classes[0 .. 6) into host memory; SHK_ERR_ARG if n_bins is not the state's
 *   shk_fragments_reset  clears both (the mode and n_bins stay as they are) */
int shk_fragments_get(shk_ctx *ctx, uint64_t *hist, uint32_t n_bins, uint64_t classes[6]);
int shk_fragments_reset(shk_ctx *ctx);

/* ---- rescue: an unplaced mate placed beside its placed partner, by dense comparison with the record ---- */
/* A mate gets a block only where a diagonal has s_min unique k-mers.  A mate with a few errors, one in a repeat of its gene, or a
 * short one stays without a block while its partner has one: pairs class 1 or 2.  The partner's record says where and on which strand
 * such a mate must lie for the pair to be proper; rescue mode compares the mate base by base with every such place and, where one
 * place is good enough and clearly the best, gives the mate an alignment record of one ungapped block.  It rests on the alignments
 * and the pairs section, unchanged: block, read coordinate, step 4's kinds, L_m, s_m, e_m, cl_m, cr_m, intron interval.  Parameters:
 * min_intron >= 1, max_frag in 1 .. 4096, max_cost in 0 .. 255, min_gap in 0 .. 255.  Integers only, no tolerance anywhere. */
#define SHK_RESCUE_MIN_LEN 32
#define SHK_RESCUE_MAX_LEN 512
/* ATTEMPTED.  Per association of a paired batch, after the alignments section's steps 1 .. 5 (3a included where it is on), rescue is
 * attempted iff exactly one mate has n_blocks >= 1 -- the ANCHOR A -- and the other, the TARGET T, has n_blocks == 0 and a length
 * L_T in [SHK_RESCUE_MIN_LEN, SHK_RESCUE_MAX_LEN].  s_A, e_A, cl_A, cr_A are the pairs section's; I_A = the total length of A's own
 * intron intervals at min_intron.  T's strand is 1 - strand_A.
 *
 * CANDIDATE.  A candidate x puts the whole target ungapped on the record: read coordinate q (in the record's orientation on T's
 * strand, as the alignments section defines it) on record base x + q for q = 0 .. L_T - 1.
 *
 * WINDOW, in signed 64-bit arithmetic (len_g: the record's length):
 *     A on strand 0:   lo = max(s_A, e_A - L_T, 0)                        hi = min(s_A - cl_A + I_A + max_frag - L_T, len_g - L_T)
 *     A on strand 1:   lo = max(e_A + cr_A - I_A - max_frag, 0)           hi = min(s_A, e_A - L_T, len_g - L_T)
 *     n_cand = max(0, hi - lo + 1)
 * These are exactly the x inside the record for which the pair would be pairs class 3 with frag <= max_frag.  The target's record
 * would be {x, 0, L_T}: s_T = x, e_T = x + L_T, no clip, no intron.  A on strand 0 is F: class 3 asks s_A <= x and e_A <= x + L_T;
 * then tstart = s_A, tend = x + L_T, introns = I_A and frag = x + L_T - s_A - I_A + cl_A, which is <= max_frag iff
 * x <= s_A - cl_A + I_A + max_frag - L_T.  A on strand 1 is R: class 3 asks x <= s_A and x + L_T <= e_A; then tstart = x,
 * tend = e_A and frag = e_A - x - I_A + cr_A, which is <= max_frag iff x >= e_A + cr_A - I_A - max_frag.
 * n_cand never exceeds max_frag: on strand 0, hi - lo + 1 <= (s_A - cl_A + I_A + max_frag - L_T) - (e_A - L_T) + 1
 * = max_frag - (e_A - s_A - I_A) - cl_A + 1, and e_A - s_A - I_A holds the anchor's block bases, at least one; on strand 1 the same
 * with hi <= s_A and cr_A.
 *
 * COST.  cost(x) = the number of the L_T target bases that are NOT A MATCH under step 4's kinds: a base that is neither a match nor
 * a mismatch (N, masked by -q, record code 4) counts as not a match, as it does in a split's cost.  cap = max_cost + min_gap; every
 * cost is taken as min(cost, cap + 1) -- the saturation lets the comparison of a candidate stop early.
 *     best   the x of smallest cost; ties go to the candidate of smallest frag: the smallest x for an anchor on strand 0, the
 *            largest x for an anchor on strand 1.
 *     cost2  the smallest cost over all OTHER candidates (a second candidate of the best's cost counts); cap + 1 with n_cand == 1.
 *
 * OUTCOME: shk_rescue, 16 bytes per association, parallel to gene_ids.
 *   state   0  not attempted; cost, cost2 and n_cand are 0
 *           1  attempted, n_cand == 0; cost = cost2 = cap + 1
 *           2  cost(best) > max_cost
 *           3  ambiguous: cost2 - cost(best) < min_gap (both saturated).  With min_gap == 0 this cannot occur.
 *           4  mate 1 rescued          5  mate 2 rescued
 *   cost    cost(best), cost2, both saturated; n_cand as above.
 * On rescue the target's shk_mate_alignment becomes n_blocks = 1, strand = 1 - strand_A, block[0] = {best, 0, L_T}, matches and
 * mismatches counted by step 4 over that block, everything else zero.  Every other alignment record of the batch stays bit-identical.
 * Example: L = 60 both, max_frag = 300, len_g = 2000; mate 1 on strand 0 with the one block {100, 2, 58}; mate 2 has no block.
 * s_A = 100, e_A = 158, cl_A = 2, I_A = 0: lo = max(100, 98, 0) = 100, hi = min(100 - 2 + 0 + 300 - 60, 1940) = 338, n_cand = 239.
 * If mate 2, reversed and complemented, differs from record bases 300 .. 359 in 3 places and from every other candidate's in at
 * least 30, then at max_cost = 8, min_gap = 4: cap = 12, cost = 3, cost2 = 13, state 5, and mate 2's record is strand 1, {300, 0, 60},
 * matches 57, mismatches 3 (fewer where one of the three is an N); pairs mode then gives class 3, frag = 360 - 100 + 2 = 262, proper.
 *
 * What the mode does NOT do:
 *   - a target that is itself spliced is not rescued: a candidate is one ungapped block;
 *   - a target that hangs over a record end is not rescued: the window keeps x in [0, len_g - L_T];
 *   - a target behind an intron that lies in the unsequenced insert is not rescued: the window is max_frag record bases wide;
 *   - a rescued mate does not enter depth, spliced depth, the junction table, pileup or aligned pileup: those accumulate before or
 *     inside align_kernel.  A rescued mate exists only in the alignment records, and through them in pairs mode and the SAM.
 *
 * Kernels (rescue.hip): directly behind the align_kernel launch that stores the records and in front of pair_kernel and the
 * publication of the records, so both see the rescued mate without knowing of the mode.  rescue_scan_kernel, one lane per read,
 * writes the state 0 records and queues the attempted associations; rescue_kernel, one wave per queued association, stages target
 * and window in LDS and prices 64 candidates per pass, four bases per instruction.  Independent of every other mode but for the
 * rescued mates' alignment records and what pairs mode derives from them.  With the mode off no launch and no allocation is added.
 * New: the reference has no counterpart. */
typedef struct shk_rescue {
  uint32_t state, cost, cost2, n_cand;
} shk_rescue;                                  /* 16 bytes */
typedef struct shk_rescues {
  uint64_t          n_assoc;                   /* = that result's n_assoc */
  const shk_rescue *entries;                   /* n_assoc records, parallel to gene_ids */
} shk_rescues;
/* Switches rescue mode on (max_frag in 1 .. 4096, min_intron >= 1, max_cost and min_gap in 0 .. 255; anything else is SHK_ERR_ARG)
 * or off (max_frag == 0; the others are ignored) for the batches submitted AFTERWARDS, through any of the four families.  State rules
 * are shk_pairs_enable's: SHK_ERR_STATE while tickets are outstanding and, switching on, while alignments mode is off.  A batch is
 * rescued only if it was submitted with alignments mode on as well.  The mode keeps no state of its own.  New: no counterpart. */
int shk_rescue_enable(shk_ctx *ctx, uint32_t min_intron, uint32_t max_frag, uint32_t max_cost, uint32_t min_gap);
/* The rescue records of the batch whose result was handed out LAST, with shk_pairs_last's rules.  New: no counterpart. */
int shk_rescue_last(const shk_ctx *ctx, shk_rescues *out);

/* Per-gene number of assigned reads accumulated over all classify calls (all
 * waited tickets) since the last reset (counts[g] for g in [0, 65536)); the quantity all-reduced
 * across GPUs.  n must be <= 65536. */
int shk_gene_counts(shk_ctx *ctx, uint64_t *counts, uint32_t n);
int shk_gene_counts_reset(shk_ctx *ctx);

/* The path's one exchange step when the read stream is sharded over several GPUs of one node (index
 * replicated, reads split): all-reduce (sum) of the per-gene counters over RCCL (xGMI).  New: the reference is
 * single process and has no counterpart (its per-read lines are merged by the output mutex, ReadOutput.hpp:38).
 * The totals land in a separate device buffer of every context; the per-GPU counters are left as they are, so
 * the call can be repeated.  RCCL is loaded on first use (librccl.so.1) and the communicators are created once.
 *
 * (a) one process, one context per GPU (`shark --gpus N`): `n_ctx` contexts; with one context and without
 *     SHK_FORCE_RCCL=1 in the environment no collective is needed and none is issued. */
int shk_gene_counts_allreduce(shk_ctx **ctxs, int n_ctx, uint64_t *totals, uint32_t n);
/* (b) one process per GPU (torch.distributed.run, mpirun): rank 0 calls shk_dist_unique_id, the launcher's own
 *     channel carries the SHK_DIST_ID_BYTES bytes to every rank, every rank calls shk_dist_init with its context;
 *     shk_dist_gene_counts_allreduce is then collective over the ranks (stream-ordered behind the classify calls
 *     made so far) and returns counts[0..n) of the totals.  Without shk_dist_init it returns the local counters. */
#define SHK_DIST_ID_BYTES 128
int shk_dist_unique_id(uint8_t *id);
int shk_dist_init(shk_ctx *ctx, const uint8_t *id, int rank, int world);
int shk_dist_gene_counts_allreduce(shk_ctx *ctx, uint64_t *totals, uint32_t n);
/* What the communicator itself says about the job this context joined with shk_dist_init: ncclCommUserRank /
 * ncclCommCount (a context that never joined one reports rank 0 of 1).  bench.py prints it as `ranks_seen`, so a
 * run that was asked for N GPUs and reached the collective with fewer cannot go unnoticed. */
int shk_dist_info(const shk_ctx *ctx, int *rank, int *world);

/* ---- measurement --------------------------------------------------------- */
/* HIP-event timing of the dominant kernel (classify) on the context's own
 * stream.  enable=1 starts recording one event pair per launch. */
int shk_timing_enable(shk_ctx *ctx, int enable);
/* n_launches classify-kernel launches since enable, their summed duration,
 * and the algorithmic work counters of the LAST classify call.  prepass_ms:
 * what ran in front of those launches for batches whose read lengths only the
 * device sees (shk_classify_device) or that are known to be ragged -- the
 * uniformity check over the offsets and, for batches of mixed lengths on small
 * indices, the sort by length; 0 for batches the host knows to be uniform. */
typedef struct shk_timing {
  uint64_t n_launches;
  double   total_ms;
  uint64_t last_n_reads;     /* pairs (or single reads) in the last call */
  uint64_t last_n_long;      /* reads routed to the general kernel */
  uint64_t last_n_tie;       /* reads with more than SHK_INLINE_IDS genes */
  uint64_t last_n_assoc;
  double   prepass_ms;
} shk_timing;
int shk_timing_get(shk_ctx *ctx, shk_timing *t);

/* Exact per-call work counters for the roofline's algorithmic-byte formula
 * (SURVEY.md 8d): counts k-mers probed, probes that hit, and gene-list
 * entries read during the NEXT classify call when enabled (a separate,
 * slower kernel build is used; never enabled in timed runs). */
typedef struct shk_work_counters {
  uint64_t n_kmers;      /* valid k-mers probed */
  uint64_t n_hits;       /* probes whose bit was set */
  uint64_t n_list_ids;   /* sum of list lengths over hits */
  uint64_t n_bases;      /* input base bytes consumed */
} shk_work_counters;
int shk_count_work(shk_ctx *ctx, const shk_batch *dev_batch, shk_work_counters *out);

/* The part's ceiling for INDEPENDENT random 16-byte lookups in a table of `table_bytes` (a power of two >= 1 MiB) on the
 * context's device: the access pattern of the position table, one bucket per k-mer at a hashed address.  On an index far
 * beyond the caches each lookup is one memory-side request (a 128-byte line of which 16 bytes are used) and the RATE of
 * those bounds the classify kernel; bench.py measures the ceiling with this call in the run whose fraction of it it
 * reports.  Allocates the table, performs about `n_lookups` lookups (five in flight per lane, 8 waves per SIMD;
 * `nontemporal` bit 0: streaming loads; bit 1: every lookup also reads 16 bytes of the other 64-byte half of its 128-byte
 * line -- the pair of rates says whether a random lookup moves a whole line or half of one, bench.py's calibration of
 * FETCH_SIZE for this access pattern; the figure returned is LINES per second either way), frees it again.  On no product
 * path; new (the reference has no counterpart). */
int shk_measure_random_lookups(shk_ctx *ctx, uint64_t table_bytes, uint64_t n_lookups, int nontemporal, double *g_lookups_per_s);

/* The ISSUE ceiling of the exact-table classify kernel's own instruction mix: a kernel that does, on register operands only
 * (no LDS, no memory), the arithmetic that kernel does for a read on its shortest way through -- stage eight bases, a slot's two
 * windows, canonical form, XXH64 (kmer_utils.hpp:81-83), the exact table's address arithmetic and compare, validity window and
 * coverage step -- `iters` times per lane with `waves_per_simd` (1 ... 8) waves resident per SIMD; *ms = its duration,
 * *wave_iterations = waves x iters.  bench.py takes the instructions per iteration from the same rocprofv3 counter pass that
 * counts the classify kernel's, and prints the classify kernel's VALU rate as a fraction of this kernel's (`mix_ceiling`) next
 * to the fraction of the 2-cycle peak.  On no product path; new (the reference has no counterpart). */
int shk_measure_valu_mix(shk_ctx *ctx, int waves_per_simd, uint32_t iters, double *ms, uint64_t *wave_iterations);

/* The same, and *shader_ghz = the clock the SIMDs held while that kernel ran: shader cycles (s_memtime) over the constant 100 MHz
 * counter (s_memrealtime) around each wave's loop, summed over the waves.  The chip lowers its clock under load, so a rate in
 * instructions per second prices a kernel against 2.4 GHz it may not have had; bench.py reports cycles per instruction beside it
 * (`roofline.clock`).  On no product path; new (the reference has no counterpart). */
int shk_measure_valu_mix_clock(shk_ctx *ctx, int waves_per_simd, uint32_t iters, double *ms, uint64_t *wave_iterations, double *shader_ghz);

/* Test-only: the three launches that assemble the result of a batch against an index of ONE record (every association is gene 0's:
 * the scan of the per-read counts writes the offsets, fills gene_ids with id 0, writes the batch's counters and counts gene 0) over
 * the caller's `count[0 .. n)`, n >= 1, on the context's device and stream; works in any mode of the context, with or without an index,
 * allocates what it needs and frees it again.  count_off / off_off (0 .. 3) place the device copies of count / gene_off that many
 * words behind a 16-byte aligned address ((0, 0): 16-byte accesses, anything else word by word).  gene_ids_cap: the capacity of the
 * device's gene_ids; ctr_long: what the counter of queued long reads holds beforehand; skip_if_long, count_genes: as a classify
 * call sets them -- gene 0 is counted when count_genes, the total fits the capacity, and not (skip_if_long and ctr_long != 0).
 * Hands back gene_off[0 .. n); gene_ids[0 .. gene_ids_cap), which starts as SHK_DEBUG_FILL16 in every word; the counter block of
 * SHK_DEBUG_COUNTER_WORDS words ([SHK_DEBUG_CTR_LONG] as given, [SHK_DEBUG_CTR_OVERFLOW] = total > gene_ids_cap,
 * [SHK_DEBUG_CTR_ASSOC_LO / _HI] = the total, every other word 0); what was added to gene 0's counter; and, per device buffer, the
 * guard words in front of it and behind it that changed -- count, gene_off, the scan's temp, gene_ids, the counters, gene 0's
 * counter, (front, back) each; a changed word of count itself is counted with its back band.  All zero on a clean run. */
#define SHK_DEBUG_FILL16 0x0FF2u
#define SHK_DEBUG_COUNTER_WORDS 16
#define SHK_DEBUG_CTR_LONG 0
#define SHK_DEBUG_CTR_OVERFLOW 2
#define SHK_DEBUG_CTR_ASSOC_LO 6
#define SHK_DEBUG_CTR_ASSOC_HI 7
int shk_debug_assemble_one(shk_ctx *ctx, const uint32_t *count, uint64_t n, uint32_t count_off, uint32_t off_off, uint64_t gene_ids_cap,
                           uint32_t ctr_long, int skip_if_long, int count_genes, uint32_t *gene_off, uint16_t *gene_ids,
                           uint32_t *counters /* [SHK_DEBUG_COUNTER_WORDS] */, uint64_t *gene0_added, uint32_t *guard_changed /* [12] */);

/* Test-only: what became of the speculation on the last batch finished.  Behind a batch that the device judged uniform,
 * shk_classify_device launches the next batch's uniform kernel for the same lengths at once and has the device look at the offsets
 * BESIDE that launch (index of one record whose uniform batches take the exact table in LDS, a length bound that fits, no
 * record mode, no accumulating state; SHK_NO_SPECULATE=1, read by shk_create: never).  0: the batch was not speculated on; 1: it was,
 * and its lengths were the expected ones; 2: it was, they were not, and the batch was run again the ordinary way.  Results, shk_last_kernel,
 * shk_gene_counts and the last_n_* figures are the same in all three cases; in shk_timing, prepass_ms of a speculated batch is about 0
 * (no pass over the offsets stands in front of its classify launch), and for a batch that was run again (2) prepass_ms and total_ms are
 * those of the first, wasted pass: the second run is not timed. */
int shk_debug_last_speculation(const shk_ctx *ctx);

/* pinned host memory helpers for callers that stream batches */
void *shk_alloc_pinned(size_t bytes);
void  shk_free_pinned(void *p);

/* library / build identification */
const char *shk_version(void);

#ifdef __cplusplus
}
#endif
#endif
