// shark_cli.cpp -- the `shark` command line on top of libsharkhip.
//
// Drop-in for the reference binary: identical flags, defaults and validation
// (argument_parser.hpp:29-174), ssv on stdout (ReadOutput.hpp:43), surviving
// reads as FASTQ in -o/-p (ReadOutput.hpp:44-47), `[shark/...] Time elapsed`
// lines on stderr (main.cpp:47-54).  Output order is the reference's `-t 1`
// order (input order, genes ascending).
//
// Host structure mirrors main.cpp's three functor stages per worker loop
// (main.cpp:66-77: split / analyze / output); which threads play them here is
// described at run_sample() below, and main() lists the stages of a run.
// Extra flags: --gpus N, --devices LIST, --batch N, --gene-counts FILE.
#include <getopt.h>
#include <sched.h>
#include <sys/stat.h>

#include <algorithm>
#include <cctype>
#include <chrono>
#include <fstream>
#include <condition_variable>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <iostream>
#include <atomic>
#include <map>
#include <memory>
#include <mutex>
#include <sstream>
#include <string>
#include <thread>
#include <tuple>
#include <unordered_map>
#include <utility>
#include <vector>

#include "../../include/shark_hip.h"
#include "fastq_block_reader.hpp"
#include "fastq_lean_reader.hpp"
#include "fastq_partition.hpp"
#include "fastx_reader.hpp"
#include "gzip_parallel.hpp"
#include "indel_host.hpp"

namespace {

// ---- argument_parser.hpp ---------------------------------------------------
const char *USAGE_MESSAGE =
    "Usage: shark -r <references> -1 <sample1> [OPTIONAL ARGUMENTS]\n"
    "\n"
    "Arguments:\n"
    "      -r, --reference                   reference sequences in FASTA format (can be gzipped)\n"
    "      -1, --sample1                     sample in FASTQ (can be gzipped)\n"
    "\n"
    "Optional arguments:\n"
    "      -h, --help                        display this help and exit\n"
    "      -2, --sample2                     second sample in FASTQ (optional, can be gzipped)\n"
    "      -o, --out1                        first output sample in FASTQ (default: sharked_sample.1)\n"
    "      -p, --out2                        second output sample in FASTQ (default: sharked_sample.2)\n"
    "      -k, --kmer-size                   size of the kmers to index (default:17, max:31)\n"
    "      -c, --confidence                  confidence for associating a read to a gene (default:0.6)\n"
    "      -b, --bf-size                     bloom filter size in GB (default:1)\n"
    "      -q, --min-base-quality            minimum base quality (assume FASTQ Illumina 1.8+ Phred scale, default:0, i.e., no filtering)\n"
    "      -s, --single                      report an association only if a single gene is found\n"
    "      -t, --threads                     number of threads (default:1)\n"
    "      -v, --verbose                     verbose mode\n"
    "\n"
    "MI355X build only:\n"
    "          --gpus N                      number of GPUs to shard the reads over (default:1)\n"
    "          --devices LIST                the devices of the N workers, comma separated (default:0,1,...,N-1; a device may be\n"
    "                                        named more than once: several workers then share it)\n"
    "          --batch N                     reads per device batch (default:65536, up to 262144 for large plain samples)\n"
    "          --gene-counts FILE            write <gene> <assigned reads> per gene (summed over the GPUs with RCCL)\n"
    "          --evidence FILE               write <read> <coverage> <kmers> <valid bases> of every read (pair), in input order: the best\n"
    "                                        gene's figures, which pass iff kmers > 0 and coverage >= c * valid bases (slower: every\n"
    "                                        k-mer of every read is probed)\n"
    "          --candidates FILE             write <read> <valid bases> <genes hit> and then <gene> <coverage> <kmers> of the read's best\n"
    "                                        genes (coverage, then kmers, then the legend's order), one line per read (pair), in input\n"
    "                                        order (as slow as --evidence; may be combined with it)\n"
    "          --candidates-n M              genes per line of --candidates (default:4, 1 to 8)\n"
    "          --placements FILE             write <read> <gene> <strand> <pos> <support> per association (paired: the same three for mate 2\n"
    "                                        behind them), in the order of the output's lines: where in the gene's record and on which\n"
    "                                        strand each mate lies by its unique k-mers (may be combined with --evidence and\n"
    "                                        --candidates; not for references of more than 65536 records)\n"
    "          --depth FILE                  write <gene> <start> <end> <depth> per run of equal depth >= 1 (0-based, half-open), genes in\n"
    "                                        the legend's order: how many placed mates cover each base of each gene's record, summed\n"
    "                                        over the whole sample on the GPUs (may be combined with --placements, --evidence and\n"
    "                                        --candidates; not for references of more than 65536 records)\n"
    "          --depth-min-support N         unique k-mers a mate's placement needs to be counted by --depth (default:1)\n"
    "          --depth-spliced               --depth counts, per mate, the record bases its diagonals explain (the union of the spans of\n"
    "                                        its best 4 diagonals with at least --depth-min-support unique k-mers on the best one's\n"
    "                                        strand) instead of one stretch of the mate's length: a spliced mate leaves its introns out\n"
    "          --segments FILE               write <read> <gene> and per mate <diagonals> and M x <strand> <pos> <support> <first> <last>\n"
    "                                        per association, in the order of the output's lines: the M diagonals of the gene's record\n"
    "                                        most of the mate's unique k-mers lie on, with the first and last k-mer slot on each (a\n"
    "                                        spliced mate lies on several; empty entries are 0 0 0 0 0; not for references of more\n"
    "                                        than 65536 records)\n"
    "          --segments-max M              diagonals per mate of --segments and --junctions (default:4, 1 to 4)\n"
    "          --junctions FILE              write <gene> <donor> <acceptor> <intron> <mates> per junction the sample's mates show, sorted\n"
    "                                        by gene, donor, acceptor (record coordinates: the first base behind the left part, the\n"
    "                                        first base of the right part; the same refusals as --segments)\n"
    "          --junctions-min-support N     unique k-mers each side of a junction needs (default:8)\n"
    "          --junctions-device            the table of --junctions is accumulated on the GPUs instead of from the segments on the\n"
    "                                        host (the same file; needs --segments-max 4, the default)\n"
    "          --junctions-capacity N        entries of that table per worker, rounded up to a power of two (default:1048576, 16 bytes\n"
    "                                        each; it must hold every distinct junction: a full table is an error, not a shorter file)\n"
    "          --pileup FILE                 write <gene> <x> <A> <C> <G> <T> per record base (0-based) at least one mate shows a base at:\n"
    "                                        how many mates show each base there, on the record's strand, under the spans --depth-spliced\n"
    "                                        counts, summed over the whole sample on the GPUs; genes in the legend's order (combines with\n"
    "                                        --depth, --junctions and --segments; not for references of more than 65536 records)\n"
    "          --pileup-min-support N        unique k-mers a diagonal of a mate needs to be read by --pileup (default:8)\n"
    "          --variants FILE               write <gene> <x> <ref> <alt> <A> <C> <G> <T> per record base (0-based) where the sample's pileup\n"
    "                                        shows another base than the record: the counts of --pileup held against the record on the\n"
    "                                        GPU; ref and alt as letters, genes in the legend's order (the same refusals as --pileup)\n"
    "          --variants-min-support N      unique k-mers a diagonal of a mate needs to be read by --variants (default:8; with --pileup\n"
    "                                        the two must agree: there is one pileup)\n"
    "          --variants-min-depth N        mates that must show a base at a site (default:8)\n"
    "          --variants-min-alt N          mates that must show the alternative base (default:3)\n"
    "          --variants-min-frac P/Q       the alternative base's share of those mates, at least P/Q (default:1/5; P <= Q <= 65535)\n"
    "          --indels FILE                 write <gene> <x> <I|D> <len> <seq> <fwd> <rev> per insertion or deletion the sample's alignments\n"
    "                                        show (the gaps between the blocks --sam shows, moved as far left as the record allows and\n"
    "                                        tabled on the GPUs): x 0-based, seq the inserted bases on the record's strand or *, fwd and rev\n"
    "                                        the mates on either strand; sorted by gene, x, kind, len, seq (honours --extend-ends and\n"
    "                                        --splice-junctions; the same refusals as --sam)\n"
    "          --indels-min-support N        unique k-mers a diagonal of a mate needs to become a block (default:8)\n"
    "          --indels-min-intron N         record bases from which on a gap is an intron, not a deletion (1 .. 65535, default:20)\n"
    "          --indels-min-mates N          mates an event needs to be written (default:2)\n"
    "          --indels-capacity N           entries of the table per worker, rounded up to a power of two (default:1048576, 16 bytes each;\n"
    "                                        it must hold every distinct event: a full table is an error, not a shorter file)\n"
    "          --sam FILE                    write the gapped alignment of every placed mate to its gene's record as SAM: one line per\n"
    "                                        association and mate with at least one block, in input order (header: @HD, one @SQ per gene;\n"
    "                                        MAPQ 255, TLEN 0, NM:i: from the record's bases; the mate's ends outside its blocks are soft\n"
    "                                        clips; the same refusals as --segments; combines with every other output)\n"
    "          --sam-min-support N           unique k-mers a diagonal of a mate needs to become a block of --sam (default:8)\n"
    "          --sam-min-intron N            record bases a gap between two blocks needs to be written as N, not D (default:20)\n"
    "          --sam-pairs                   --sam: fill in the pair-level fields -- MAPQ from the read's number of genes (1: 60, 2: 3, 3-4: 1,\n"
    "                                        more: 0), 0x2 on both lines of an inward pair whose fragment is at most --fragments-max, TLEN\n"
    "                                        = the pair's span on the record, positive on the left mate's line (needs --sam FILE)\n"
    "          --sam-rescue                  --sam: a mate without a block whose partner has one is compared base by base with every place\n"
    "                                        beside the partner at which the pair would be inward with a fragment of at most\n"
    "                                        --fragments-max (1 .. 4096 here); the one clearly best place becomes its alignment, one\n"
    "                                        ungapped block, and its line carries YR:i:<bases that are not a match> (needs --sam FILE)\n"
    "          --rescue-max-cost N           bases of a rescued mate that may differ from the record (0 .. 255, default:8)\n"
    "          --rescue-min-gap N            bases by which every other place must be worse (0 .. 255, default:4)\n"
    "          --fragments FILE              write the sample's pair classes and fragment-size histogram, accumulated on the GPUs: six\n"
    "                                        lines `class <name> <count>` (none mate1 mate2 inward outward tandem; every association),\n"
    "                                        one line `frag <len> <count>` per non-empty bin and `frag >=<bins-1> <count>` for the rest\n"
    "                                        (inward pairs of reads with one gene; introns either mate shows are taken out; alignments as\n"
    "                                        --sam's, at --sam-min-support; the same refusals as --sam)\n"
    "          --fragments-max N             the longest fragment of a proper pair (default:1000)\n"
    "          --fragments-bins N            bins of the histogram, the last one open-ended (2 .. 4096, default:1024)\n"
    "          --fragments-min-intron N      record bases a gap needs to count as an intron of the pair (default: --sam-min-intron's)\n"
    "          --extend-ends                 --sam, --pileup-aligned and --indels: grow a mate's outermost blocks over its clipped ends base by base\n"
    "                                        (match 1, mismatch 4, 5 for reaching the mate's end), so that a substitution within k of\n"
    "                                        an end is shown instead of clipped\n"
    "          --extend-penalty N            the mismatch penalty of --extend-ends (1 .. 15, default:4)\n"
    "          --extend-bonus N              its bonus for reaching the mate's end (0 .. 15, default:5)\n"
    "          --pileup-aligned              --pileup / --variants count the bases of the alignment --sam shows (trimmed, gaps closed,\n"
    "                                        ends extended under --extend-ends) instead of the bases under the voting windows\n"
    "          --splice-junctions FILE       --sam, --pileup-aligned and --indels: try a mate's clipped end of a few bases across the introns FILE lists\n"
    "                                        (what --junctions writes: <gene> <donor> <acceptor> <intron> [<mates>]; the intron is record\n"
    "                                        bases [donor, donor + intron)) and place it where that is good and clearly the best\n"
    "          --splice-min-mates N          FILE's lines with fewer mates are left out (default:1)\n"
    "          --splice-min-overhang N       the shortest clipped end that is tried (1 .. 48, default:3)\n"
    "          --splice-max-cost N           read bases of the evaluated end that may disagree with the record (0 .. 64, default:2)\n"
    "          --splice-min-gap N            by how many such bases every other placement must be worse (0 .. 64, default:2)\n"
    "          --kmer-table                  one gene, k <= 17: also build the exact table keyed by the k-mer itself (no XXH64 per probe; the\n"
    "                                        same output).  Costs tens of milliseconds when the index is built and pays on the GPU\n"
    "                                        alone, so it is off here, where the host and the link bound a run\n"
    "      -t N also sets the number of host threads that parse FASTQ / format output (default: up to 16)\n";

struct Options {
  std::string fasta_path, sample1_path, sample2_path, out1_path, out2_path;
  bool paired_flag = false;
  unsigned k = 17;
  double c = 0.6;
  uint64_t bf_size = (uint64_t)1 << 33;
  int min_quality = 0;     // as typed; the library narrows it to the reference's `char` (argument_parser.hpp:144)
  bool single = false, verbose = false;
  int nThreads = 1;
  int gpus = 1;
  bool gpus_given = false;
  std::vector<int> devices;     // --devices: worker g runs on devices[g] (empty: worker g on device g)
  uint64_t batch = 1u << 16;
  bool batch_given = false;     // (--batch; otherwise the sample's size decides: auto_batch below)
  std::string gene_counts_path;
  std::string evidence_path;
  FILE *evidence_file = nullptr;   // (--evidence, opened by main() before any work is done)
  std::string candidates_path;
  FILE *candidates_file = nullptr; // (--candidates, likewise)
  unsigned candidates_n = 4;
  bool candidates_n_given = false;
  std::string placements_path;
  FILE *placements_file = nullptr; // (--placements, likewise)
  std::string depth_path;
  FILE *depth_file = nullptr;      // (--depth, likewise; written once, after the last batch)
  unsigned depth_min_support = 1;
  std::string segments_path;
  FILE *segments_file = nullptr;   // (--segments, likewise)
  unsigned segments_max = SHK_MAX_SEGMENTS;
  std::string junctions_path;
  FILE *junctions_file = nullptr;  // (--junctions, likewise; written once, after the last batch)
  unsigned junctions_min_support = 8;
  bool depth_spliced = false;             // (--depth-spliced)
  bool junctions_device = false;          // (--junctions-device: the table comes from the library's junction table, not from ReadOutput's)
  uint64_t junctions_capacity = 1u << 20; // (--junctions-capacity; entries per worker: 16 MiB, a thousand times the junctions of a human transcriptome's panel)
  bool junctions_capacity_given = false;
  std::string pileup_path;
  FILE *pileup_file = nullptr;     // (--pileup, likewise; written once, after the last batch)
  unsigned pileup_min_support = 8;
  bool pileup_min_support_given = false;
  std::string variants_path;
  FILE *variants_file = nullptr;   // (--variants, likewise; written once, after the last batch and after --pileup's file)
  unsigned variants_min_support = 8;
  std::string indels_path;
  FILE *indels_file = nullptr;     // (--indels, likewise; written once, after the last batch)
  unsigned indels_min_support = 8, indels_min_intron = 20, indels_min_mates = 2;
  uint64_t indels_capacity = 1u << 20;    // (--indels-capacity; entries per worker: 16 MiB)
  bool indels_sub_flag_given = false;
  std::string sam_path;
  FILE *sam_file = nullptr;        // (--sam, likewise; the header is written once the reference is read, the lines per batch)
  unsigned sam_min_support = 8, sam_min_intron = 20;
  bool sam_sub_flag_given = false;
  bool sam_pairs = false;                 // (--sam-pairs)
  bool sam_rescue = false;                // (--sam-rescue; --rescue-max-cost, --rescue-min-gap)
  unsigned rescue_max_cost = 8, rescue_min_gap = 4;
  bool rescue_sub_flag_given = false;
  std::string splice_path;                // (--splice-junctions; --splice-min-mates, --splice-min-overhang, --splice-max-cost, --splice-min-gap)
  unsigned splice_min_mates = 1, splice_min_overhang = 3, splice_max_cost = 2, splice_min_gap = 2;
  bool splice_sub_flag_given = false;
  std::string fragments_path;
  FILE *fragments_file = nullptr;  // (--fragments, likewise; written once, after the last batch)
  unsigned fragments_max = 1000, fragments_bins = 1024, fragments_min_intron = 0;   // (0: --sam-min-intron's value)
  bool fragments_sub_flag_given = false;
  bool extend_ends = false;               // (--extend-ends; --extend-penalty, --extend-bonus)
  unsigned extend_penalty = 4, extend_bonus = 5;
  bool extend_sub_flag_given = false;
  bool pileup_aligned = false;            // (--pileup-aligned)
  bool kmer_table = false;         // (--kmer-table: the one-gene index's table keyed by the k-mer, shk_ref_kmer_table; off here unless asked for)
  shk_variant_params variants_params{8, 3, 1, 5};   // (--variants-min-depth, -min-alt, -min-frac)
  bool variants_sub_flag_given = false;
  bool variants_min_support_given = false;
};

// The command line is described by one table: option names, whether a value follows, and a handler that
// stores the value and applies that option's own check at once -- options are checked in the order they
// appear, as the reference does (argument_parser.hpp:84-174), so the first bad option decides the message.
// Flags, messages and exit codes are the contract (tests/test_cabi_cpu.py::test_cli_argument_contract).
[[noreturn]] void reject(const char *before, const char *message)
{
  std::cerr << before << message << std::endl << "aborting..." << std::endl;
  exit(EXIT_FAILURE);
}

// values are extracted the way operator>> does it (leading blanks skipped, trailing text ignored, 0 on failure)
template <typename T>
T value_of(const char *text)
{
  T v{};
  std::istringstream in(text ? text : "");
  in >> v;
  return v;
}

struct OptionRow {
  int key;                 // short option character, or >= 1000 for long-only options
  const char *name;
  bool takes_value;
  void (*apply)(Options &, const char *);
};

const OptionRow OPTION_TABLE[] = {
    {'r', "reference", true, [](Options &o, const char *v) { o.fasta_path = value_of<std::string>(v); }},
    {'t', "threads", true,
     [](Options &o, const char *v) {
       o.nThreads = value_of<int>(v);
       // (the reference prints the literal word here, argument_parser.hpp:95)
       if (o.nThreads <= 0) reject("USAGE_MESSAGE", "shark: at least 1 thread is required.");
     }},
    {'1', "sample1", true, [](Options &o, const char *v) { o.sample1_path = value_of<std::string>(v); }},
    {'2', "sample2", true, [](Options &o, const char *v) { o.sample2_path = value_of<std::string>(v); o.paired_flag = true; }},
    {'o', "out1", true, [](Options &o, const char *v) { o.out1_path = value_of<std::string>(v); }},
    {'p', "out2", true, [](Options &o, const char *v) { o.out2_path = value_of<std::string>(v); }},
    {'k', "kmer-size", true,
     [](Options &o, const char *v) {
       o.k = value_of<unsigned>(v);
       if (o.k < 1 || o.k > 31) reject(USAGE_MESSAGE, "shark: k must be in the range [1, 31].");
     }},
    {'c', "confidence", true,
     [](Options &o, const char *v) {
       o.c = value_of<double>(v);
       if (o.c < 0 || o.c > 1) reject("", "shark: c must be in the range [0, 1].");
     }},
    {'b', "bf-size", true, [](Options &o, const char *v) { o.bf_size = value_of<uint64_t>(v) << 33; /* GB -> bits */ }},
    {'q', "min-base-quality", true,
     [](Options &o, const char *v) {
       o.min_quality = value_of<int>(v);
       if (o.min_quality < 0) reject(USAGE_MESSAGE, "shark: q must be a positive value.");
     }},
    {'s', "single", false, [](Options &o, const char *) { o.single = true; }},
    {'v', "verbose", false, [](Options &o, const char *) { o.verbose = true; }},
    {'h', "help", false, [](Options &, const char *) { std::cerr << USAGE_MESSAGE; exit(EXIT_SUCCESS); }},
    {1000, "gpus", true, [](Options &o, const char *v) { o.gpus = std::max(1, value_of<int>(v)); o.gpus_given = true; }},
    {1003, "devices", true,
     [](Options &o, const char *v) {
       // a list of non-negative device numbers; anything else is refused (a typo must not silently become device 0)
       o.devices.clear();
       const std::string text = v ? v : "";
       size_t at = 0;
       while (at <= text.size()) {
         const size_t comma = std::min(text.find(',', at), text.size());
         const std::string item = text.substr(at, comma - at);
         if (item.empty() || item.size() > 4 || item.find_first_not_of("0123456789") != std::string::npos)
           reject("", "shark: --devices takes a comma separated list of device numbers.");
         o.devices.push_back(atoi(item.c_str()));
         at = comma + 1;
       }
     }},
    {1001, "batch", true, [](Options &o, const char *v) { o.batch = std::max<uint64_t>(1, value_of<uint64_t>(v)); o.batch_given = true; }},
    {1002, "gene-counts", true, [](Options &o, const char *v) { o.gene_counts_path = value_of<std::string>(v); }},
    {1004, "evidence", true, [](Options &o, const char *v) { o.evidence_path = value_of<std::string>(v); }},
    {1005, "candidates", true, [](Options &o, const char *v) { o.candidates_path = value_of<std::string>(v); }},
    {1006, "candidates-n", true,
     [](Options &o, const char *v) {
       o.candidates_n = value_of<unsigned>(v);
       o.candidates_n_given = true;
       if (o.candidates_n < 1 || o.candidates_n > SHK_MAX_CANDIDATES) reject(USAGE_MESSAGE, "shark: --candidates-n must be in the range [1, 8].");
     }},
    {1007, "placements", true, [](Options &o, const char *v) { o.placements_path = value_of<std::string>(v); }},
    {1008, "depth", true, [](Options &o, const char *v) { o.depth_path = value_of<std::string>(v); }},
    {1009, "depth-min-support", true,
     [](Options &o, const char *v) {
       o.depth_min_support = value_of<unsigned>(v);
       if (o.depth_min_support < 1) reject(USAGE_MESSAGE, "shark: --depth-min-support must be at least 1.");
     }},
    {1010, "segments", true, [](Options &o, const char *v) { o.segments_path = value_of<std::string>(v); }},
    {1011, "segments-max", true,
     [](Options &o, const char *v) {
       o.segments_max = value_of<unsigned>(v);
       if (o.segments_max < 1 || o.segments_max > SHK_MAX_SEGMENTS) reject(USAGE_MESSAGE, "shark: --segments-max must be in the range [1, 4].");
     }},
    {1012, "junctions", true, [](Options &o, const char *v) { o.junctions_path = value_of<std::string>(v); }},
    {1013, "junctions-min-support", true,
     [](Options &o, const char *v) {
       o.junctions_min_support = value_of<unsigned>(v);
       if (o.junctions_min_support < 1) reject(USAGE_MESSAGE, "shark: --junctions-min-support must be at least 1.");
     }},
    {1024, "kmer-table", false, [](Options &o, const char *) { o.kmer_table = true; }},
    {1014, "depth-spliced", false, [](Options &o, const char *) { o.depth_spliced = true; }},
    {1015, "junctions-device", false, [](Options &o, const char *) { o.junctions_device = true; }},
    {1016, "junctions-capacity", true,
     [](Options &o, const char *v) {
       o.junctions_capacity = value_of<uint64_t>(v);
       o.junctions_capacity_given = true;
       if (o.junctions_capacity < 1 || o.junctions_capacity > (1ull << 32)) reject(USAGE_MESSAGE, "shark: --junctions-capacity must be in the range [1, 4294967296].");
     }},
    {1017, "pileup", true, [](Options &o, const char *v) { o.pileup_path = value_of<std::string>(v); }},
    {1018, "pileup-min-support", true,
     [](Options &o, const char *v) {
       o.pileup_min_support = value_of<unsigned>(v);
       o.pileup_min_support_given = true;
       if (o.pileup_min_support < 1) reject(USAGE_MESSAGE, "shark: --pileup-min-support must be at least 1.");
     }},
    {1019, "variants", true, [](Options &o, const char *v) { o.variants_path = value_of<std::string>(v); }},
    {1020, "variants-min-support", true,
     [](Options &o, const char *v) {
       o.variants_min_support = value_of<unsigned>(v);
       o.variants_sub_flag_given = o.variants_min_support_given = true;
       if (o.variants_min_support < 1) reject(USAGE_MESSAGE, "shark: --variants-min-support must be at least 1.");
     }},
    {1021, "variants-min-depth", true,
     [](Options &o, const char *v) {
       o.variants_params.min_depth = value_of<unsigned>(v);
       o.variants_sub_flag_given = true;
       if (o.variants_params.min_depth < 1) reject(USAGE_MESSAGE, "shark: --variants-min-depth must be at least 1.");
     }},
    {1022, "variants-min-alt", true,
     [](Options &o, const char *v) {
       o.variants_params.min_alt = value_of<unsigned>(v);
       o.variants_sub_flag_given = true;
       if (o.variants_params.min_alt < 1) reject(USAGE_MESSAGE, "shark: --variants-min-alt must be at least 1.");
     }},
    {1023, "variants-min-frac", true,
     [](Options &o, const char *v) {
       // P/Q, both decimal, nothing else
       unsigned long long num = 0, den = 0;
       int used = 0;
       const bool parsed = sscanf(v, "%llu/%llu%n", &num, &den, &used) == 2 && v[used] == '\0' && isdigit((unsigned char)v[0]);
       o.variants_sub_flag_given = true;
       if (!parsed || den < 1 || den > 65535 || num > den) reject(USAGE_MESSAGE, "shark: --variants-min-frac must be P/Q with P <= Q and Q in the range [1, 65535].");
       o.variants_params.frac_num = (uint32_t)num;
       o.variants_params.frac_den = (uint32_t)den;
     }},
    {1024, "sam", true, [](Options &o, const char *v) { o.sam_path = value_of<std::string>(v); }},
    {1025, "sam-min-support", true,
     [](Options &o, const char *v) {
       o.sam_min_support = value_of<unsigned>(v);
       o.sam_sub_flag_given = true;
       if (o.sam_min_support < 1) reject(USAGE_MESSAGE, "shark: --sam-min-support must be at least 1.");
     }},
    {1026, "sam-min-intron", true,
     [](Options &o, const char *v) {
       o.sam_min_intron = value_of<unsigned>(v);
       o.sam_sub_flag_given = true;
     }},
    {1027, "extend-ends", false, [](Options &o, const char *) { o.extend_ends = true; }},
    {1028, "extend-penalty", true,
     [](Options &o, const char *v) {
       o.extend_penalty = value_of<unsigned>(v);
       o.extend_sub_flag_given = true;
       if (o.extend_penalty < 1 || o.extend_penalty > 15) reject(USAGE_MESSAGE, "shark: --extend-penalty must be in the range [1, 15].");
     }},
    {1029, "extend-bonus", true,
     [](Options &o, const char *v) {
       o.extend_bonus = value_of<unsigned>(v);
       o.extend_sub_flag_given = true;
       if (o.extend_bonus > 15) reject(USAGE_MESSAGE, "shark: --extend-bonus must be in the range [0, 15].");
     }},
    {1030, "pileup-aligned", false, [](Options &o, const char *) { o.pileup_aligned = true; }},
    {1031, "sam-pairs", false, [](Options &o, const char *) { o.sam_pairs = true; }},
    {1032, "fragments", true, [](Options &o, const char *v) { o.fragments_path = value_of<std::string>(v); }},
    {1033, "fragments-max", true,
     [](Options &o, const char *v) {
       o.fragments_max = value_of<unsigned>(v);
       o.fragments_sub_flag_given = true;
     }},
    {1034, "fragments-bins", true,
     [](Options &o, const char *v) {
       o.fragments_bins = value_of<unsigned>(v);
       o.fragments_sub_flag_given = true;
       if (o.fragments_bins < 2 || o.fragments_bins > 4096) reject(USAGE_MESSAGE, "shark: --fragments-bins must be 2 to 4096.");
     }},
    {1035, "fragments-min-intron", true,
     [](Options &o, const char *v) {
       o.fragments_min_intron = value_of<unsigned>(v);
       o.fragments_sub_flag_given = true;
       if (o.fragments_min_intron < 1) reject(USAGE_MESSAGE, "shark: --fragments-min-intron must be at least 1.");
     }},
    {1036, "sam-rescue", false, [](Options &o, const char *) { o.sam_rescue = true; }},
    {1037, "rescue-max-cost", true,
     [](Options &o, const char *v) {
       o.rescue_max_cost = value_of<unsigned>(v);
       o.rescue_sub_flag_given = true;
       if (o.rescue_max_cost > 255) reject(USAGE_MESSAGE, "shark: --rescue-max-cost must be 0 to 255.");
     }},
    {1038, "rescue-min-gap", true,
     [](Options &o, const char *v) {
       o.rescue_min_gap = value_of<unsigned>(v);
       o.rescue_sub_flag_given = true;
       if (o.rescue_min_gap > 255) reject(USAGE_MESSAGE, "shark: --rescue-min-gap must be 0 to 255.");
     }},
    {1039, "splice-junctions", true, [](Options &o, const char *v) { o.splice_path = value_of<std::string>(v); }},
    {1040, "splice-min-mates", true,
     [](Options &o, const char *v) {
       o.splice_min_mates = value_of<unsigned>(v);
       o.splice_sub_flag_given = true;
     }},
    {1041, "splice-min-overhang", true,
     [](Options &o, const char *v) {
       o.splice_min_overhang = value_of<unsigned>(v);
       o.splice_sub_flag_given = true;
       if (o.splice_min_overhang < 1 || o.splice_min_overhang > SHK_SPLICE_MAX_OVERHANG) reject(USAGE_MESSAGE, "shark: --splice-min-overhang must be 1 to 48.");
     }},
    {1042, "splice-max-cost", true,
     [](Options &o, const char *v) {
       o.splice_max_cost = value_of<unsigned>(v);
       o.splice_sub_flag_given = true;
       if (o.splice_max_cost > 64) reject(USAGE_MESSAGE, "shark: --splice-max-cost must be 0 to 64.");
     }},
    {1043, "splice-min-gap", true,
     [](Options &o, const char *v) {
       o.splice_min_gap = value_of<unsigned>(v);
       o.splice_sub_flag_given = true;
       if (o.splice_min_gap > 64) reject(USAGE_MESSAGE, "shark: --splice-min-gap must be 0 to 64.");
     }},
    {1044, "indels", true, [](Options &o, const char *v) { o.indels_path = value_of<std::string>(v); }},
    {1045, "indels-min-support", true,
     [](Options &o, const char *v) {
       o.indels_min_support = value_of<unsigned>(v);
       o.indels_sub_flag_given = true;
       if (o.indels_min_support < 1) reject(USAGE_MESSAGE, "shark: --indels-min-support must be at least 1.");
     }},
    {1046, "indels-min-intron", true,
     [](Options &o, const char *v) {
       o.indels_min_intron = value_of<unsigned>(v);
       o.indels_sub_flag_given = true;
       if (o.indels_min_intron < 1 || o.indels_min_intron > 65535) reject(USAGE_MESSAGE, "shark: --indels-min-intron must be 1 to 65535.");
     }},
    {1047, "indels-min-mates", true,
     [](Options &o, const char *v) {
       o.indels_min_mates = value_of<unsigned>(v);
       o.indels_sub_flag_given = true;
     }},
    {1048, "indels-capacity", true,
     [](Options &o, const char *v) {
       o.indels_capacity = value_of<uint64_t>(v);
       o.indels_sub_flag_given = true;
       if (o.indels_capacity < 1 || o.indels_capacity > (1ull << 32)) reject(USAGE_MESSAGE, "shark: --indels-capacity must be in the range [1, 4294967296].");
     }},
};

// Reads per device batch when --batch does not say.  A batch costs the device path 0.5-2 ms of launches, copies and bookkeeping
// whatever its size, and the ring of batch buffers (two dozen of them) is paid for in page faults at the start and at exit:
// 64 M pairs, 2 % on-target, sample phase 0.63 s at 65 536 pairs per batch, 0.47 s at 262 144, 0.44 s at 524 288; end to end 64 M
// pairs want 262 144 (half the sample written out again: 3.33 -> 2.75 s), 16 M pairs 65 536 (0.42 s against 0.52 s), compressed
// samples, whose size in records nobody knows up front, 65 536 (8 M pairs: 0.74 s against 0.88 s).  So: by the sample's size in
// records, estimated from the first record of a plain file.
inline uint64_t auto_batch(const std::string &sample1, uint64_t fallback)
{
  // (a regular file only: reading the head of a pipe would take it away from the reader)
  struct stat st;
  if (stat(sample1.c_str(), &st) != 0 || !S_ISREG(st.st_mode)) return fallback;
  FILE *f = fopen(sample1.c_str(), "rb");
  if (!f) return fallback;
  std::vector<char> head(1u << 16);
  const size_t got = fread(head.data(), 1, head.size(), f);
  uint64_t size = 0;
  if (fseeko(f, 0, SEEK_END) == 0) size = (uint64_t)ftello(f);
  fclose(f);
  if (got < 2 || ((unsigned char)head[0] == 0x1f && (unsigned char)head[1] == 0x8b)) return fallback;
  size_t rec = 0;
  int lines = 0;
  for (size_t i = 0; i < got && lines < 4; ++i)
    if (head[i] == '\n' && ++lines == 4) rec = i + 1;
  if (!rec) return fallback;
  const uint64_t records = size / rec;
  return records >= 48000000ull ? (1u << 18) : (records >= 24000000ull ? (1u << 17) : fallback);
}

Options parse_arguments(int argc, char **argv)
{
  // getopt_long's two descriptions are generated from the table
  std::string shorts;
  std::vector<struct option> longs;
  for (const OptionRow &row : OPTION_TABLE) {
    if (row.key < 256) {
      shorts.push_back((char)row.key);
      if (row.takes_value) shorts.push_back(':');
    }
    longs.push_back({row.name, row.takes_value ? required_argument : no_argument, nullptr, row.key});
  }
  longs.push_back({nullptr, 0, nullptr, 0});

  Options opt;
  int key;
  while ((key = getopt_long(argc, argv, shorts.c_str(), longs.data(), nullptr)) != -1) {
    const OptionRow *hit = nullptr;
    for (const OptionRow &row : OPTION_TABLE)
      if (row.key == key) hit = &row;
    if (!hit) {
      std::cerr << "shark : unknown argument" << std::endl << "\n" << USAGE_MESSAGE;
      exit(EXIT_FAILURE);
    }
    hit->apply(opt, optarg);
  }
  if (opt.fasta_path.empty() || opt.sample1_path.empty()) {
    std::cerr << "shark : missing required files" << std::endl << "\n" << USAGE_MESSAGE;
    exit(EXIT_FAILURE);
  }
  if (opt.candidates_n_given && opt.candidates_path.empty()) reject(USAGE_MESSAGE, "shark: --candidates-n needs --candidates FILE.");
  if (opt.depth_spliced && opt.depth_path.empty()) reject(USAGE_MESSAGE, "shark: --depth-spliced needs --depth FILE.");
  if (opt.junctions_device && opt.junctions_path.empty()) reject(USAGE_MESSAGE, "shark: --junctions-device needs --junctions FILE.");
  if (opt.junctions_capacity_given && !opt.junctions_device) reject(USAGE_MESSAGE, "shark: --junctions-capacity needs --junctions-device.");
  if (opt.junctions_device && opt.segments_max < SHK_MAX_SEGMENTS) reject(USAGE_MESSAGE, "shark: --junctions-device needs --segments-max 4 (the device's table is defined at 4 diagonals per mate).");
  if (opt.pileup_min_support_given && opt.pileup_path.empty()) reject(USAGE_MESSAGE, "shark: --pileup-min-support needs --pileup FILE.");
  if (opt.variants_sub_flag_given && opt.variants_path.empty()) reject(USAGE_MESSAGE, "shark: --variants-min-support, --variants-min-depth, --variants-min-alt and --variants-min-frac need --variants FILE.");
  if (!opt.variants_path.empty() && !opt.pileup_path.empty() && opt.variants_min_support != opt.pileup_min_support)
    reject(USAGE_MESSAGE, "shark: --variants-min-support and --pileup-min-support must be equal (there is one pileup).");
  if (opt.indels_sub_flag_given && opt.indels_path.empty())
    reject(USAGE_MESSAGE, "shark: --indels-min-support, --indels-min-intron, --indels-min-mates and --indels-capacity need --indels FILE.");
  if (opt.sam_sub_flag_given && opt.sam_path.empty()) reject(USAGE_MESSAGE, "shark: --sam-min-support and --sam-min-intron need --sam FILE.");
  if (opt.sam_pairs && opt.sam_path.empty()) reject(USAGE_MESSAGE, "shark: --sam-pairs needs --sam FILE.");
  if (opt.sam_rescue && opt.sam_path.empty()) reject(USAGE_MESSAGE, "shark: --sam-rescue needs --sam FILE.");
  if (opt.rescue_sub_flag_given && !opt.sam_rescue) reject(USAGE_MESSAGE, "shark: --rescue-max-cost and --rescue-min-gap need --sam-rescue.");
  if (opt.fragments_sub_flag_given && opt.fragments_path.empty() && !opt.sam_pairs && !opt.sam_rescue)
    reject(USAGE_MESSAGE, "shark: --fragments-max, --fragments-bins and --fragments-min-intron need --fragments FILE (or --sam FILE --sam-pairs).");
  if (opt.fragments_min_intron == 0) opt.fragments_min_intron = opt.sam_min_intron;
  if ((opt.sam_pairs || !opt.fragments_path.empty()) && opt.fragments_min_intron < 1)
    reject(USAGE_MESSAGE, "shark: --sam-pairs and --fragments need an intron length of at least 1 (--sam-min-intron, --fragments-min-intron).");
  if (opt.sam_rescue && (opt.fragments_max < 1 || opt.fragments_max > 4096)) reject(USAGE_MESSAGE, "shark: --sam-rescue needs --fragments-max of 1 to 4096.");
  if (opt.sam_rescue && opt.fragments_min_intron < 1)
    reject(USAGE_MESSAGE, "shark: --sam-rescue needs an intron length of at least 1 (--sam-min-intron, --fragments-min-intron).");
  if (opt.pileup_aligned && opt.pileup_path.empty() && opt.variants_path.empty()) reject(USAGE_MESSAGE, "shark: --pileup-aligned needs --pileup FILE or --variants FILE.");
  if (opt.splice_sub_flag_given && opt.splice_path.empty())
    reject(USAGE_MESSAGE, "shark: --splice-min-mates, --splice-min-overhang, --splice-max-cost and --splice-min-gap need --splice-junctions FILE.");
  if (!opt.splice_path.empty() && opt.sam_path.empty() && !opt.pileup_aligned && opt.indels_path.empty()) reject(USAGE_MESSAGE, "shark: --splice-junctions needs --sam FILE or --pileup-aligned (or --indels FILE).");
  if (opt.extend_sub_flag_given && !opt.extend_ends) reject(USAGE_MESSAGE, "shark: --extend-penalty and --extend-bonus need --extend-ends.");
  if (opt.extend_ends && opt.sam_path.empty() && !opt.pileup_aligned && opt.indels_path.empty()) reject(USAGE_MESSAGE, "shark: --extend-ends needs --sam FILE or --pileup-aligned (or --indels FILE).");
  if (opt.out1_path.empty()) opt.out1_path = "sharked_sample.1";
  if (opt.out2_path.empty() && !opt.sample2_path.empty()) opt.out2_path = "sharked_sample.2";
  // --devices alone says how many workers there are; with --gpus N it has to name N devices
  if (!opt.devices.empty()) {
    if (!opt.gpus_given) opt.gpus = (int)opt.devices.size();
    if ((size_t)opt.gpus != opt.devices.size()) reject("", "shark: --devices must name as many devices as --gpus says.");
  } else {
    for (int g = 0; g < opt.gpus; ++g) opt.devices.push_back(g);
  }
  return opt;
}

// progress lines on stderr in the reference's format (main.cpp:49-54; whole seconds since start)
class Progress {
 public:
  void operator()(const std::string &stage) const
  {
    const auto secs = std::chrono::duration_cast<std::chrono::seconds>(std::chrono::steady_clock::now() - t0_).count();
    std::cerr << "[shark/" << stage << "] Time elapsed " << secs << std::endl;
  }

 private:
  std::chrono::steady_clock::time_point t0_ = std::chrono::steady_clock::now();
};
const Progress pelapsed;

// -v: a millisecond timeline of the run's phases on stderr (stderr is not part of the contract)
class Timeline {
 public:
  void on() { on_ = true; }
  void operator()(const char *what)
  {
    if (!on_) return;
    const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0_).count();
    const double epoch = std::chrono::duration<double>(std::chrono::system_clock::now().time_since_epoch()).count();
    std::lock_guard<std::mutex> l(m_);
    std::cerr << "[shark/ms] " << what << " " << ms << " (epoch " << std::fixed << epoch << std::defaultfloat << ")" << std::endl;
    // (SHARK_TRACE_RSS=1: the resident anonymous memory beside every stage -- what holds how much when)
    static const bool rss = getenv("SHARK_TRACE_RSS") != nullptr;
    if (rss) {
      std::ifstream st("/proc/self/status");
      std::string line;
      while (std::getline(st, line))
        if (line.compare(0, 8, "RssAnon:") == 0) std::cerr << "[shark/rss] " << what << " " << line.substr(8) << std::endl;
    }
  }

 private:
  std::chrono::steady_clock::time_point t0_ = std::chrono::steady_clock::now();
  bool on_ = false;
  std::mutex m_;
};
Timeline timeline;

// ---- one batch of reads, structure of arrays ---------------------------------
// allocator that leaves chars uninitialised on resize (the fillers overwrite every byte); large blocks on huge pages
template <typename T>
using default_init_allocator = shk::NoInitAlloc<T>;

// Batch buffers are page-locked once the HIP runtime is up (shk_alloc_pinned: 0.07 s per GB, tools/pin_cost.py; a recycled batch
// keeps its buffers); those allocated earlier -- the readers start while the runtime initialises -- are ordinary memory.
std::atomic<bool> g_pin_batches{false};

template <typename T>
struct pinned_allocator {
  using value_type = T;
  pinned_allocator() = default;
  template <typename U> pinned_allocator(const pinned_allocator<U> &) {}
  template <typename U> struct rebind { using other = pinned_allocator<U>; };
  T *allocate(size_t n)
  {
    // header word in front of the block: 1 = pinned, 0 = malloc
    const size_t bytes = n * sizeof(T) + 64;
    char *raw = g_pin_batches.load(std::memory_order_relaxed) ? static_cast<char *>(shk_alloc_pinned(bytes)) : nullptr;
    bool pinned = raw != nullptr;
    if (!raw) raw = static_cast<char *>(shk::big_alloc(bytes));
    if (!raw) throw std::bad_alloc();
    *reinterpret_cast<uint64_t *>(raw) = pinned ? 1 : 0;
    return reinterpret_cast<T *>(raw + 64);
  }
  void deallocate(T *p, size_t n)
  {
    char *raw = reinterpret_cast<char *>(p) - 64;
    if (*reinterpret_cast<uint64_t *>(raw)) shk_free_pinned(raw); else shk::big_free(raw, n * sizeof(T) + 64);
  }
  template <typename U> void construct(U *p) noexcept { ::new (static_cast<void *>(p)) U; }
  template <typename U, typename... A> void construct(U *p, A &&...a) { ::new (static_cast<void *>(p)) U(std::forward<A>(a)...); }
  template <typename U> bool operator==(const pinned_allocator<U> &) const { return true; }
  template <typename U> bool operator!=(const pinned_allocator<U> &) const { return false; }
};

template <typename CharAlloc, typename OffAlloc>
struct StringsT {
  std::vector<char, CharAlloc> bytes;
  std::vector<uint64_t, OffAlloc> off{0};
  void push(const char *p, size_t n) { bytes.insert(bytes.end(), p, p + n); off.push_back(bytes.size()); }
  size_t size() const { return off.size() - 1; }
  const char *at(size_t i) const { return bytes.data() + off[i]; }
  size_t len(size_t i) const { return (size_t)(off[i + 1] - off[i]); }
  void reset() { bytes.clear(); off.assign(1, 0); }
  void truncate(size_t keep) { off.resize(keep + 1); bytes.resize(off[keep]); }
};
using Strings = StringsT<default_init_allocator<char>, std::allocator<uint64_t>>;           // read names (host only)
using DevStrings = StringsT<pinned_allocator<char>, pinned_allocator<uint64_t>>;             // what the GPU reads

struct ReadBatch {
  uint64_t index = 0;       // position in the input stream (ordering contract)
  uint64_t first_read = 0;  // global index of its first read
  Strings id1, id2;
  DevStrings seq1, qual1, seq2, qual2;
  // records whose quality string does not have the sequence's length as the reference sees them (C strings: a NUL cuts the
  // sequence short, FastqSplitter.hpp:55,:63; a FASTA-style record has no qualities): the device reads qualities at the
  // sequence offsets, the output (ReadOutput.hpp:44-47) prints the quality string as it was
  std::map<size_t, std::string> qual_as_read1, qual_as_read2;
  // lean batches (the parallel readers', fastq_lean_reader.hpp): only what the GPU reads was copied; names and qualities of the
  // associated reads are fetched from the files again by the output stage
  bool lean = false;
  shk::BatchFilePart part1, part2;
  // compressed samples: the inflated text of this batch's records, per mate (part1.mem / part2.mem point into them); the buffers are
  // handed round between the cutters and the batches, never freed
  std::vector<char, default_init_allocator<char>> text1, text2;
  std::shared_ptr<const struct FormattedBatch> text;   // what the output stage will write for this batch (filled by a formatter thread)
  // result
  std::vector<uint32_t> gene_off;
  std::vector<uint16_t> gene_ids;
  std::vector<shk_read_evidence> evidence;   // (--evidence) one record per read
  std::vector<shk_read_candidates> cand_reads;   // (--candidates) one header per read ...
  std::vector<shk_candidate> cand_entries;       // ... and cand_m entries
  uint32_t cand_m = 0;
  std::vector<shk_placement> placements;         // (--placements) one record per association
  std::vector<uint32_t> seg_keys;                // (--segments, --junctions) two headers per association ...
  std::vector<shk_segment> seg_entries;          // ... and 2 x seg_m entries
  uint32_t seg_m = 0;
  std::vector<shk_mate_alignment> alignments;    // (--sam) two records per association
  std::vector<shk_pair> pairs;                   // (--sam-pairs) one record per association
  std::vector<shk_rescue> rescues;               // (--sam-rescue) likewise
  int rc = 0;
  void reset()
  {
    id1.reset(); id2.reset(); seq1.reset(); qual1.reset(); seq2.reset(); qual2.reset();
    qual_as_read1.clear(); qual_as_read2.clear();
    lean = false;
    text.reset();
    gene_off.clear(); gene_ids.clear(); evidence.clear(); cand_reads.clear(); cand_entries.clear(); cand_m = 0; placements.clear();
    seg_keys.clear(); seg_entries.clear(); seg_m = 0;
    alignments.clear();
    pairs.clear();
    rescues.clear();
    rc = 0;
  }
};

// Batches are recycled.  Once the HIP runtime is up the pool becomes a RING of `limit` batches whose bases live in page-locked
// memory: filled once (0.07 s per GB to lock, tools/pin_cost.py), handed round for the whole sample -- their copies to the device
// are DMA at the link's rate, where a copy from ordinary memory makes the runtime lock and unlock the pages every time (which is
// what bounded the CLI's GPU phase: 4.8 GB of bases took 0.3 s on the submitting thread).  A small ring also means a small
// process: leaving it costs the kernel a few milliseconds instead of the 0.15 s it took to free gigabytes of parsed batches.
class BatchPool {
 public:
  // nullptr after shutdown()
  std::unique_ptr<ReadBatch> acquire()
  {
    std::unique_lock<std::mutex> l(m_);
    cv_.wait(l, [&] { return stop_ || !free_.empty() || limit_ == 0 || made_ < limit_; });
    if (stop_) return nullptr;
    if (!free_.empty()) {
      std::unique_ptr<ReadBatch> b = std::move(free_.back());
      free_.pop_back();
      return b;
    }
    ++made_;
    l.unlock();
    return std::unique_ptr<ReadBatch>(new ReadBatch());
  }
  void release(std::unique_ptr<ReadBatch> b)
  {
    b->reset();
    std::lock_guard<std::mutex> l(m_);
    if (limit_ || free_.size() < 64) free_.push_back(std::move(b));
    else --made_;
    cv_.notify_one();
  }
  // from now on at most `limit` batches exist; `reserve_bytes` per mate are page-locked for each right away (by the caller's thread:
  // concurrent page-locking from many threads is several times slower than one thread doing it all)
  void make_ring(size_t limit, size_t reserve_bytes, size_t reserve_reads, bool paired, bool with_qual)
  {
    std::vector<std::unique_ptr<ReadBatch>> fresh;
    for (size_t i = 0; i < limit; ++i) {
      std::unique_ptr<ReadBatch> b(new ReadBatch());
      b->seq1.bytes.reserve(reserve_bytes);
      b->seq1.off.reserve(reserve_reads + 1);
      if (with_qual) b->qual1.bytes.reserve(reserve_bytes);
      if (paired) {
        b->seq2.bytes.reserve(reserve_bytes);
        b->seq2.off.reserve(reserve_reads + 1);
        if (with_qual) b->qual2.bytes.reserve(reserve_bytes);
      }
      fresh.push_back(std::move(b));
    }
    std::lock_guard<std::mutex> l(m_);
    for (auto &b : fresh) free_.push_back(std::move(b));
    made_ += limit;
    limit_ = made_;
    cv_.notify_all();
  }
  void shutdown()
  {
    std::lock_guard<std::mutex> l(m_);
    stop_ = true;
    cv_.notify_all();
  }

 private:
  std::mutex m_;
  std::condition_variable cv_;
  std::vector<std::unique_ptr<ReadBatch>> free_;
  size_t made_ = 0, limit_ = 0;   // limit_ == 0: unbounded
  bool stop_ = false;
};

// FastqSplitter role (FastqSplitter.hpp:47-93): batches of reads in input order.
// Plain four-line FASTQ goes through the block-parallel reader; everything else
// (gzip, multi-line records, CR/LF, ...) through the serial kseq-rule reader.
class BatchSplitter {
 public:
  // (compressed samples: the host threads are shared between the mate files' inflaters)
  BatchSplitter(const Options &o, unsigned threads, BatchPool &pool)
      : r1_(o.sample1_path, std::max(2u, threads / (o.paired_flag ? 2u : 1u))), pool_(pool), paired_(o.paired_flag), maxnum_(o.batch), threads_(threads)
  {
    if (paired_) r2_.reset(new shk::FastxReader(o.sample2_path, std::max(2u, threads / 2u)));
    m1_.reset(new shk::FastqMmap(o.sample1_path, threads));
    if (paired_) m2_.reset(new shk::FastqMmap(o.sample2_path, threads));
    fast_ = m1_->usable() && (!paired_ || m2_->usable()) && !getenv("SHARK_SERIAL_READER");
  }
  bool ok() const { return r1_.ok() && (!paired_ || r2_->ok()); }
  // continue with the serial kseq-rule reader at a record boundary (behind the batches the parallel feed delivered)
  void resume_serial(uint64_t off1, uint64_t off2, uint64_t next_index, uint64_t n_reads)
  {
    fast_ = false;
    r1_.seek(off1);
    if (paired_) r2_->seek(off2);
    next_index_ = next_index;
    n_reads_ = n_reads;
  }
  // continue with the serial kseq-rule reader behind the first `n` records of each mate file (compressed samples whose parallel
  // parse met an irregular record: strict records are the kseq reader's records, so the first n are simply read over)
  void skip_records(uint64_t n, uint64_t next_index)
  {
    fast_ = false;
    auto skip = [n](shk::FastxReader &r) {
      shk::FastxRecord a;
      for (uint64_t i = 0; i < n; ++i)
        if (r.read(a) < 0) break;
    };
    if (paired_) {
      std::thread t2([&] { skip(*r2_); });
      skip(r1_);
      t2.join();
    } else {
      skip(r1_);
    }
    next_index_ = next_index;
    n_reads_ = n;
  }
  std::string stage_report() const
  {
    std::ostringstream o;
    o << "read " << m1_->t_read + (m2_ ? m2_->t_read : 0) << " scan " << m1_->t_scan + (m2_ ? m2_->t_scan : 0) << " merge "
      << m1_->t_merge + (m2_ ? m2_->t_merge : 0) << " validate " << m1_->t_valid + (m2_ ? m2_->t_valid : 0);
    return o.str();
  }
  double t_index = 0, t_fill = 0, t_serial = 0;   // seconds spent (verbose report)
  std::unique_ptr<ReadBatch> operator()()
  {
    std::unique_ptr<ReadBatch> b = pool_.acquire();
    if (!b) return nullptr;
    b->index = next_index_++;
    b->first_read = n_reads_;
    if (fast_) {
      shk::RecordBlock &k1 = blk1_, &k2 = blk2_;   // reused: their buffers keep their capacity
      bool irr1 = false, irr2 = false;
      auto ta = std::chrono::steady_clock::now();
      size_t n = m1_->next_block(maxnum_, k1, irr1);
      if (paired_) n = std::min(n, m2_->next_block(maxnum_, k2, irr2));
      auto tb = std::chrono::steady_clock::now();
      t_index += std::chrono::duration<double>(tb - ta).count();
      if (n) {
        fill(k1, n, b->id1, b->seq1, b->qual1);
        m1_->advance(k1, n);
        if (paired_) {
          fill(k2, n, b->id2, b->seq2, b->qual2);
          m2_->advance(k2, n);
        }
      }
      t_fill += std::chrono::duration<double>(std::chrono::steady_clock::now() - tb).count();
      if (n < maxnum_) {
        // end of a file or an irregular record: the serial reader takes over from here
        fast_ = false;
        if (m1_->at_end() || (paired_ && m2_->at_end())) {
          done_ = true;   // a mate file is exhausted: the reference's read loop ends here too (FastqSplitter.hpp:53,60)
        } else {
          r1_.seek(m1_->cursor());
          if (paired_) r2_->seek(m2_->cursor());
        }
      }
    }
    if (!fast_ && !done_) {
      auto ts = std::chrono::steady_clock::now();
      // the two mate files are parsed (and, for .gz, inflated) by two threads at once; the pair
      // stream ends with the shorter file, as in the reference's read loop (FastqSplitter.hpp:60)
      const size_t have = b->seq1.size(), want = (size_t)maxnum_ - have;
      auto fill_serial = [want](shk::FastxReader &r, Strings &id, DevStrings &seq, DevStrings &qual, std::map<size_t, std::string> &qual_as_read) {
        shk::FastxRecord a;
        size_t got = 0;
        while (got < want && r.read(a) >= 0) {
          // the reference builds std::string from C strings (FastqSplitter.hpp:55,63): stop at NUL
          id.push(a.name.c_str(), strlen(a.name.c_str()));
          const size_t sl = strnlen(a.seq.data(), a.seq.size());
          seq.push(a.seq.data(), sl);
          // The device reads qualities at the sequence offsets.  The reference masks position i only for i < qual.length()
          // (FastqSplitter.hpp:104-109 with the C-string lengths of :55,:63): a record without a quality line, or one cut
          // short by a NUL, is not masked behind the end of its quality string -- those positions get the top quality.
          const size_t qfull = strnlen(a.qual.data(), a.qual.size());
          if (qfull != sl) qual_as_read[seq.size() - 1] = std::string(a.qual.data(), qfull);
          const size_t ql = std::min(sl, qfull);
          a.qual.resize(ql);
          a.qual.resize(sl, '\x7f');
          qual.push(a.qual.data(), sl);
          ++got;
        }
        return got;
      };
      size_t got1 = 0, got2 = 0;
      if (paired_) {
        std::thread t2([&] { got2 = fill_serial(*r2_, b->id2, b->seq2, b->qual2, b->qual_as_read2); });
        got1 = fill_serial(r1_, b->id1, b->seq1, b->qual1, b->qual_as_read1);
        t2.join();
        const size_t keep = have + std::min(got1, got2);
        if (got1 != got2) {   // one file ended: drop the unpaired surplus, nothing more will be read
          b->id1.truncate(keep); b->id2.truncate(keep);
          b->seq1.truncate(keep); b->qual1.truncate(keep); b->seq2.truncate(keep); b->qual2.truncate(keep);
          done_ = true;
        }
      } else {
        got1 = fill_serial(r1_, b->id1, b->seq1, b->qual1, b->qual_as_read1);
      }
      if (got1 < want) done_ = true;
      t_serial += std::chrono::duration<double>(std::chrono::steady_clock::now() - ts).count();
    }
    n_reads_ += b->seq1.size();
    if (b->seq1.size() == 0) { pool_.release(std::move(b)); return nullptr; }
    return b;
  }

 private:
  // copy n strict records into the structure-of-arrays strings, in parallel
  void fill(const shk::RecordBlock &k, size_t n, Strings &id, DevStrings &seq, DevStrings &qual)
  {
    const auto &idl = k.id_len, &sql = k.seq_len;   // measured while the block was validated
    id.off.resize(n + 1);
    seq.off.resize(n + 1);
    qual.off.resize(n + 1);
    uint64_t ai = 0, as = 0;
    for (size_t r = 0; r < n; ++r) {
      id.off[r] = ai; seq.off[r] = as; qual.off[r] = as;
      ai += idl[r]; as += sql[r];
    }
    id.off[n] = ai; seq.off[n] = as; qual.off[n] = as;
    id.bytes.resize(ai);
    seq.bytes.resize(as);
    qual.bytes.resize(as);
    shk::parallel_for(threads_, n, [&](size_t b, size_t e, unsigned) {
      for (size_t r = b; r < e; ++r) {
        memcpy(id.bytes.data() + id.off[r], k.base + k.begin(4 * r) + 1, idl[r]);
        memcpy(seq.bytes.data() + seq.off[r], k.base + k.nl[4 * r] + 1, sql[r]);
        memcpy(qual.bytes.data() + qual.off[r], k.base + k.nl[4 * r + 2] + 1, sql[r]);
      }
    });
  }

  shk::FastxReader r1_;
  BatchPool &pool_;
  std::unique_ptr<shk::FastxReader> r2_;
  std::unique_ptr<shk::FastqMmap> m1_, m2_;
  shk::RecordBlock blk1_, blk2_;
  bool paired_, fast_ = false, done_ = false;
  uint64_t maxnum_;
  unsigned threads_;
  uint64_t next_index_ = 0, n_reads_ = 0;
};

template <typename T>
class BoundedQueue {
 public:
  explicit BoundedQueue(size_t cap) : cap_(cap) {}
  void push(T v)
  {
    std::unique_lock<std::mutex> l(m_);
    cv_space_.wait(l, [&] { return q_.size() < cap_; });
    q_.push_back(std::move(v));
    cv_item_.notify_one();
  }
  bool pop(T &v)
  {
    std::unique_lock<std::mutex> l(m_);
    cv_item_.wait(l, [&] { return !q_.empty() || closed_; });
    if (q_.empty()) return false;
    v = std::move(q_.front());
    q_.pop_front();
    cv_space_.notify_one();
    return true;
  }
  // 1 = got an item, 0 = nothing there right now, -1 = closed and drained
  int try_pop(T &v)
  {
    std::lock_guard<std::mutex> l(m_);
    if (q_.empty()) return closed_ ? -1 : 0;
    v = std::move(q_.front());
    q_.pop_front();
    cv_space_.notify_one();
    return 1;
  }
  void close()
  {
    std::lock_guard<std::mutex> l(m_);
    closed_ = true;
    cv_item_.notify_all();
  }

 private:
  std::mutex m_;
  std::condition_variable cv_item_, cv_space_;
  std::deque<T> q_;
  size_t cap_;
  bool closed_ = false;
};


// ---- compressed samples ------------------------------------------------------------------------------------------------------
// The reference reads a .gz sample through gzread on the parsing thread.  Here the text comes out of the parallel inflaters
// (fastx_reader.hpp: BGZF blocks, or ordinary gzip in two passes, gzip_parallel.hpp) faster than one kseq-rule parser takes it
// (0.7 GB/s per file), so it is parsed like a plain file -- by several threads, sequences only, names and qualities read back
// for the associated reads --, from memory instead of from the file: one CUTTER per mate file takes the inflated text in order,
// counts newlines (32 bytes at a time) and cuts it into pieces of exactly --batch records (four lines each); the pieces of the two
// mates are joined by index and parsed by the parser threads (lean_parse_mem), which is also where a record that is not strict
// four-line FASTQ is noticed: that batch and everything behind it is then read by the serial reader, as for plain files.
struct GzPiece {
  std::vector<char, default_init_allocator<char>> text;
  size_t records = 0;      // whole groups of four lines in `text`
  bool last = false;       // the stream ended behind this piece
};

#if defined(__x86_64__)
__attribute__((target("avx2"))) inline size_t newlines_until_avx2(const char *p, size_t n, uint64_t need, uint64_t &found)
{
  // scans [p, p + n) until `need` newlines have been seen; returns the number of bytes scanned (ends right behind the need-th
  // newline when it is reached), found = newlines in the scanned part
  const __m256i nl = _mm256_set1_epi8('\n');
  size_t i = 0;
  uint64_t c = 0;
  for (; i + 32 <= n; i += 32) {
    const uint32_t m = (uint32_t)_mm256_movemask_epi8(_mm256_cmpeq_epi8(_mm256_loadu_si256(reinterpret_cast<const __m256i *>(p + i)), nl));
    const unsigned k = (unsigned)__builtin_popcount(m);
    if (c + k >= need) {
      uint32_t mm = m;
      for (uint64_t skip = need - c - 1; skip; --skip) mm &= mm - 1;      // drop the newlines in front of the wanted one
      found = need;
      return i + (size_t)__builtin_ctz(mm) + 1;
    }
    c += k;
  }
  for (; i < n; ++i)
    if (p[i] == '\n' && ++c == need) { found = c; return i + 1; }
  found = c;
  return n;
}
#endif
inline size_t newlines_until(const char *p, size_t n, uint64_t need, uint64_t &found)
{
#if defined(__x86_64__)
  if (shk::cpu_has_avx2()) return newlines_until_avx2(p, n, need, found);
#endif
  uint64_t c = 0;
  const char *q = p, *e = p + n;
  while (q < e) {
    const char *x = (const char *)memchr(q, '\n', (size_t)(e - q));
    if (!x) break;
    q = x + 1;
    if (++c == need) { found = c; return (size_t)(q - p); }
  }
  found = c;
  return n;
}

class GzCutter {
 public:
  GzCutter(const std::string &path, unsigned inflate_threads, uint64_t batch) : src_(path, inflate_threads), batch_(batch), q_(3) {}
  ~GzCutter() { stop(); }
  bool ok() const { return src_.ok(); }
  void start() { th_ = std::thread([this] { run(); }); }
  // the next piece in stream order; nullptr behind the last one
  std::unique_ptr<GzPiece> next()
  {
    std::unique_ptr<GzPiece> p;
    if (!q_.pop(p)) return nullptr;
    return p;
  }
  void recycle(std::unique_ptr<GzPiece> p)
  {
    std::lock_guard<std::mutex> l(m_);
    if (free_.size() < 8) free_.push_back(std::move(p));
  }
  // ends the cutter early (a failure elsewhere): whatever it still wants to hand over is dropped
  void stop()
  {
    quit_ = true;
    std::thread drain([this] { std::unique_ptr<GzPiece> p; while (q_.pop(p)) {} });
    if (th_.joinable()) th_.join();
    q_.close();
    drain.join();
  }
  double seconds = 0;   // spent scanning and copying (verbose report)

 private:
  std::unique_ptr<GzPiece> fresh()
  {
    {
      std::lock_guard<std::mutex> l(m_);
      if (!free_.empty()) {
        std::unique_ptr<GzPiece> p = std::move(free_.back());
        free_.pop_back();
        p->text.clear();
        p->records = 0;
        p->last = false;
        return p;
      }
    }
    return std::unique_ptr<GzPiece>(new GzPiece());
  }
  void run()
  {
    std::unique_ptr<GzPiece> cur = fresh();
    uint64_t lines = 0;                 // newlines in cur
    const uint64_t per = 4 * batch_;
    const char *d;
    size_t n;
    char last_byte = '\n';
    while (!quit_ && src_.next(d, n)) {
      auto t0 = std::chrono::steady_clock::now();
      size_t at = 0;
      while (at < n && !quit_) {
        uint64_t found = 0;
        const size_t used = newlines_until(d + at, n - at, per - lines, found);
        const size_t o = cur->text.size();
        cur->text.resize(o + used);
        memcpy(cur->text.data() + o, d + at, used);
        at += used;
        lines += found;
        if (lines == per) {
          cur->records = batch_;
          seconds += std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
          q_.push(std::move(cur));
          t0 = std::chrono::steady_clock::now();
          cur = fresh();
          lines = 0;
        }
      }
      if (n) last_byte = d[n - 1];
      seconds += std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    }
    if (!quit_) {
      // a last record without its newline is a record all the same (kseq.h reads the quality up to the end of the file)
      if (!cur->text.empty() && last_byte != '\n') { cur->text.push_back('\n'); ++lines; }
      cur->records = (size_t)(lines / 4);
      cur->last = true;
      q_.push(std::move(cur));
    }
    q_.close();
  }
  shk::InflateAhead src_;
  uint64_t batch_;
  BoundedQueue<std::unique_ptr<GzPiece>> q_;
  std::mutex m_;
  std::vector<std::unique_ptr<GzPiece>> free_;
  std::atomic<bool> quit_{false};
  std::thread th_;
};

// ReadAnalyzer role (ReadAnalyzer.hpp:39-110): reads -> associations, on one GPU.  Up to SHK_PIPE_DEPTH batches are in
// flight: the copies of the next batches overlap the kernels of the current one (shk_classify_submit / _wait).
class ReadAnalyzer {
 public:
  ReadAnalyzer(shk_ctx *ctx, bool need_qual, bool evidence, bool candidates = false, bool placements = false, bool segments = false, bool alignments = false,
               bool pairs = false, bool rescue = false)
      : ctx_(ctx), need_qual_(need_qual), evidence_(evidence), candidates_(candidates), placements_(placements), segments_(segments), alignments_(alignments),
        pairs_(pairs), rescue_(rescue) {}
  // false: the batch failed at once (b.rc is set) and is not in flight
  bool submit(std::unique_ptr<ReadBatch> b)
  {
    shk_batch in{};
    in.n = b->seq1.size();
    in.seq1 = b->seq1.bytes.data();
    in.off1 = b->seq1.off.data();
    if (b->seq2.size() == in.n && (b->lean || b->id2.size() == in.n) && in.n) {
      in.seq2 = b->seq2.bytes.data();
      in.off2 = b->seq2.off.data();
    }
    if (need_qual_) {
      // quality strings share the sequence offsets (kseq.h:216 guarantees equal lengths; the serial reader pads the rest)
      in.qual1 = b->qual1.bytes.data();
      if (in.seq2) in.qual2 = b->qual2.bytes.data();
    }
    uint64_t ticket = 0;
    b->rc = shk_classify_submit(ctx_, &in, &ticket);
    const bool ok = b->rc == SHK_OK;
    if (ok) flying_.emplace_back(ticket, std::move(b)); else failed_ = std::move(b);
    return ok;
  }
  size_t in_flight() const { return flying_.size(); }
  std::unique_ptr<ReadBatch> take_failed() { return std::move(failed_); }
  // the oldest batch in flight, classified
  std::unique_ptr<ReadBatch> wait()
  {
    std::unique_ptr<ReadBatch> b = std::move(flying_.front().second);
    const uint64_t ticket = flying_.front().first;
    flying_.pop_front();
    shk_result out{};
    b->rc = shk_classify_wait(ctx_, ticket, &out);
    if (b->rc == SHK_OK) {
      b->gene_off.assign(out.gene_off, out.gene_off + out.n + 1);
      b->gene_ids.assign(out.gene_ids, out.gene_ids + out.n_assoc);
      if (evidence_) {
        shk_evidence ev{};
        b->rc = shk_evidence_last(ctx_, &ev);
        if (b->rc == SHK_OK) b->evidence.assign(ev.reads, ev.reads + ev.n);
      }
      if (candidates_ && b->rc == SHK_OK) {
        shk_candidates cd{};
        b->rc = shk_candidates_last(ctx_, &cd);
        if (b->rc == SHK_OK) {
          b->cand_m = cd.m;
          b->cand_reads.assign(cd.reads, cd.reads + cd.n);
          b->cand_entries.assign(cd.entries, cd.entries + cd.n * cd.m);
        }
      }
      if (placements_ && b->rc == SHK_OK) {
        shk_placements pl{};
        b->rc = shk_placement_last(ctx_, &pl);
        if (b->rc == SHK_OK) b->placements.assign(pl.entries, pl.entries + pl.n_assoc);
      }
      if (segments_ && b->rc == SHK_OK) {
        shk_segments sg{};
        b->rc = shk_segments_last(ctx_, &sg);
        if (b->rc == SHK_OK) {
          b->seg_m = sg.m;
          b->seg_keys.assign(sg.n_keys, sg.n_keys + 2 * sg.n_assoc);
          b->seg_entries.assign(sg.entries, sg.entries + 2 * sg.n_assoc * sg.m);
        }
      }
      if (alignments_ && b->rc == SHK_OK) {
        shk_alignments al{};
        b->rc = shk_alignments_last(ctx_, &al);
        if (b->rc == SHK_OK) b->alignments.assign(al.entries, al.entries + 2 * al.n_assoc);
      }
      if (pairs_ && b->rc == SHK_OK) {
        shk_pairs pr{};
        b->rc = shk_pairs_last(ctx_, &pr);
        if (b->rc == SHK_OK) b->pairs.assign(pr.entries, pr.entries + pr.n_assoc);
      }
      if (rescue_ && b->rc == SHK_OK) {
        shk_rescues rs{};
        b->rc = shk_rescue_last(ctx_, &rs);
        if (b->rc == SHK_OK) b->rescues.assign(rs.entries, rs.entries + rs.n_assoc);
      }
    }
    return b;
  }

 private:
  shk_ctx *ctx_;
  bool need_qual_, evidence_, candidates_, placements_, segments_, alignments_, pairs_, rescue_;
  std::deque<std::pair<uint64_t, std::unique_ptr<ReadBatch>>> flying_;
  std::unique_ptr<ReadBatch> failed_;
};

// ReadOutput role (ReadOutput.hpp:37-50).  The reference starts a new output
// call -- and clears previd -- every 50 000 input reads (main.cpp:215,
// ReadOutput.hpp:39), so 50 000-read chunks are independent and are formatted
// in parallel; the text is then written in input order.
// An output FASTQ file written at explicit offsets: the thread that emits the batches in order only assigns each piece its
// place in the file; the bytes are written by a few helper threads (pwrite), so an on-target-heavy sample -- gigabytes of output
// FASTQ -- is not throttled by one thread's write calls.  Not seekable (a pipe, a terminal): written in place, in order.
class OffsetWriter {
 public:
  OffsetWriter() = default;
  // (every error return of run_sample() that runs while a writer is in scope comes through here: the helper threads are joined, never
  // destroyed while joinable -- that would be std::terminate instead of the exit code the caller was promised)
  ~OffsetWriter() { (void)close(); }
  OffsetWriter(const OffsetWriter &) = delete;
  OffsetWriter &operator=(const OffsetWriter &) = delete;
  bool open(const std::string &path, unsigned helpers)
  {
    fd_ = ::open(path.c_str(), O_WRONLY | O_CREAT | O_TRUNC, 0666);
    if (fd_ < 0) return false;
    seekable_ = lseek(fd_, 0, SEEK_CUR) != (off_t)-1;
    if (seekable_)
      for (unsigned i = 0; i < std::max(1u, helpers); ++i) th_.emplace_back([this] { work(); });
    return true;
  }
  bool is_open() const { return fd_ >= 0; }
  // `keep` keeps the bytes alive until they are written
  void append(const char *p, size_t n, const std::shared_ptr<const void> &keep)
  {
    if (!n) return;
    if (!seekable_) { write_all(p, n, (uint64_t)-1); return; }
    {
      std::unique_lock<std::mutex> l(m_);
      space_.wait(l, [&] { return q_.size() < 256; });   // (the text of at most that many pieces waits to be written)
      q_.push_back(Job{p, n, off_, keep});
    }
    off_ += n;
    cv_.notify_one();
  }
  bool close()
  {
    {
      std::lock_guard<std::mutex> l(m_);
      closing_ = true;
    }
    cv_.notify_all();
    for (auto &t : th_) t.join();
    th_.clear();
    const bool ok = !failed_.load() && (fd_ < 0 || ::close(fd_) == 0);
    fd_ = -1;
    return ok;
  }

 private:
  struct Job { const char *p; size_t n; uint64_t off; std::shared_ptr<const void> keep; };
  void write_all(const char *p, size_t n, uint64_t off)
  {
    while (n) {
      const ssize_t w = off == (uint64_t)-1 ? ::write(fd_, p, n) : ::pwrite(fd_, p, n, (off_t)off);
      if (w <= 0) { failed_ = true; return; }
      p += w; n -= (size_t)w;
      if (off != (uint64_t)-1) off += (uint64_t)w;
    }
  }
  void work()
  {
    for (;;) {
      Job j;
      {
        std::unique_lock<std::mutex> l(m_);
        cv_.wait(l, [&] { return !q_.empty() || closing_; });
        if (q_.empty()) return;
        j = std::move(q_.front());
        q_.pop_front();
        space_.notify_one();
      }
      const auto t0 = std::chrono::steady_clock::now();
      write_all(j.p, j.n, j.off);
      j.keep.reset();                                    // (the text's last owner frees it here, on this thread)
      busy_ns_ += (uint64_t)std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::steady_clock::now() - t0).count();
      bytes_ += j.n;
    }
  }
 public:
  // (-v) bytes written by the helper threads and the seconds they spent writing and freeing
  uint64_t bytes_written() const { return bytes_.load(); }
  double busy_seconds() const { return 1e-9 * (double)busy_ns_.load(); }
 private:
  std::atomic<uint64_t> bytes_{0}, busy_ns_{0};
  int fd_ = -1;
  bool seekable_ = false, closing_ = false;
  uint64_t off_ = 0;
  std::atomic<bool> failed_{false};
  std::mutex m_;
  std::condition_variable cv_, space_;
  std::deque<Job> q_;
  std::vector<std::thread> th_;
};

// The text is produced per batch by any thread, in any order (format); the batches are then written in input order
// (emit), which is also where the one thing that crosses a batch boundary is settled: whether the first associated read
// of a batch that starts in the middle of a 50 000-read chunk repeats the previous batch's last read name.
struct JunctionHit { uint32_t gene; int64_t donor, acceptor, intron; };   // (--junctions) one mate's one junction
struct FormattedSegment {
  std::string ssv, fq1, fq2;        // fq: the FASTQ records behind the segment's first one
  std::string evd;                  // (--evidence) <id> <cov> <nk> <len> of every read of the segment
  std::string cnd;                  // (--candidates) <id> <len> <n_genes> { <gene> <cov> <nk>} of every read of the segment
  std::string plc;                  // (--placements) <id> <gene> <strand> <pos> <support> [mate 2's three] of every association of the segment
  std::string sgm;                  // (--segments) <id> <gene> and per mate <n_keys> and m x <strand> <pos> <support> <first> <last>, per association
  std::string sam;                  // (--sam) one SAM line per association and mate with a block
  std::vector<JunctionHit> jnc;     // (--junctions) the junctions of the segment's mates, added to the run's table when the segment is written
  std::string head1, head2;         // the first associated read's FASTQ records, printed unless its name equals the carried one
  std::string head_id, last_id;
  bool has_assoc = false, carries = false;
  void reset()
  {
    ssv.clear(); fq1.clear(); fq2.clear(); evd.clear(); cnd.clear(); plc.clear(); sgm.clear(); sam.clear(); jnc.clear(); head1.clear(); head2.clear(); head_id.clear(); last_id.clear();
    has_assoc = carries = false;
  }
};
struct FormattedBatch {
  std::vector<FormattedSegment> segs;   // (the first n of them are this batch's; the others keep their strings' memory for the next use)
  size_t n = 0;
};
// The text of a batch lives from its formatter to the writer threads' last write of it; then the object -- its strings keep their
// capacity -- goes back here for a later batch.  (Without the pool every batch's text was fresh memory: 20 GB of page faults on the
// formatter threads and as many pages unmapped by the writer threads, each unmap stopping every thread that faults, for a sample
// half of which is written out again.)  Never more objects than were alive at once.
class TextPool {
 public:
  std::shared_ptr<FormattedBatch> get()
  {
    static const bool off = getenv("SHARK_NO_TEXT_POOL") != nullptr;      // (A/B timing)
    if (off) return std::make_shared<FormattedBatch>();
    FormattedBatch *p = nullptr;
    {
      std::lock_guard<std::mutex> l(st_->m);
      if (!st_->free.empty()) { p = st_->free.back(); st_->free.pop_back(); }
    }
    if (!p) p = new FormattedBatch();
    // (the deleter owns the pool's state: a text may outlive this object on an error return)
    std::shared_ptr<State> st = st_;
    return std::shared_ptr<FormattedBatch>(p, [st](FormattedBatch *q) {
      std::lock_guard<std::mutex> l(st->m);
      st->free.push_back(q);
      st->cv.notify_one();
    });
  }
  // No text will be asked for any more (every batch is formatted): from now on `threads` helpers give the pages of every text
  // that comes back -- and of those that are back already -- to the system at once, side by side (MADV_DONTNEED takes the address
  // space's lock shared; unmapping takes it exclusively).  What the process still holds when it ends, its end has to give back on
  // ONE thread: 0.08 s per GB, 0.7-0.9 s for the 10 GB of a 64 M-pair sample half of which is written out again.
  void retire(unsigned threads)
  {
    for (unsigned t = 0; t < std::max(1u, threads); ++t)
      reapers_.emplace_back([st = st_] {
        for (;;) {
          FormattedBatch *q;
          {
            std::unique_lock<std::mutex> l(st->m);
            st->cv.wait(l, [&] { return !st->free.empty() || st->done; });
            if (st->free.empty()) return;
            q = st->free.back();
            st->free.pop_back();
          }
          for (FormattedSegment &sg : q->segs)
            for (std::string *x : {&sg.ssv, &sg.fq1, &sg.fq2, &sg.evd, &sg.cnd, &sg.plc, &sg.sgm, &sg.sam}) drop_pages(*x);
          // (the object itself and its small strings are left to the process's end)
        }
      });
  }
  // every text is back (the writers are closed): the helpers finish what is left
  void finish()
  {
    {
      std::lock_guard<std::mutex> l(st_->m);
      st_->done = true;
    }
    st_->cv.notify_all();
    for (auto &t : reapers_) t.join();
    reapers_.clear();
  }
  // (an error return in between: the helpers are joined, never destroyed while joinable; the state is left to the process's end)
  ~TextPool() { finish(); new std::shared_ptr<State>(st_); }

 private:
  static void drop_pages(std::string &x)
  {
    if (x.capacity() < (1u << 20)) return;
    const uintptr_t a = ((uintptr_t)x.data() + 4095u) & ~(uintptr_t)4095u, e = ((uintptr_t)x.data() + x.capacity()) & ~(uintptr_t)4095u;
    if (e > a) (void)madvise((void *)a, (size_t)(e - a), MADV_DONTNEED);
  }
  struct State {
    std::mutex m;
    std::condition_variable cv;
    std::vector<FormattedBatch *> free;
    bool done = false;
  };
  std::shared_ptr<State> st_ = std::make_shared<State>();
  std::vector<std::thread> reapers_;
};

class ReadOutput {
 public:
  ReadOutput(OffsetWriter *out1, OffsetWriter *out2, const std::vector<std::string> &legend, FILE *evidence = nullptr, FILE *candidates = nullptr,
             FILE *placements = nullptr, bool paired = false, FILE *segments = nullptr, bool junctions = false, uint32_t k = 0, uint32_t junctions_min_support = 8,
             FILE *sam = nullptr, uint32_t sam_min_intron = 20, bool sam_pairs = false, bool sam_rescue = false)
      : out1_(out1), out2_(out2), legend_(legend), evidence_(evidence), candidates_(candidates), placements_(placements), paired_(paired),
        every_read_(evidence || candidates), segments_(segments), junctions_(junctions), k_(k), s_min_(junctions_min_support),
        sam_(sam), sam_min_intron_(sam_min_intron), sam_pairs_(sam_pairs), sam_rescue_(sam_rescue) {}
  bool failed() const { return failed_.load(); }
  bool evidence_write_failed() const { return failed_write_; }
  bool candidates_write_failed() const { return failed_write_cand_; }
  bool placements_write_failed() const { return failed_write_plc_; }
  bool segments_write_failed() const { return failed_write_sgm_; }
  bool sam_write_failed() const { return failed_write_sam_; }

  // The junctions of one mate of L bytes from its m reported segments (include/shark_hip.h, "segments"): the segments with at least
  // s_min votes on rank 0's strand, sorted by their record span [lo, hi); every consecutive pair whose second diagonal lies further
  // along the record is a junction (donor = hi of the first, acceptor = lo of the second, intron = the diagonals' distance).
  static void mate_junctions(const shk_segment *e, uint32_t m, int64_t L, int64_t k, uint32_t s_min, uint32_t gene, std::vector<JunctionHit> &out)
  {
    struct Span { int64_t lo, hi, pos; } kept[SHK_MAX_SEGMENTS];
    uint32_t n = 0;
    for (uint32_t r = 0; r < m && r < SHK_MAX_SEGMENTS; ++r) {
      if (e[r].support < 1 || e[r].support < s_min || e[r].strand != e[0].strand) continue;
      const int64_t pos = e[r].pos, first = e[r].first, last = e[r].last;
      kept[n++] = e[r].strand == 0 ? Span{pos + first, pos + last + k, pos} : Span{pos + L - k - last, pos + L - first, pos};
    }
    std::stable_sort(kept, kept + n, [](const Span &a, const Span &b) { return a.lo != b.lo ? a.lo < b.lo : a.hi < b.hi; });
    for (uint32_t i = 0; i + 1 < n; ++i)
      if (kept[i + 1].pos > kept[i].pos) out.push_back(JunctionHit{gene, kept[i].hi, kept[i + 1].lo, kept[i + 1].pos - kept[i].pos});
  }
  // --junctions: <gene> <donor> <acceptor> <intron> <mates>, sorted by gene index, donor, acceptor (mates that disagree on the intron
  // of one (gene, donor, acceptor) -- an indel next to the junction --: the smallest)
  bool write_junctions(FILE *f) const
  {
    std::string text;
    for (const auto &kv : junction_table_) {
      const uint32_t g = std::get<0>(kv.first);
      text += g < legend_.size() ? legend_[g] : std::string();
      text += ' '; text += std::to_string(std::get<1>(kv.first));
      text += ' '; text += std::to_string(std::get<2>(kv.first));
      text += ' '; text += std::to_string(kv.second.first);
      text += ' '; text += std::to_string(kv.second.second);
      text += '\n';
    }
    return fwrite(text.data(), 1, text.size(), f) == text.size();
  }

  // thread-safe; nothing is written
  void format(const ReadBatch &b, FormattedBatch &out) const
  {
    const size_t n = b.seq1.size();
    out.n = 0;
    shk::RecordFetcher f1, f2;
    // segments: [first, last) read ranges that do not cross a 50 000 boundary
    for (size_t first = 0; first < n;) {
      const uint64_t g = b.first_read + first;
      const size_t last = (size_t)std::min<uint64_t>(n, first + (50000 - g % 50000));
      if (out.n == out.segs.size()) out.segs.emplace_back();
      FormattedSegment &sg = out.segs[out.n++];
      sg.reset();
      sg.carries = g % 50000 != 0;                  // continues the previous batch's chunk: previd is known only when the batches are written
      std::string previd;
      bool reserved = false;
      if (b.lean) {
        // many associated reads in this segment: its byte range in one read; few: one read per record
        const size_t n_assoc = b.gene_off[last] - b.gene_off[first];
        if (n_assoc * 10 > last - first || every_read_) {     // (--evidence and --candidates name every read)
          f1.load_dense(b.part1, first, last);
          if (out2_ || (sam_ && paired_)) f2.load_dense(b.part2, first, last);
        } else {
          f1.unload();
          f2.unload();
        }
      }
      if (evidence_) sg.evd.reserve((last - first) * 48);
      if (candidates_) sg.cnd.reserve((last - first) * 64);
      for (size_t i = first; i < last; ++i) {
        const bool assoc = b.gene_off[i] != b.gene_off[i + 1];
        if (!assoc && !every_read_) continue;
        shk::RecordFetcher::View v1{nullptr, 0, nullptr, 0, nullptr}, v2{nullptr, 0, nullptr, 0, nullptr};
        const char *id;
        size_t id_len;
        if (b.lean) {
          if (!f1.get(b.part1, i, v1) || (assoc && (out2_ || (sam_ && paired_)) && !f2.get(b.part2, i, v2))) { failed_ = true; continue; }
          id = v1.id;
          id_len = v1.id_len;
        } else {
          id = b.id1.at(i);
          id_len = b.id1.len(i);
        }
        if (evidence_ && b.evidence.size() != n) failed_ = true;      // (a batch without a record per read: an error exit, never a short file)
        if (evidence_ && i < b.evidence.size()) {
          // the read's name as the ssv prints it, then the best gene's coverage and k-mer count and the read's valid length
          char num[48];
          const shk_read_evidence &e = b.evidence[i];
          const int w = snprintf(num, sizeof(num), " %u %u %u\n", e.cov, e.nk, e.len);
          sg.evd.append(id, id_len);
          sg.evd.append(num, (size_t)w);
        }
        if (candidates_ && (b.cand_reads.size() != n || b.cand_entries.size() != n * b.cand_m)) failed_ = true;   // (likewise)
        if (candidates_ && i < b.cand_reads.size() && (i + 1) * (size_t)b.cand_m <= b.cand_entries.size()) {
          // the read's name as the ssv prints it, its valid length, the number of genes it hit, and the filled entries in rank
          // order: the gene as the ssv names it, its coverage and its k-mer count
          char num[48];
          const shk_read_candidates &h = b.cand_reads[i];
          int w = snprintf(num, sizeof(num), " %u %u", h.len, h.n_genes);
          sg.cnd.append(id, id_len);
          sg.cnd.append(num, (size_t)w);
          for (uint32_t r = 0; r < b.cand_m; ++r) {
            const shk_candidate &e = b.cand_entries[i * (size_t)b.cand_m + r];
            if (e.nk == 0) break;
            if (e.gene >= legend_.size()) { failed_ = true; break; }
            sg.cnd.push_back(' ');
            sg.cnd.append(legend_[e.gene]);
            w = snprintf(num, sizeof(num), " %u %u", e.cov, e.nk);
            sg.cnd.append(num, (size_t)w);
          }
          sg.cnd.push_back('\n');
        }
        if (!assoc) continue;
        if (placements_ && b.placements.size() != b.gene_ids.size()) failed_ = true;   // (a batch without a record per association: an error exit)
        if (sam_ && b.alignments.size() != 2 * b.gene_ids.size()) failed_ = true;      // (likewise)
        if (sam_ && sam_pairs_ && b.pairs.size() != b.gene_ids.size()) failed_ = true;  // (likewise)
        if (sam_ && sam_rescue_ && b.rescues.size() != b.gene_ids.size()) failed_ = true;   // (likewise)
        const bool seg_mode = segments_ || junctions_;
        if (seg_mode && (b.seg_m == 0 || b.seg_keys.size() != 2 * b.gene_ids.size() || b.seg_entries.size() != 2 * b.gene_ids.size() * b.seg_m)) failed_ = true;   // (likewise)
        for (uint32_t j = b.gene_off[i]; j < b.gene_off[i + 1]; ++j) {
          const std::string &gene = legend_[b.gene_ids[j]];
          if (placements_ && j < b.placements.size()) {
            // the ssv line's two fields, then per mate the strand, the record coordinate of the mate's leftmost base and the votes
            char num[96];
            const shk_placement &pl = b.placements[j];
            const int w = paired_ ? snprintf(num, sizeof(num), " %u %d %u %u %d %u\n", pl.mate[0].strand, pl.mate[0].pos, pl.mate[0].support,
                                             pl.mate[1].strand, pl.mate[1].pos, pl.mate[1].support)
                                  : snprintf(num, sizeof(num), " %u %d %u\n", pl.mate[0].strand, pl.mate[0].pos, pl.mate[0].support);
            sg.plc.append(id, id_len);
            sg.plc.push_back(' ');
            sg.plc.append(gene);
            sg.plc.append(num, (size_t)w);
          }
          if (seg_mode && b.seg_m && 2 * (size_t)(j + 1) <= b.seg_keys.size() && 2 * (size_t)(j + 1) * b.seg_m <= b.seg_entries.size()) {
            const shk_segment *e = b.seg_entries.data() + 2 * (size_t)j * b.seg_m;
            if (segments_) {
              // the ssv line's two fields, then per mate the number of diagonals and the reported ones in rank order
              char num[96];
              sg.sgm.append(id, id_len);
              sg.sgm.push_back(' ');
              sg.sgm.append(gene);
              for (uint32_t t = 0; t < (paired_ ? 2u : 1u); ++t) {
                int w = snprintf(num, sizeof(num), " %u", b.seg_keys[2 * (size_t)j + t]);
                sg.sgm.append(num, (size_t)w);
                for (uint32_t r = 0; r < b.seg_m; ++r) {
                  const shk_segment &x = e[t * b.seg_m + r];
                  w = snprintf(num, sizeof(num), " %u %d %u %u %u", x.strand, x.pos, x.support, x.first, x.last);
                  sg.sgm.append(num, (size_t)w);
                }
              }
              sg.sgm.push_back('\n');
            }
            if (junctions_) {
              mate_junctions(e, b.seg_m, (int64_t)b.seq1.len(i), k_, s_min_, b.gene_ids[j], sg.jnc);
              if (i < b.seq2.size()) mate_junctions(e + b.seg_m, b.seg_m, (int64_t)b.seq2.len(i), k_, s_min_, b.gene_ids[j], sg.jnc);
            }
          }
          if (sam_ && 2 * (size_t)(j + 1) <= b.alignments.size()) {
            // (--sam) mate 1's line, then mate 2's; a lean batch's qualities come from the file again, as the FASTQ output's do
            const shk_mate_alignment *al = b.alignments.data() + 2 * (size_t)j;
            const shk_pair *pr = sam_pairs_ && (size_t)j < b.pairs.size() ? b.pairs.data() + (size_t)j : nullptr;   // (--sam-pairs)
            const shk_rescue *rs = sam_rescue_ && (size_t)j < b.rescues.size() ? b.rescues.data() + (size_t)j : nullptr;   // (--sam-rescue)
            for (uint32_t t = 0; t < (paired_ ? 2u : 1u); ++t) {
              if (al[t].n_blocks == 0) continue;
              const DevStrings &seq = t ? b.seq2 : b.seq1, &qual = t ? b.qual2 : b.qual1;
              const std::map<size_t, std::string> &odd = t ? b.qual_as_read2 : b.qual_as_read1;
              if (i >= seq.size()) { failed_ = true; continue; }
              const char *q = nullptr;      // (nullptr: no quality string of the sequence's length -- FASTA input)
              if (b.lean) q = t ? v2.qual : v1.qual;
              else if (i < qual.size() && qual.len(i) == seq.len(i) && odd.find(i) == odd.end()) q = qual.at(i);
              if (!sam_line(sg.sam, id, id_len, gene, j > b.gene_off[i], paired_, t, al[t], al[1 - t], seq.at(i), seq.len(i), q, sam_min_intron_, pr,
                            rs && rs->state == 4u + t ? rs : nullptr))
                failed_ = true;
            }
          }
          sg.ssv.append(id, id_len);
          sg.ssv.push_back(' ');
          sg.ssv.append(gene);
          sg.ssv.push_back('\n');
          const bool head = !sg.has_assoc;            // the segment's first association
          const bool same = !(head && sg.carries) && previd.size() == id_len && memcmp(previd.data(), id, id_len) == 0;
          if (!same) {
            std::string &o1 = (head && sg.carries) ? sg.head1 : sg.fq1, &o2 = (head && sg.carries) ? sg.head2 : sg.fq2;
            if (b.lean) {
              if (out1_) record_view(o1, v1);
              if (out2_) record_view(o2, v2);
            } else {
              if (out1_) record(o1, b.id1, b.seq1, b.qual1, b.qual_as_read1, i);
              if (out2_) record(o2, b.id2, b.seq2, b.qual2, b.qual_as_read2, i);
            }
            // (the segment's text in one allocation: by its first record and the reads it has left -- a string that doubles its way
            //  to 8 MB copies itself twice over and page-faults every step)
            if (!reserved && &o1 == &sg.fq1) {
              reserved = true;
              size_t left = 0;
              for (size_t r = i; r < last; ++r) left += b.gene_off[r] != b.gene_off[r + 1];
              if (out1_) sg.fq1.reserve(sg.fq1.size() * left + (sg.fq1.size() * left >> 4) + 64);
              if (out2_) sg.fq2.reserve(sg.fq2.size() * left + (sg.fq2.size() * left >> 4) + 64);
              sg.ssv.reserve(sg.ssv.size() * left + (sg.ssv.size() * left >> 3) + 64);
            }
          }
          if (head) sg.head_id.assign(id, id_len);
          previd.assign(id, id_len);
          sg.has_assoc = true;
        }
      }
      sg.last_id = previd;
      first = last;
    }
  }

  // in input order, one thread
  void emit(const std::shared_ptr<const FormattedBatch> &fp)
  {
    const FormattedBatch &f = *fp;
    for (size_t si = 0; si < f.n; ++si) {
      const FormattedSegment &sg = f.segs[si];
      fwrite(sg.ssv.data(), 1, sg.ssv.size(), stdout);
      if (evidence_ && fwrite(sg.evd.data(), 1, sg.evd.size(), evidence_) != sg.evd.size()) failed_write_ = true;
      if (candidates_ && fwrite(sg.cnd.data(), 1, sg.cnd.size(), candidates_) != sg.cnd.size()) failed_write_cand_ = true;
      if (placements_ && fwrite(sg.plc.data(), 1, sg.plc.size(), placements_) != sg.plc.size()) failed_write_plc_ = true;
      if (segments_ && fwrite(sg.sgm.data(), 1, sg.sgm.size(), segments_) != sg.sgm.size()) failed_write_sgm_ = true;
      if (sam_ && fwrite(sg.sam.data(), 1, sg.sam.size(), sam_) != sg.sam.size()) failed_write_sam_ = true;
      for (const JunctionHit &h : sg.jnc) {
        auto it = junction_table_.emplace(std::make_tuple(h.gene, h.donor, h.acceptor), std::make_pair(h.intron, (uint64_t)0)).first;
        it->second.first = std::min(it->second.first, h.intron);
        ++it->second.second;
      }
      // (ReadOutput.hpp:44-48: a read's FASTQ records are printed unless its name equals the one printed just before it)
      const bool head_repeats = sg.carries && sg.has_assoc && sg.head_id == carry_;
      if (out1_) {
        if (!head_repeats) out1_->append(sg.head1.data(), sg.head1.size(), fp);
        out1_->append(sg.fq1.data(), sg.fq1.size(), fp);
      }
      if (out2_) {
        if (!head_repeats) out2_->append(sg.head2.data(), sg.head2.size(), fp);
        out2_->append(sg.fq2.data(), sg.fq2.size(), fp);
      }
      carry_ = sg.has_assoc ? sg.last_id : (sg.carries ? carry_ : std::string());
    }
  }

 private:
  // One line of --sam (include/shark_hip.h, "alignments"): `a` is this mate's record, `other` the same association's
  // other mate's.  CIGAR and NM are shk_alignment_cigar's; SEQ and QUAL are the mate's bytes in the record's orientation.
  // false: the record does not fit a mate of L bytes (the library's answer is inconsistent: an error exit, never a wrong line).
  // pair (--sam-pairs; nullptr without): the association's pair record (include/shark_hip.h, "pairs") -- MAPQ is its mapq, 0x2
  // is set iff proper, TLEN is tend - tstart on the left mate's line and its negative on the other's for classes 3, 4 and 5.
  // rescued (--sam-rescue; nullptr for a mate that was not rescued): the association's rescue record -- YR:i:<cost> behind NM:i:.
  static bool sam_line(std::string &f, const char *id, size_t id_len, const std::string &gene, bool secondary, bool paired, uint32_t t,
                       const shk_mate_alignment &a, const shk_mate_alignment &other, const char *seq, size_t L, const char *qual, uint32_t min_intron,
                       const shk_pair *pair = nullptr, const shk_rescue *rescued = nullptr)
  {
    // (at most 4 M, 3 I, 3 N or D and 2 S, ten decimal digits each)
    char cigar[160], num[64];
    uint32_t nm = 0;
    if (shk_alignment_cigar(&a, (uint32_t)L, min_intron, cigar, sizeof(cigar), &nm) != SHK_OK) return false;
    unsigned flag = secondary ? 0x100u : 0u;
    if (a.strand) flag |= 0x10u;
    const bool mate_has = paired && other.n_blocks != 0;
    if (paired) {
      flag |= 0x1u | (t == 0 ? 0x40u : 0x80u);
      if (!mate_has) flag |= 0x8u;
      else if (other.strand) flag |= 0x20u;
    }
    unsigned mapq = 255;
    long long tlen = 0;
    if (pair) {
      if (pair->proper) flag |= 0x2u;
      mapq = pair->mapq;
      if (pair->cls >= 3 && pair->cls <= 5) tlen = pair->left == t ? (long long)pair->tend - pair->tstart : (long long)pair->tstart - pair->tend;
    }
    f.append(id, id_len);
    int w = snprintf(num, sizeof(num), "\t%u\t", flag);
    f.append(num, (size_t)w);
    f.append(gene);
    w = snprintf(num, sizeof(num), "\t%u\t%u\t", a.block[0].x + 1, mapq);
    f.append(num, (size_t)w);
    f.append(cigar);
    if (mate_has) w = snprintf(num, sizeof(num), "\t=\t%u\t%lld\t", other.block[0].x + 1, tlen);
    else w = snprintf(num, sizeof(num), "\t*\t0\t0\t");
    f.append(num, (size_t)w);
    if (!a.strand) {
      f.append(seq, L);
    } else {
      // reversed; A<->T and C<->G with the case kept, every other byte N
      for (size_t p = L; p-- > 0;) {
        char c;
        switch (seq[p]) {
          case 'A': c = 'T'; break;
          case 'C': c = 'G'; break;
          case 'G': c = 'C'; break;
          case 'T': c = 'A'; break;
          case 'a': c = 't'; break;
          case 'c': c = 'g'; break;
          case 'g': c = 'c'; break;
          case 't': c = 'a'; break;
          default: c = 'N';
        }
        f.push_back(c);
      }
    }
    f.push_back('\t');
    if (!qual) f.push_back('*');
    else if (!a.strand) f.append(qual, L);
    else
      for (size_t p = L; p-- > 0;) f.push_back(qual[p]);
    if (rescued) w = snprintf(num, sizeof(num), "\tNM:i:%u\tYR:i:%u\n", nm, rescued->cost);
    else w = snprintf(num, sizeof(num), "\tNM:i:%u\n", nm);
    f.append(num, (size_t)w);
    return true;
  }
  static void record_view(std::string &f, const shk::RecordFetcher::View &v)
  {
    f.push_back('@');
    f.append(v.id, v.id_len);
    f.push_back('\n');
    f.append(v.seq, v.seq_len);
    f.append("\n+\n");
    f.append(v.qual, v.seq_len);
    f.push_back('\n');
  }
  static void record(std::string &f, const Strings &id, const DevStrings &seq, const DevStrings &qual, const std::map<size_t, std::string> &qual_as_read, size_t i)
  {
    f.push_back('@');
    if (i < id.size()) f.append(id.at(i), id.len(i));
    f.push_back('\n');
    if (i < seq.size()) f.append(seq.at(i), seq.len(i));
    f.append("\n+\n");
    const auto odd = qual_as_read.empty() ? qual_as_read.end() : qual_as_read.find(i);
    if (odd != qual_as_read.end()) f.append(odd->second);
    else if (i < qual.size()) f.append(qual.at(i), qual.len(i));
    f.push_back('\n');
  }
  OffsetWriter *out1_, *out2_;
  const std::vector<std::string> &legend_;
  FILE *evidence_;          // (--evidence) written by emit(), in input order
  FILE *candidates_;        // (--candidates) likewise
  FILE *placements_;        // (--placements) likewise, one line per association
  bool paired_;             // (--placements) the sample has two files: mate 2's fields are printed
  bool every_read_;         // one of the two: every read is named, not only the associated ones
  FILE *segments_;          // (--segments) likewise, one line per association
  bool junctions_;          // (--junctions) the mates' junctions are collected; write_junctions prints the table
  uint32_t k_, s_min_;      // (--junctions) the k-mer length and the support either side needs
  FILE *sam_;               // (--sam) likewise, one line per association and mate with a block
  uint32_t sam_min_intron_; // (--sam) the gap from which shk_alignment_cigar writes N
  bool sam_pairs_;          // (--sam-pairs) the lines carry the pair records' MAPQ, 0x2 and TLEN
  bool sam_rescue_;         // (--sam-rescue) a rescued mate's line carries YR:i:
  std::map<std::tuple<uint32_t, int64_t, int64_t>, std::pair<int64_t, uint64_t>> junction_table_;   // (gene, donor, acceptor) -> intron, mates
  bool failed_write_ = false, failed_write_cand_ = false, failed_write_plc_ = false, failed_write_sgm_ = false, failed_write_sam_ = false;
  mutable std::atomic<bool> failed_{false};   // a record could not be read back from its file (I/O error)
  std::string carry_;   // previd at the end of the previous batch (only used when a batch starts mid-chunk)
};

// CPUs this process can actually run threads on: the machine's count, cut down to its affinity mask and to its cgroup's CPU quota
// (cgroup v2 cpu.max, v1 cpu.cfs_quota_us / cpu.cfs_period_us)
unsigned usable_cpus()
{
  unsigned n = std::max(1u, std::thread::hardware_concurrency());
  cpu_set_t set;
  CPU_ZERO(&set);
  if (sched_getaffinity(0, sizeof(set), &set) == 0) {
    const int c = CPU_COUNT(&set);
    if (c > 0) n = std::min(n, (unsigned)c);
  }
  long quota = -1, period = -1;
  if (FILE *f = fopen("/sys/fs/cgroup/cpu.max", "r")) {
    char q[64];
    if (fscanf(f, "%63s %ld", q, &period) == 2 && strcmp(q, "max") != 0) quota = atol(q);
    fclose(f);
  } else {
    if (FILE *fq = fopen("/sys/fs/cgroup/cpu/cpu.cfs_quota_us", "r")) { if (fscanf(fq, "%ld", &quota) != 1) quota = -1; fclose(fq); }
    if (FILE *fp = fopen("/sys/fs/cgroup/cpu/cpu.cfs_period_us", "r")) { if (fscanf(fp, "%ld", &period) != 1) period = -1; fclose(fp); }
  }
  if (quota > 0 && period > 0) n = std::min(n, (unsigned)std::max(1L, (quota + period - 1) / period));
  return std::max(1u, n);
}

// ---- the stages of main(), in the order it runs them ---------------------------------------------------------------------------
// the reference opens its inputs unchecked (main.cpp:88-106) and then reads nothing from a file that is not there; here a
// sample that cannot be opened is reported before any work is done
bool samples_can_be_opened(const Options &opt, bool report = true)
{
  for (const std::string *path : {&opt.sample1_path, &opt.sample2_path}) {
    if (path->empty()) continue;
    // (a pipe is not opened for the check: it can be opened once.  access() says whether it may be read.)
    struct stat st;
    const bool pipe = stat(path->c_str(), &st) == 0 && !S_ISREG(st.st_mode) && !S_ISDIR(st.st_mode);
    FILE *f = pipe ? nullptr : fopen(path->c_str(), "rb");
    if (f) fclose(f);
    if (pipe ? access(path->c_str(), R_OK) != 0 : !f) {
      if (report) std::cerr << "shark: cannot open the sample " << *path << std::endl;
      return false;
    }
  }
  return true;
}

// set once by one thread, waited for by others
class Flag {
 public:
  void set() { std::lock_guard<std::mutex> l(m_); on_ = true; cv_.notify_all(); }
  void wait() { std::unique_lock<std::mutex> l(m_); cv_.wait(l, [&] { return on_; }); }
 private:
  std::mutex m_;
  std::condition_variable cv_;
  bool on_ = false;
};

struct RingPlan { size_t limit = 0, bytes = 0, reads = 0; bool paired = false, with_qual = false; };   // what the ring of batches has to hold; known once the sample is partitioned

// ---- contexts: one per GPU, index replicated by deterministic rebuild.  Creating the first context initialises the HIP runtime
// (a few hundred milliseconds); that happens on a thread of its own while the main thread reads the reference and the readers
// (which need no GPU) already parse the sample.  Every return of main() waits for that thread (the destructor). -------
class GpuStart {
 public:
  std::vector<shk_ctx *> ctxs;
  int rc = SHK_OK, bad = -1;     // (valid once `created` is set) the first worker whose context could not be created
  Flag created;                  // every shk_create has returned
  Flag ring_ready;               // the ring of batches exists: the readers may acquire batches
  GpuStart(const Options &opt, BatchPool &pool) : ctxs((size_t)opt.gpus, nullptr), opt_(opt), pool_(pool), th_([this] { run(); }) {}
  ~GpuStart() { join(); }
  void join() { if (th_.joinable()) th_.join(); }
  // The ring lives in ordinary memory by default: its buffers are handed round, so the runtime's registration of them is paid once
  // per buffer (measured: the same rate as page-locked buffers at what the readers deliver), it exists before the HIP runtime does --
  // the readers fill it while the runtime initialises -- and it costs nothing to set up: the caller's thread builds it.
  // SHARK_PINNED=1: page-locked memory, which only exists once the HIP runtime is up: the context thread builds it.
  void make_ring(const RingPlan &plan) { plan_ = plan; if (pin_ring_) ring_planned_.set(); else build_ring(); }
 private:
  void run()
  {
    // N workers start like N workers (main.cpp:219-223 starts the reference's N threads at once): every context is created on a
    // thread of its own -- the runtime comes up once, whoever gets there first; streams, the filter's allocation and its clearing,
    // the slots' buffers then proceed side by side (serially, two contexts took 2.3 x one context's time, eight would have taken
    // longer than a 16 M-pair sample on one GPU)
    const int n_gpus = opt_.gpus;
    std::vector<int> rcs((size_t)n_gpus, SHK_OK);
    auto create = [&](const int g) {
      shk_params p{};
      p.k = opt_.k; p.c = opt_.c; p.bf_bits = opt_.bf_size; p.min_quality = opt_.min_quality; p.single = opt_.single;
      p.device = opt_.devices[(size_t)g];   // worker g's device (--devices)
      rcs[(size_t)g] = shk_create(&p, &ctxs[(size_t)g]);
    };
    {
      std::vector<std::thread> th;
      for (int g = 1; g < n_gpus; ++g) th.emplace_back(create, g);
      create(0);
      for (auto &t : th) t.join();
    }
    for (int g = n_gpus - 1; g >= 0; --g)
      if (rcs[(size_t)g] != SHK_OK) { rc = rcs[(size_t)g]; bad = g; }
    timeline("contexts created");
    created.set();
    if (!pin_ring_) return;
    ring_planned_.wait();
    if (rc == SHK_OK) g_pin_batches = true;
    build_ring();
  }
  void build_ring() { pool_.make_ring(plan_.limit, plan_.bytes, plan_.reads, plan_.paired, plan_.with_qual); timeline("batch ring ready"); ring_ready.set(); }
  const Options &opt_;
  BatchPool &pool_;
  const bool pin_ring_ = getenv("SHARK_PINNED") && getenv("SHARK_PINNED")[0] == '1';
  RingPlan plan_;
  Flag ring_planned_;            // (SHARK_PINNED=1) plan_ is set
  std::thread th_;               // (last: it starts in the constructor and uses the members above)
};

// ---- the feed in use (parallel_feed: plain files; gz_feed: gzip'd files; neither: the serial reader alone) and the partition of the sample ----
struct FeedPlan {
  unsigned io_threads, n_readers = 0, n_gz_parsers = 0;
  bool parallel_feed, gz_feed, fixed_width = false;
  shk::BatchTable tab1, tab2;
  uint64_t n_par_records = 0;       // records both mate files certainly have: the pair stream of the strict part
  uint64_t n_par_batches = 0;
  uint64_t window = 0;              // a reader runs at most that many batches ahead of the drain; also the ring's size
  RingPlan ring;
  std::unique_ptr<GzCutter> cut1, cut2;
  FeedPlan(const Options &opt, unsigned io_threads_, bool need_qual) : io_threads(io_threads_)
  {
    // (the parallel feeds look into the sample files, read them twice and seek in them: regular files only -- a pipe goes to the
    //  serial reader, which opens it once and keeps names and qualities in memory)
    const bool samples_are_files = shk::regular_file(opt.sample1_path) && (!opt.paired_flag || shk::regular_file(opt.sample2_path));
    parallel_feed = samples_are_files && !getenv("SHARK_SERIAL_READER") && !getenv("SHARK_SINGLE_SPLITTER");
    // compressed samples (gzip magic in both mate files); SHARK_GZ_SERIAL_PARSE=1: the serial kseq-rule reader behind the
    // inflaters instead (A/B timing; no test sets it)
    auto is_gzip = [](const std::string &path) {
      unsigned char h[2] = {0, 0};
      FILE *f = fopen(path.c_str(), "rb");
      const bool gz = f && fread(h, 1, 2, f) == 2 && h[0] == 0x1f && h[1] == 0x8b;
      if (f) fclose(f);
      return gz;
    };
    gz_feed = parallel_feed && !getenv("SHARK_GZ_SERIAL_PARSE") && is_gzip(opt.sample1_path) && (!opt.paired_flag || is_gzip(opt.sample2_path));
    if (gz_feed) {
      parallel_feed = false;
      const unsigned gz_inflaters = std::max(2u, io_threads / (opt.paired_flag ? 2u : 1u));
      n_gz_parsers = std::max(2u, io_threads / 3u);
      cut1.reset(new GzCutter(opt.sample1_path, gz_inflaters, opt.batch));
      if (opt.paired_flag) cut2.reset(new GzCutter(opt.sample2_path, gz_inflaters, opt.batch));
      cut1->start();
      if (cut2) cut2->start();
    }
    if (parallel_feed) partition(opt);
    timeline("sample partitioned");
    n_par_batches = (n_par_records + opt.batch - 1) / opt.batch;
    n_readers = parallel_feed ? (unsigned)std::max<uint64_t>(1, std::min<uint64_t>(io_threads, n_par_batches)) : 0;
    // the ring: a batch per reader, what the GPUs hold in flight, and a few being turned into text or waiting for their turn to be written
    // (never more batches than the sample has, plus what the serial reader and the GPU pipelines need: --batch may be large)
    const uint64_t in_flight = (uint64_t)opt.gpus * (SHK_PIPE_DEPTH + 2);
    window = gz_feed ? n_gz_parsers + in_flight + 6 : std::min<uint64_t>(n_readers + in_flight + 6, n_par_batches + in_flight + 2);
    uint64_t widest = 0;
    for (uint64_t i = 0; i < n_par_batches; ++i) {
      widest = std::max(widest, tab1.off[i + 1] - tab1.off[i]);
      if (opt.paired_flag) widest = std::max(widest, tab2.off[i + 1] - tab2.off[i]);
    }
    ring = RingPlan{(size_t)window, n_par_batches ? (size_t)(widest / 2 + 64) : (gz_feed ? (size_t)opt.batch * 160 : 0),
                    (n_par_batches || gz_feed) ? (size_t)opt.batch : 0, opt.paired_flag, need_qual};
  }
 private:
  // fixed-width records: batch offsets are arithmetic; otherwise a parallel newline count of both files
  void partition(const Options &opt)
  {
    uint64_t rl1 = 0, rl2 = 0;
    std::vector<uint64_t> cnt1, cnt2;
    fixed_width = shk::fixed_record_file(opt.sample1_path, tab1, rl1) && (!opt.paired_flag || shk::fixed_record_file(opt.sample2_path, tab2, rl2));
    if (!fixed_width) {
      if (tab1.fd >= 0) { ::close(tab1.fd); tab1.fd = -1; }
      if (tab2.fd >= 0) { ::close(tab2.fd); tab2.fd = -1; }
      shk::count_file(opt.sample1_path, io_threads, tab1, cnt1);
      if (tab1.ok && opt.paired_flag) shk::count_file(opt.sample2_path, io_threads, tab2, cnt2);
      parallel_feed = tab1.ok && (!opt.paired_flag || tab2.ok);
      if (!parallel_feed) return;
    }
    n_par_records = opt.paired_flag ? std::min(tab1.n_records, tab2.n_records) : tab1.n_records;
    if (fixed_width) {
      shk::fixed_record_batches(tab1, rl1, opt.batch, n_par_records);
      if (opt.paired_flag) shk::fixed_record_batches(tab2, rl2, opt.batch, n_par_records);
      return;
    }
    shk::locate_batches(tab1, cnt1, opt.batch, n_par_records, io_threads);
    if (opt.paired_flag) shk::locate_batches(tab2, cnt2, opt.batch, n_par_records, io_threads);
    parallel_feed = tab1.ok && (!opt.paired_flag || tab2.ok);
    if (!parallel_feed) n_par_records = 0;
  }
};

// ---- the order of the batches ---------------------------------------------------------------------------------------------------
// Batches leave the readers, go round the workers (batch i to worker i mod N) and the formatters in any order, and are written in
// input order.  Two rules hold them together:
//  * a reader must not run ahead of the drain without bound: at most `window` batches beyond the one being written;
//  * batch j may only leave a reader once every batch before it is KNOWN to be strict four-line FASTQ: an irregular batch
//    i < j that keeps the four-line alignment (an empty read, a sequence/quality length mismatch, a lone CR, a NUL) lets
//    batch j validate, yet everything from i on belongs to the serial reader -- which numbers its batches from i again
//    and may cut the records differently.
class BatchOrder {
 public:
  using Queue = BoundedQueue<std::unique_ptr<ReadBatch>>;
  // (the inputs' capacity is never reached: the readers' window bounds what is in flight)
  BatchOrder(int n_workers, uint64_t window) : window_(window) { for (int g = 0; g < n_workers; ++g) todo_.emplace_back(new Queue(1u << 20)); }
  // -- the parallel readers, for the batch i each of them holds --
  // waits until batch i is inside the window; false: it belongs to the serial reader
  bool admit(uint64_t i)
  {
    if (i >= irregular_at_.load()) return false;
    std::unique_lock<std::mutex> l(m_);
    cv_.wait(l, [&] { return i < drained_ + window_ || i >= irregular_at_.load(); });
    return i < irregular_at_.load();
  }
  // batch i is not strict four-line FASTQ: it and everything behind it belongs to the serial reader
  void mark_irregular(uint64_t i)
  {
    uint64_t cur = irregular_at_.load();
    while (i < cur && !irregular_at_.compare_exchange_weak(cur, i)) {}
    { std::lock_guard<std::mutex> l(m_); }   // (a waiter that has just found its predicate false is asleep before it is notified)
    cv_.notify_all();
  }
  // batch i is strict: waits until every batch before it is, too; false: one of them was not
  // (batch indices are handed out in increasing order, so the reader of the smallest outstanding one never waits here)
  bool commit(uint64_t i)
  {
    {
      std::unique_lock<std::mutex> l(m_);
      cv_.wait(l, [&] { return validated_ == i || i >= irregular_at_.load(); });
      if (i >= irregular_at_.load()) return false;
      validated_ = i + 1;
    }
    cv_.notify_all();
    return true;
  }
  uint64_t first_irregular() const { return irregular_at_.load(); }
  // -- any reader: a batch on its way to its worker --
  void dispatch(std::unique_ptr<ReadBatch> b)
  {
    { std::lock_guard<std::mutex> l(m_); n_batches_ = std::max(n_batches_, b->index + 1); }
    todo_[(size_t)(b->index % todo_.size())]->push(std::move(b));
  }
  Queue &input(int worker) { return *todo_[(size_t)worker]; }
  void close_inputs() { for (auto &q : todo_) q->close(); }
  // no batch will be dispatched any more
  void feed_closed() { std::lock_guard<std::mutex> l(m_); split_finished_ = true; cv_.notify_all(); }
  // -- the formatters: a batch that is ready to be written --
  void finished(std::unique_ptr<ReadBatch> b) { std::lock_guard<std::mutex> l(m_); done_[b->index] = std::move(b); cv_.notify_all(); }
  // -- the drain: the next batch in input order (nullptr behind the last one), and the step behind it --
  std::unique_ptr<ReadBatch> next_in_order()
  {
    std::unique_lock<std::mutex> l(m_);
    cv_.wait(l, [&] { return done_.count(drained_) || (split_finished_ && drained_ >= n_batches_); });
    auto it = done_.find(drained_);
    if (it == done_.end()) return nullptr;
    std::unique_ptr<ReadBatch> b = std::move(it->second);
    done_.erase(it);
    return b;
  }
  void advance() { { std::lock_guard<std::mutex> l(m_); ++drained_; } cv_.notify_all(); }
 private:
  std::vector<std::unique_ptr<Queue>> todo_;            // per-worker input queues
  const uint64_t window_;
  std::atomic<uint64_t> irregular_at_{UINT64_MAX};      // first batch a reader found not to be strict four-line FASTQ
  std::mutex m_;                                        // guards everything below
  std::condition_variable cv_;
  std::map<uint64_t, std::unique_ptr<ReadBatch>> done_;
  uint64_t n_batches_ = 0;                              // batches handed to the workers so far
  uint64_t validated_ = 0;                              // number of leading batches known to be strict
  uint64_t drained_ = 0;                                // the drain's position: batches written
  bool split_finished_ = false;
};

// ---- the parallel feed: readers of plain files; or, compressed samples, a joiner of the two cutters' pieces and parsers ---------
class ParallelFeed {
 public:
  ParallelFeed(const Options &opt, FeedPlan &plan, BatchOrder &order, BatchPool &pool, Flag &ring_ready, bool need_qual)
      : t_reader(plan.n_readers, 0.0), opt_(opt), plan_(plan), order_(order), pool_(pool), ring_ready_(ring_ready), need_qual_(need_qual)
  {
    if (plan.parallel_feed) {
      std::vector<char> head(1u << 16);
      for (int m = 0; m < (opt.paired_flag ? 2 : 1); ++m) {
        shk::BatchTable &t = m ? plan.tab2 : plan.tab1;
        const size_t got = (size_t)std::min<uint64_t>(head.size(), t.file_size);
        if (got && shk::pread_all(t.fd, head.data(), 0, got)) shk::layout_of(head.data(), got, m ? lay2_ : lay1_);
      }
    }
    for (unsigned r = 0; r < plan.n_readers; ++r) threads_.emplace_back([this, r] { plain_reader(r); });
    if (plan.gz_feed) {
      gz_joiner_ = std::thread([this] { join_pieces(); });
      for (unsigned r = 0; r < plan.n_gz_parsers; ++r) threads_.emplace_back([this] { gz_parser(); });
    }
  }
  // every batch the feed can deliver is dispatched
  void join() { if (gz_joiner_.joinable()) gz_joiner_.join(); for (auto &t : threads_) t.join(); threads_.clear(); }
  // a failure before the workers take batches: end the readers (they stop at an irregular batch 0) and take their batches back
  void stop()
  {
    order_.mark_irregular(0);
    order_.close_inputs();
    pool_.shutdown();
    // (the parsers drop every job once batch 0 counts as irregular; the joiner notices the same and stops the cutters)
    std::thread drop_jobs([&] { std::unique_ptr<GzJob> j; while (plan_.gz_feed && gz_jobs_.pop(j)) {} });
    join();
    drop_jobs.join();
    std::unique_ptr<ReadBatch> b;   // (the inputs never fill up: nobody waited for this)
    for (int g = 0; g < opt_.gpus; ++g) while (order_.input(g).pop(b)) {}
  }
  uint64_t gz_batches() const { return gz_batches_.load(); }
  std::vector<double> t_reader;   // seconds each plain reader spent parsing (verbose report)
 private:
  struct GzJob { uint64_t index; std::unique_ptr<GzPiece> p1, p2; size_t want; };
  enum class Delivery { done, serial, stopped };   // dispatched; the batch belongs to the serial reader; the pool is shut down
  // The one hand-over of a strict batch i: `parse` fills the batch and says whether all its records are strict.
  template <typename Parse>
  Delivery deliver(uint64_t i, Parse &&parse)
  {
    if (!order_.admit(i)) return Delivery::serial;
    std::unique_ptr<ReadBatch> b = pool_.acquire();
    if (!b) return Delivery::stopped;
    b->index = i; b->first_read = i * opt_.batch; b->lean = true;
    if (!parse(*b)) { pool_.release(std::move(b)); order_.mark_irregular(i); return Delivery::serial; }
    if (!order_.commit(i)) { pool_.release(std::move(b)); return Delivery::serial; }
    order_.dispatch(std::move(b));
    return Delivery::done;
  }
  void plain_reader(unsigned r)
  {
    shk::LeanScratch sc;
    ring_ready_.wait();   // the ring of batches exists (at once; page-locked: once the HIP runtime is up)
    const shk::BatchTable &tab1 = plan_.tab1, &tab2 = plan_.tab2;
    for (;;) {
      const uint64_t i = next_batch_.fetch_add(1);
      if (i >= plan_.n_par_batches) break;
      const size_t want = (size_t)std::min<uint64_t>(opt_.batch, plan_.n_par_records - i * opt_.batch);
      const Delivery d = deliver(i, [&](ReadBatch &b) {
        const auto t0 = std::chrono::steady_clock::now();
        size_t ok1 = shk::lean_parse_range(tab1.fd, tab1.off[i], tab1.off[i + 1], want, lay1_, need_qual_, sc, b.seq1.bytes, b.seq1.off, b.qual1.bytes, b.part1);
        size_t ok2 = want;
        if (opt_.paired_flag && ok1 == want)
          ok2 = shk::lean_parse_range(tab2.fd, tab2.off[i], tab2.off[i + 1], want, lay2_, need_qual_, sc, b.seq2.bytes, b.seq2.off, b.qual2.bytes, b.part2);
        if (ok1 < want || ok2 < want) return false;
        t_reader[r] += std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
        return true;
      });
      // a plain reader ENDS at the first batch that is not its to deliver: every index it could claim next lies behind it
      if (d != Delivery::done) break;
    }
  }
  // compressed samples: the pieces of the two mates, joined by index
  void join_pieces()
  {
    GzCutter *cut1 = plan_.cut1.get(), *cut2 = plan_.cut2.get();
    for (uint64_t i = 0;; ++i) {
      std::unique_ptr<GzPiece> a = cut1->next(), b2;
      if (cut2) b2 = cut2->next();
      if (!a || (cut2 && !b2)) break;
      // the pair stream ends with the shorter mate file (FastqSplitter.hpp:60)
      const size_t want = cut2 ? std::min(a->records, b2->records) : a->records;
      const bool ends = a->last || (b2 && b2->last) || want < opt_.batch;
      if (want) {
        std::unique_ptr<GzJob> j(new GzJob{i, std::move(a), std::move(b2), want});
        gz_batches_ = i + 1;
        gz_jobs_.push(std::move(j));
      }
      if (ends || i >= order_.first_irregular()) break;
    }
    gz_jobs_.close();
    // (whatever the cutters still hold is not part of the pair stream -- or belongs to the serial reader)
    cut1->stop();
    if (cut2) cut2->stop();
  }
  void gz_parser()
  {
    ring_ready_.wait();
    shk::RecordLayout gl1, gl2;
    std::unique_ptr<GzJob> j;
    while (gz_jobs_.pop(j)) {
      const Delivery d = deliver(j->index, [&](ReadBatch &b) {
        // the text moves into the batch (its old buffer goes back to the cutter); a piece with more records than the pair
        // stream takes is cut behind the want-th record
        auto take = [&](GzPiece &p, std::vector<char, default_init_allocator<char>> &text, shk::RecordLayout &lay) -> size_t {
          text.swap(p.text);
          size_t len = text.size();
          if (p.records > j->want) {
            uint64_t found = 0;
            len = newlines_until(text.data(), text.size(), 4 * (uint64_t)j->want, found);
          }
          if (!lay.usable()) shk::layout_of(text.data(), len, lay);
          return len;
        };
        const size_t len1 = take(*j->p1, b.text1, gl1);
        size_t ok1 = shk::lean_parse_mem(b.text1.data(), len1, j->want, gl1, need_qual_, b.seq1.bytes, b.seq1.off, b.qual1.bytes, b.part1);
        size_t ok2 = j->want;
        if (j->p2 && ok1 == j->want) {
          const size_t len2 = take(*j->p2, b.text2, gl2);
          ok2 = shk::lean_parse_mem(b.text2.data(), len2, j->want, gl2, need_qual_, b.seq2.bytes, b.seq2.off, b.qual2.bytes, b.part2);
        }
        plan_.cut1->recycle(std::move(j->p1));
        if (j->p2) plan_.cut2->recycle(std::move(j->p2));
        return ok1 == j->want && ok2 == j->want;
      });
      // Unlike a plain reader, a parser GOES ON behind a batch that is not its to deliver, dropping the jobs: the joiner pushes
      // into a queue of two and must never be left blocked there -- the serial feed and stop() join it before the parsers.  Only a
      // pool that is shut down (stop(), which empties the queue itself) ends a parser early.
      if (d == Delivery::stopped) break;
    }
  }
  const Options &opt_;
  FeedPlan &plan_;
  BatchOrder &order_;
  BatchPool &pool_;
  Flag &ring_ready_;
  const bool need_qual_;            // the device reads qualities only with -q
  shk::RecordLayout lay1_, lay2_;   // the layout of each plain file's first record: the readers' fast check
  std::atomic<uint64_t> next_batch_{0};
  BoundedQueue<std::unique_ptr<GzJob>> gz_jobs_{2};
  std::atomic<uint64_t> gz_batches_{0};   // batches the joiner handed out
  std::vector<std::thread> threads_;      // plain readers or gzip parsers
  std::thread gz_joiner_;
};

// ---- --splice-junctions: the file's lines as the sorted, merged site list of shk_splice_sites_set.  A line `<gene> <donor> <acceptor> <intron>
// [<mates>]` becomes (gene, donor, donor + intron): the intron interval of the alignment blocks (the left block keeps the microhomology), not
// the file's acceptor column, which is the right span's lo and includes the overlap.  Returns the message of the line that is malformed, names
// an unknown gene or lies outside its record (empty: none). ----
std::string read_splice_sites(const Options &opt, const std::vector<std::string> &legend_ID, const std::vector<uint64_t> &gene_start,
                              std::vector<shk_splice_site> &sites)
{
  std::ifstream in(opt.splice_path);
  if (!in) return "shark: cannot open the --splice-junctions file " + opt.splice_path;
  std::unordered_map<std::string, uint32_t> index;
  for (size_t g = legend_ID.size(); g-- > 0;) index[legend_ID[g]] = (uint32_t)g;   // (a name given twice: the first record, as --depth's readers take it)
  std::string line;
  for (uint64_t n = 1; std::getline(in, line); ++n) {
    const std::string where = "shark: --splice-junctions " + opt.splice_path + " line " + std::to_string(n) + ": ";
    std::istringstream fields(line);
    std::vector<std::string> f;
    for (std::string w; fields >> w;) f.push_back(w);
    if (f.empty()) continue;
    uint64_t v[4] = {0, 0, 0, 1};
    bool ok = f.size() == 4 || f.size() == 5;
    for (size_t i = 1; ok && i < f.size(); ++i) {
      ok = !f[i].empty() && f[i].size() <= 10 && f[i].find_first_not_of("0123456789") == std::string::npos;
      if (ok) v[i - 1] = std::stoull(f[i]);
    }
    if (!ok) return where + "malformed (<gene> <donor> <acceptor> <intron> [<mates>])";
    const auto it = index.find(f[0]);
    if (it == index.end()) return where + "unknown gene " + f[0];
    const uint32_t g = it->second;
    const uint64_t len_g = (size_t)g + 1 < gene_start.size() ? gene_start[g + 1] - gene_start[g] : 0;
    if (!(v[0] >= 1 && v[2] >= 1 && v[0] + v[2] + 1 <= len_g)) return where + "the site lies outside its record";
    if (v[3] >= opt.splice_min_mates) sites.push_back({g, (uint32_t)v[0], (uint32_t)(v[0] + v[2])});
  }
  const auto key = [](const shk_splice_site &t) { return std::make_tuple(t.gene, t.donor, t.acceptor); };
  std::sort(sites.begin(), sites.end(), [&](const shk_splice_site &a, const shk_splice_site &b) { return key(a) < key(b); });
  sites.erase(std::unique(sites.begin(), sites.end(), [&](const shk_splice_site &a, const shk_splice_site &b) { return key(a) == key(b); }), sites.end());
  return std::string();
}

// ---- 1+2. reference: legend in file order (FastaSplitter.hpp:48) + index -- while the readers already parse the sample.
// Returns the message of the failure that ended it (empty: none). ----
std::string build_index(const Options &opt, GpuStart &gpu, std::vector<std::string> &legend_ID)
{
  {
    shk::FastxReader fa(opt.fasta_path);
    if (!fa.ok()) return "shark: cannot open " + opt.fasta_path;
    gpu.created.wait();
    if (gpu.rc != SHK_OK)
      return "shark: cannot create a context on GPU " + std::to_string(opt.devices[(size_t)gpu.bad]) + ": " + shk_strerror(gpu.rc);
    shk::FastxRecord rec;
    std::string sam_header = "@HD\tVN:1.6\tSO:unsorted\n";       // (--sam) one @SQ per gene in id order, under --depth's names
    while (fa.read(rec) >= 0) {
      legend_ID.push_back(rec.name.c_str());
      if (opt.placements_file && legend_ID.size() > 65536) return "shark: --placements is not available for a reference of more than 65536 records (gene ids wrap there).";
      if (opt.depth_file && legend_ID.size() > 65536) return "shark: --depth is not available for a reference of more than 65536 records (gene ids wrap there).";
      if (opt.segments_file && legend_ID.size() > 65536) return "shark: --segments is not available for a reference of more than 65536 records (gene ids wrap there).";
      if (opt.junctions_file && legend_ID.size() > 65536) return "shark: --junctions is not available for a reference of more than 65536 records (gene ids wrap there).";
      if (opt.pileup_file && legend_ID.size() > 65536) return "shark: --pileup is not available for a reference of more than 65536 records (gene ids wrap there).";
      if (opt.variants_file && legend_ID.size() > 65536) return "shark: --variants is not available for a reference of more than 65536 records (gene ids wrap there).";
      if (opt.sam_file && legend_ID.size() > 65536) return "shark: --sam is not available for a reference of more than 65536 records (gene ids wrap there).";
      if (opt.indels_file && legend_ID.size() > 65536) return "shark: --indels is not available for a reference of more than 65536 records (gene ids wrap there).";
      if (opt.fragments_file && legend_ID.size() > 65536) return "shark: --fragments is not available for a reference of more than 65536 records (gene ids wrap there).";
      const size_t len = strnlen(rec.seq.data(), rec.seq.size());  // C-string semantics (main.cpp:164)
      if (opt.sam_file) sam_header += "@SQ\tSN:" + legend_ID.back() + "\tLN:" + std::to_string(len) + "\n";
      for (auto *ctx : gpu.ctxs) {
        const int rc = shk_ref_add(ctx, rec.seq.data(), len);
        if (rc != SHK_OK) return std::string("shark: ") + shk_strerror(rc);
      }
    }
    if (opt.sam_file && fwrite(sam_header.data(), 1, sam_header.size(), opt.sam_file) != sam_header.size()) return "shark: cannot write the SAM file " + opt.sam_path;
  }
  pelapsed("Transcript file processed");
  timeline("reference read");
  if (opt.placements_file || opt.depth_file || opt.segments_file || opt.junctions_file || opt.pileup_file || opt.variants_file || opt.sam_file ||
      opt.fragments_file || opt.indels_file)
    for (auto *ctx : gpu.ctxs)
      if (const int rc = shk_ref_keep_positions(ctx)) return std::string("shark: ") + shk_strerror(rc);
  // (the k-mer keyed table repays its enumeration behind several hundred million pairs classified at the GPU's speed: not in a run of this command)
  for (auto *ctx : gpu.ctxs)
    if (const int rc = shk_ref_kmer_table(ctx, opt.kmer_table ? 1 : 0)) return std::string("shark: ") + shk_strerror(rc);
  // (--variants: the records' bases stay on the device; only worker 0 is asked for the sites, but every replica is built alike)
  // (--sam: every worker's alignments kernel reads them)
  // (--pileup-aligned: the accumulating alignments kernel reads them as well)
  // (--fragments: alignments mode runs for it as it does for --sam)
  // (--indels: the alignments kernel runs for it, and its own kernel reads them when it moves an event)
  if (opt.variants_file || opt.sam_file || opt.pileup_aligned || opt.fragments_file || opt.indels_file)
    for (auto *ctx : gpu.ctxs)
      if (const int rc = shk_ref_keep_bases(ctx)) return std::string("shark: ") + shk_strerror(rc);
  {
    const size_t n = gpu.ctxs.size();
    std::vector<std::thread> th;
    std::vector<int> rcs(n, 0);
    for (size_t g = 0; g < n; ++g) th.emplace_back([&, g] { rcs[g] = shk_ref_finalize(gpu.ctxs[g]); });
    for (auto &t : th) t.join();
    for (size_t g = 0; g < n; ++g)
      if (rcs[g] != SHK_OK)
        return "shark: index build failed on GPU " + std::to_string(g) + ": " + shk_strerror(rcs[g]) + " " + shk_last_error(gpu.ctxs[g]);
  }
  timeline("index built");
  pelapsed("First switch performed");
  shk_index_info info{};
  shk_index_info_get(gpu.ctxs[0], &info);
  pelapsed("BF created from transcripts (" + std::to_string(info.nidx) + " genes)");
  pelapsed("Second switch performed");
  return "";
}

// ---- the serial feed: everything the parallel feed did not (or could not) deliver, through the kseq-rule reader `fs` (created
// only when there is something left; failed: it could not open the sample) ----
void serial_feed(const Options &opt, const FeedPlan &plan, ParallelFeed &feed, BatchOrder &order, BatchPool &pool, std::unique_ptr<BatchSplitter> &fs, bool &failed)
{
  feed.join();
  timeline("parallel readers done");
  const shk::BatchTable &tab1 = plan.tab1, &tab2 = plan.tab2;
  // the parallel feed delivered batches [0, stop); an irregular record sends the rest through the serial reader
  const uint64_t irregular = order.first_irregular();
  const uint64_t stop = std::min<uint64_t>(irregular, plan.gz_feed ? feed.gz_batches() : plan.n_par_batches);
  // plain files: nothing is left when the readers delivered every batch and a mate file ends exactly there (the pair stream ends
  // with the shorter file, FastqSplitter.hpp:60); compressed samples: the joiner saw the end of the pair stream
  const bool needed = plan.gz_feed ? irregular != UINT64_MAX
                                   : !plan.parallel_feed || stop < plan.n_par_batches ||
                                         !(tab1.off[stop] >= tab1.file_size || (opt.paired_flag && tab2.off[stop] >= tab2.file_size));
  if (needed) fs.reset(new BatchSplitter(opt, plan.io_threads, pool));
  failed = needed && !fs->ok();
  if (needed && !failed) {
    // behind what was delivered: compressed samples are read over (the delivered records are strict: the kseq reader's records are
    // the same), plain files are entered at the batch's offset, a purely serial run starts at the start
    if (plan.gz_feed) fs->skip_records(stop * opt.batch, stop);
    else if (plan.parallel_feed) fs->resume_serial(tab1.off[stop], opt.paired_flag ? tab2.off[stop] : 0, stop, std::min<uint64_t>(stop * opt.batch, plan.n_par_records));
    while (std::unique_ptr<ReadBatch> b = (*fs)()) order.dispatch(std::move(b));
  }
  order.close_inputs();
  timeline("serial reader done");
  order.feed_closed();
}

// analyzers: one thread per worker, SHK_PIPE_DEPTH batches in flight each; t_gpu[g]: seconds inside shk_classify_submit / _wait
std::vector<std::thread> start_analyzers(const std::vector<shk_ctx *> &ctxs, bool need_qual, bool evidence, bool candidates, bool placements, bool segments, bool alignments, bool pairs, bool rescue, BatchOrder &order, BatchOrder::Queue &to_format, std::vector<double> &t_gpu)
{
  std::vector<std::thread> analyzers;
  for (int g = 0; g < (int)ctxs.size(); ++g) {
    analyzers.emplace_back([&, g, need_qual, evidence, candidates, placements, segments, alignments, pairs, rescue] {
      ReadAnalyzer ra(ctxs[(size_t)g], need_qual, evidence, candidates, placements, segments, alignments, pairs, rescue);
      BatchOrder::Queue &todo = order.input(g);
      bool open = true;
      while (open || ra.in_flight()) {
        // keep the pipeline full; block for input only when nothing is in flight
        while (open && ra.in_flight() < SHK_PIPE_DEPTH) {
          std::unique_ptr<ReadBatch> b;
          int got;
          if (ra.in_flight() == 0) got = todo.pop(b) ? 1 : -1;
          else got = todo.try_pop(b);
          if (got < 0) { open = false; break; }
          if (got == 0) break;
          auto t0 = std::chrono::steady_clock::now();
          if (!ra.submit(std::move(b))) to_format.push(ra.take_failed());
          t_gpu[(size_t)g] += std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
        }
        if (ra.in_flight()) {
          auto t0 = std::chrono::steady_clock::now();
          std::unique_ptr<ReadBatch> b = ra.wait();
          t_gpu[(size_t)g] += std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
          to_format.push(std::move(b));
        }
      }
    });
  }
  return analyzers;
}

// ---- 3. sample ---------------------------------------------------------------
// Three roles, as in main.cpp:66-77 (split / analyze / output), decoupled by queues; the host does NOT join or mask the reads: the device does.
//   readers    the parallel feed (plain four-line FASTQ: whole batches parsed independently into structure-of-arrays batches --
//              the feed scales with host cores instead of one splitter mutex, FastqSplitter.hpp:48; gzip: cut and parsed from
//              memory) and, from the first batch that is not strict on or for anything else, the serial kseq-rule reader
//   analyzers  one thread per GPU, batch i -> GPU i mod N, SHK_PIPE_DEPTH batches in flight per GPU (ReadAnalyzer role)
//   formatters classified batches -> text, in any order
//   output     this thread, batches in input order (ReadOutput.hpp:37-50)
// The reference is read and the index built in between, while the readers already parse.  Returns main()'s exit code.
int run_sample(const Options &opt, GpuStart &gpu, BatchPool &pool, std::vector<std::string> &legend_ID)
{
  // readers / parsers / formatters: sixteen per worker (what one GPU's feed was measured to use), as far as this process has cores
  // to run them on -- its affinity mask and its cgroup's CPU quota count, not the machine's (a one-GPU share of a host is 16 cores
  // whatever hardware_concurrency() says: more threads than that only take turns)
  const unsigned io_threads = opt.nThreads > 1 ? (unsigned)opt.nThreads : std::max(1u, std::min(16u * (unsigned)opt.gpus, usable_cpus()));
  const bool need_qual = static_cast<char>(opt.min_quality) != 0;   // the device reads qualities only with -q (the reference's char, argument_parser.hpp:144)
  // (the reference opens its outputs unchecked and writes nothing to a file it could not open, main.cpp:99-106: same here)
  TextPool text_pool;               // (in front of the writers: they hand the last texts back while they close)
  OffsetWriter w1, w2;
  // one writer thread per output file: tmpfs takes 8.7 GB/s from ONE thread writing a file and 3.6-4.6 GB/s from 2-12 threads
  // writing disjoint parts of it (tools/tmpfs_write_bench.cpp); the command with half the sample written out again, 32 M pairs,
  // the same files: 2.74 / 2.80 s with one helper per file, 2.93-3.38 s with three, 3.65 s with two
  unsigned write_helpers = 1;
  if (const char *e = getenv("SHARK_WRITE_HELPERS")) write_helpers = (unsigned)std::max(1, atoi(e));
  w1.open(opt.out1_path, write_helpers);
  if (opt.paired_flag && opt.out2_path != "") w2.open(opt.out2_path, write_helpers);
  OffsetWriter *out1 = w1.is_open() ? &w1 : nullptr, *out2 = w2.is_open() ? &w2 : nullptr;
  ReadOutput ro(out1, out2, legend_ID, opt.evidence_file, opt.candidates_file, opt.placements_file, opt.paired_flag, opt.segments_file,
                opt.junctions_file != nullptr && !opt.junctions_device, opt.k, opt.junctions_min_support, opt.sam_file, opt.sam_min_intron,
                opt.sam_pairs, opt.sam_rescue);
  setvbuf(stdout, nullptr, _IOFBF, 1 << 22);

  FeedPlan plan(opt, io_threads, need_qual);
  BatchOrder order(opt.gpus, plan.window);
  gpu.make_ring(plan.ring);
  ParallelFeed feed(opt, plan, order, pool, gpu.ring_ready, need_qual);
  // (the one early exit while the feed runs: whatever fails in there, the feed is stopped first)
  const std::string index_error = build_index(opt, gpu, legend_ID);
  if (!index_error.empty()) {
    feed.stop();
    std::cerr << index_error << std::endl;
    return EXIT_FAILURE;
  }
  // (--evidence: every worker's batches carry their reads' evidence from the first one on; the contexts exist, nothing is in flight)
  if (opt.evidence_file)
    for (shk_ctx *ctx : gpu.ctxs)
      if (const int rc = shk_evidence_enable(ctx, 1)) {
        feed.stop();
        std::cerr << "shark: evidence mode could not be switched on: " << shk_strerror(rc) << std::endl;
        return EXIT_FAILURE;
      }
  if (opt.candidates_file)
    for (shk_ctx *ctx : gpu.ctxs)
      if (const int rc = shk_candidates_enable(ctx, opt.candidates_n)) {
        feed.stop();
        std::cerr << "shark: candidates mode could not be switched on: " << shk_strerror(rc) << std::endl;
        return EXIT_FAILURE;
      }
  if (opt.placements_file)
    for (shk_ctx *ctx : gpu.ctxs)
      if (const int rc = shk_placement_enable(ctx, 1)) {
        feed.stop();
        std::cerr << "shark: placement mode could not be switched on: " << shk_strerror(rc) << " " << shk_last_error(ctx) << std::endl;
        return EXIT_FAILURE;
      }
  // (--segments, --junctions: one mode of the library serves both; the junctions are computed from the segments on the host)
  const bool host_junctions = opt.junctions_file && !opt.junctions_device;
  if (opt.segments_file || host_junctions)
    for (shk_ctx *ctx : gpu.ctxs)
      if (const int rc = shk_segments_enable(ctx, opt.segments_max)) {
        feed.stop();
        std::cerr << "shark: segments mode could not be switched on: " << shk_strerror(rc) << " " << shk_last_error(ctx) << std::endl;
        return EXIT_FAILURE;
      }
  // (--depth: every worker adds its batches' placed mates to its own depth state; write_depth sums the workers' arrays at the end)
  if (opt.depth_file)
    for (shk_ctx *ctx : gpu.ctxs)
      if (const int rc = opt.depth_spliced ? shk_depth_enable_spliced(ctx, opt.depth_min_support) : shk_depth_enable(ctx, opt.depth_min_support)) {
        feed.stop();
        std::cerr << "shark: depth mode could not be switched on: " << shk_strerror(rc) << " " << shk_last_error(ctx) << std::endl;
        return EXIT_FAILURE;
      }
  // (--junctions-device: every worker adds its batches' junctions to its own table; write_junctions_device merges the tables at the end)
  if (opt.junctions_file && opt.junctions_device)
    for (shk_ctx *ctx : gpu.ctxs)
      if (const int rc = shk_junctions_enable(ctx, opt.junctions_min_support, opt.junctions_capacity)) {
        feed.stop();
        std::cerr << "shark: the junction table could not be switched on: " << shk_strerror(rc) << " " << shk_last_error(ctx) << std::endl;
        return EXIT_FAILURE;
      }
  // (--pileup: every worker adds its batches' bases to its own pileup state; write_pileup sums the workers' arrays at the end)
  // (--variants reads the same state, at the same floor: parse_arguments saw to that)
  if (opt.pileup_file || opt.variants_file)
    for (shk_ctx *ctx : gpu.ctxs)
      if (const int rc = (opt.pileup_aligned ? shk_pileup_enable_aligned : shk_pileup_enable)(ctx, opt.pileup_file ? opt.pileup_min_support : opt.variants_min_support)) {
        feed.stop();
        std::cerr << "shark: pileup mode could not be switched on: " << shk_strerror(rc) << " " << shk_last_error(ctx) << std::endl;
        return EXIT_FAILURE;
      }
  // (--extend-ends: every worker's alignments kernel extends the ends alike, for --sam and for --pileup-aligned)
  if (opt.extend_ends)
    for (shk_ctx *ctx : gpu.ctxs)
      if (const int rc = shk_alignments_extend(ctx, opt.extend_penalty, opt.extend_bonus)) {
        feed.stop();
        std::cerr << "shark: end extension could not be switched on: " << shk_strerror(rc) << " " << shk_last_error(ctx) << std::endl;
        return EXIT_FAILURE;
      }
  // (--splice-junctions: every worker gets the same list and the same parameters, for --sam and for --pileup-aligned; an empty list leaves the step off)
  if (!opt.splice_path.empty()) {
    std::vector<uint64_t> gene_start(legend_ID.size() + 1, 0);
    std::vector<shk_splice_site> sites;
    std::string error;
    if (const int rc = gpu.ctxs.empty() ? SHK_ERR_STATE : shk_depth_layout(gpu.ctxs[0], gene_start.data(), (uint32_t)legend_ID.size()))
      error = std::string("shark: --splice-junctions is not available for this reference: ") + shk_strerror(rc);
    else error = read_splice_sites(opt, legend_ID, gene_start, sites);
    if (!error.empty()) {
      feed.stop();
      std::cerr << error << std::endl;
      return EXIT_FAILURE;
    }
    if (!sites.empty())
      for (shk_ctx *ctx : gpu.ctxs) {
        int rc = shk_splice_sites_set(ctx, sites.data(), sites.size());
        if (!rc) rc = shk_alignments_splice(ctx, opt.splice_min_overhang, opt.splice_max_cost, opt.splice_min_gap);
        if (rc) {
          feed.stop();
          std::cerr << "shark: spliced ends could not be switched on: " << shk_strerror(rc) << " " << shk_last_error(ctx) << std::endl;
          return EXIT_FAILURE;
        }
      }
  }
  // (--sam: every worker's batches carry their mates' alignments; --fragments: the same records are what pairs mode reads)
  if (opt.sam_file || opt.fragments_file)
    for (shk_ctx *ctx : gpu.ctxs)
      if (const int rc = shk_alignments_enable(ctx, opt.sam_min_support)) {
        feed.stop();
        std::cerr << "shark: alignments mode could not be switched on: " << shk_strerror(rc) << " " << shk_last_error(ctx) << std::endl;
        return EXIT_FAILURE;
      }
  // (--indels: every worker adds its batches' events to its own table; write_indels sums the tables in worker 0's at the end)
  if (opt.indels_file)
    for (shk_ctx *ctx : gpu.ctxs)
      if (const int rc = shk_indels_enable(ctx, opt.indels_min_support, opt.indels_min_intron, opt.indels_capacity)) {
        feed.stop();
        std::cerr << "shark: indels mode could not be switched on: " << shk_strerror(rc) << " " << shk_last_error(ctx) << std::endl;
        return EXIT_FAILURE;
      }
  // (--sam-pairs, --fragments: every worker's batches carry their pair records and add to that worker's fragments state;
  //  write_fragments sums the workers' states at the end)
  if (opt.sam_pairs || opt.fragments_file)
    for (shk_ctx *ctx : gpu.ctxs)
      if (const int rc = shk_pairs_enable(ctx, opt.fragments_min_intron, opt.fragments_max, opt.fragments_bins)) {
        feed.stop();
        std::cerr << "shark: pairs mode could not be switched on: " << shk_strerror(rc) << " " << shk_last_error(ctx) << std::endl;
        return EXIT_FAILURE;
      }
  // (--sam-rescue: in front of pairs mode on the device, so --sam-pairs sees the rescued mate)
  if (opt.sam_file && opt.sam_rescue)
    for (shk_ctx *ctx : gpu.ctxs)
      if (const int rc = shk_rescue_enable(ctx, opt.fragments_min_intron, opt.fragments_max, opt.rescue_max_cost, opt.rescue_min_gap)) {
        feed.stop();
        std::cerr << "shark: rescue mode could not be switched on: " << shk_strerror(rc) << " " << shk_last_error(ctx) << std::endl;
        return EXIT_FAILURE;
      }
  std::unique_ptr<BatchSplitter> fs;
  bool serial_failed = false;
  std::thread splitter([&] { serial_feed(opt, plan, feed, order, pool, fs, serial_failed); });
  std::vector<double> t_gpu((size_t)opt.gpus, 0.0);
  // classified batches are turned into text by `n_formatters` threads, in any order (ReadOutput::format: names and qualities of
  // the associated reads are fetched from the sample files there); the drain below writes the text in input order
  BatchOrder::Queue to_format(1u << 20);
  // half as many formatters as readers: with half the sample written out again the two writer threads are what the command waits for,
  // and they get their cores only if the others leave some (-t 12 on a 16-core share, 16 M / 64 M pairs at 0.50 on-target: 0.84-0.85 /
  // 2.25 s with twelve formatters, 0.75 / 2.09 s with six, 0.81 / 2.07 s with four, 1.12 s with three -- then THEY are the wait)
  unsigned n_formatters = std::max(2u, (io_threads + 1) / 2);
  if (const char *e = getenv("SHARK_FORMATTERS")) n_formatters = (unsigned)std::max(1, atoi(e));      // (A/B timing)
  std::vector<std::thread> formatters;
  for (unsigned f = 0; f < n_formatters; ++f) {
    formatters.emplace_back([&] {
      std::unique_ptr<ReadBatch> b;
      while (to_format.pop(b)) {
        if (b->rc == SHK_OK) {
          std::shared_ptr<FormattedBatch> text = text_pool.get();
          ro.format(*b, *text);
          b->text = text;
        }
        order.finished(std::move(b));
      }
    });
  }
  std::vector<std::thread> analyzers = start_analyzers(gpu.ctxs, need_qual, opt.evidence_file != nullptr, opt.candidates_file != nullptr, opt.placements_file != nullptr,
                                                        opt.segments_file != nullptr || host_junctions, opt.sam_file != nullptr, opt.sam_file != nullptr && opt.sam_pairs,
                                                        opt.sam_file != nullptr && opt.sam_rescue, order,
                                                        to_format, t_gpu);
  // ordered drain
  int failed = 0;
  double t_out = 0;
  while (std::unique_ptr<ReadBatch> b = order.next_in_order()) {
    if (b->rc != SHK_OK) {
      failed = b->rc;
    } else {
      auto t0 = std::chrono::steady_clock::now();
      ro.emit(b->text);
      t_out += std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    }
    pool.release(std::move(b));
    order.advance();
  }
  timeline("drain done");
  splitter.join();
  for (auto &t : analyzers) t.join();
  to_format.close();
  for (auto &t : formatters) t.join();
  text_pool.retire(std::min(8u, io_threads));
  fflush(stdout);
  timeline("pipeline threads joined");
  const char *error = serial_failed                                  ? "shark: cannot open the sample"
                      : ro.failed()                                  ? "shark: cannot read the sample again for the output (or a batch came back without its evidence or candidates)"
                      : shk::parallel_gunzip_out_of_memory().load() ? "shark: out of memory while inflating the sample"
                                                                     : nullptr;
  if (error) {
    std::cerr << error << std::endl;
    return EXIT_FAILURE;
  }
  if (opt.verbose) {
    double tr = 0;
    for (double x : feed.t_reader) tr += x;
    std::cerr << "[shark/io] threads " << io_threads << ", parallel readers " << plan.n_readers << (plan.fixed_width ? " fixed-width records (" : " (") << std::min<uint64_t>(order.first_irregular(), plan.n_par_batches)
              << " batches, " << tr << " thread-seconds), serial reader: " << (fs ? "index " + std::to_string(fs->t_index) + " s (" + fs->stage_report() + "), fill " + std::to_string(fs->t_fill) + " s, serial " + std::to_string(fs->t_serial) + " s" : std::string("not needed"))
              << "; classify(gpu0) " << t_gpu[0] << " s, output " << t_out << " s" << std::endl;
    // per GPU: seconds its analyzer thread spent inside shk_classify_submit / _wait (the host-fed multi-GPU leg of bench.py reads this)
    std::cerr << "[shark/gpu-busy]";
    for (double t : t_gpu) std::cerr << " " << t;
    std::cerr << std::endl;
  }
  bool written = true;
  const bool evidence_written = !opt.evidence_file || (fclose(opt.evidence_file) == 0 && !ro.evidence_write_failed());
  const bool candidates_written = !opt.candidates_file || (fclose(opt.candidates_file) == 0 && !ro.candidates_write_failed());
  const bool placements_written = !opt.placements_file || (fclose(opt.placements_file) == 0 && !ro.placements_write_failed());
  const bool segments_written = !opt.segments_file || (fclose(opt.segments_file) == 0 && !ro.segments_write_failed());
  const bool sam_written = !opt.sam_file || (fclose(opt.sam_file) == 0 && !ro.sam_write_failed());
  bool junctions_written = true;
  if (host_junctions) {      // (--junctions-device: written by main() from the workers' tables, as --depth is)
    junctions_written = ro.write_junctions(opt.junctions_file);
    junctions_written = fclose(opt.junctions_file) == 0 && junctions_written;
  }
  if (out1) written = w1.close() && written;
  if (out2) written = w2.close() && written;
  text_pool.finish();
  if (opt.verbose)
    std::cerr << "[shark/writers] " << w1.bytes_written() << " + " << w2.bytes_written() << " bytes, busy " << w1.busy_seconds() << " + " << w2.busy_seconds() << " s" << std::endl;
  if (!written) {
    std::cerr << "shark: cannot write the output FASTQ" << std::endl;
    return EXIT_FAILURE;
  }
  if (!evidence_written) {
    std::cerr << "shark: cannot write the evidence file " << opt.evidence_path << std::endl;
    return EXIT_FAILURE;
  }
  if (!candidates_written) {
    std::cerr << "shark: cannot write the candidates file " << opt.candidates_path << std::endl;
    return EXIT_FAILURE;
  }
  if (!placements_written) {
    std::cerr << "shark: cannot write the placements file " << opt.placements_path << std::endl;
    return EXIT_FAILURE;
  }
  if (!segments_written) {
    std::cerr << "shark: cannot write the segments file " << opt.segments_path << std::endl;
    return EXIT_FAILURE;
  }
  if (!junctions_written) {
    std::cerr << "shark: cannot write the junctions file " << opt.junctions_path << std::endl;
    return EXIT_FAILURE;
  }
  if (!sam_written) {
    std::cerr << "shark: cannot write the SAM file " << opt.sam_path << std::endl;
    return EXIT_FAILURE;
  }
  if (failed) {
    std::cerr << "shark: classification failed: " << shk_strerror(failed) << std::endl;
    return EXIT_FAILURE;
  }
  timeline("output files closed");
  return EXIT_SUCCESS;
}

// per-gene assigned-read counts: the one exchange step of the sharded run (RCCL all-reduce over xGMI)
bool gene_counts(const Options &opt, std::vector<shk_ctx *> &ctxs, const std::vector<std::string> &legend_ID)
{
  const int n_gpus = opt.gpus;
  std::vector<uint64_t> totals(legend_ID.size() ? legend_ID.size() : 1, 0);
  const uint32_t ng = (uint32_t)std::min<size_t>(legend_ID.size(), 65536);
  {
    std::vector<int> distinct(opt.devices);
    std::sort(distinct.begin(), distinct.end());
    distinct.erase(std::unique(distinct.begin(), distinct.end()), distinct.end());
    if (distinct.size() != opt.devices.size())
      std::cerr << "shark: " << n_gpus << " workers on " << distinct.size() << " device(s): the per-gene counts of workers that share a device are "
                << "added on it" << (distinct.size() > 1 ? ", RCCL reduces over the distinct devices" : " (no collective)") << std::endl;
  }
  const int rc = shk_gene_counts_allreduce(ctxs.data(), n_gpus, totals.data(), ng);
  if (rc != SHK_OK) {
    std::cerr << "shark: gene count reduction failed: " << shk_strerror(rc) << " " << shk_last_error(ctxs[0]) << std::endl;
    return false;
  }
  if (opt.gene_counts_path != "") {
    FILE *gc = fopen(opt.gene_counts_path.c_str(), "w");
    if (gc) {
      for (uint32_t g = 0; g < ng; ++g)
        if (totals[g]) fprintf(gc, "%s %llu\n", legend_ID[g].c_str(), (unsigned long long)totals[g]);
      fclose(gc);
    }
  }
  if (opt.verbose) {
    uint64_t sum = 0;
    for (uint32_t g = 0; g < ng; ++g) sum += totals[g];
    std::cerr << "[shark/counts] " << sum << " associations over " << n_gpus << " GPU(s)" << std::endl;
  }
  return true;
}

// --depth: the workers' depth arrays (one per context, each over the batches that worker classified) summed on the host -- depth is
// additive over contexts --, then one line per maximal run of equal depth >= 1: <gene> <start> <end> <depth>, genes in id order
bool write_depth(const Options &opt, std::vector<shk_ctx *> &ctxs, const std::vector<std::string> &legend_ID)
{
  shk_index_info info{};
  shk_index_info_get(ctxs[0], &info);
  const uint32_t n_genes = (uint32_t)info.nidx;
  std::vector<uint64_t> gene_start((size_t)n_genes + 1, 0);
  int rc = shk_depth_layout(ctxs[0], gene_start.data(), n_genes);
  if (rc != SHK_OK) {
    std::cerr << "shark: the depth layout could not be read: " << shk_strerror(rc) << " " << shk_last_error(ctxs[0]) << std::endl;
    fclose(opt.depth_file);
    return false;
  }
  std::vector<uint32_t> depth((size_t)gene_start[n_genes], 0), part;
  for (size_t g = 0; g < ctxs.size() && rc == SHK_OK; ++g) {
    std::vector<uint32_t> &into = g == 0 ? depth : part;
    into.assign(depth.size(), 0);
    rc = shk_depth_get_all(ctxs[g], into.data(), into.size(), 0);
    if (g != 0 && rc == SHK_OK)
      for (size_t x = 0; x < depth.size(); ++x) depth[x] += part[x];
    if (rc != SHK_OK) std::cerr << "shark: the depth of worker " << g << " could not be read: " << shk_strerror(rc) << " " << shk_last_error(ctxs[g]) << std::endl;
  }
  if (rc != SHK_OK) {
    fclose(opt.depth_file);
    return false;
  }
  std::string text;
  bool ok = true;
  for (uint32_t g = 0; g < n_genes; ++g) {
    const uint32_t *d = depth.data() + gene_start[g];
    const uint64_t len = gene_start[g + 1] - gene_start[g];
    const std::string &name = g < legend_ID.size() ? legend_ID[g] : std::string();
    for (uint64_t x = 0; x < len;) {
      uint64_t e = x + 1;
      while (e < len && d[e] == d[x]) ++e;
      if (d[x]) {
        text += name;
        text += ' '; text += std::to_string(x);
        text += ' '; text += std::to_string(e);
        text += ' '; text += std::to_string(d[x]);
        text += '\n';
      }
      x = e;
    }
    if (text.size() > (1u << 20) || g + 1 == n_genes) {
      ok = ok && fwrite(text.data(), 1, text.size(), opt.depth_file) == text.size();
      text.clear();
    }
  }
  ok = (fclose(opt.depth_file) == 0) && ok;
  if (!ok) std::cerr << "shark: cannot write the depth file " << opt.depth_path << std::endl;
  return ok;
}

// --junctions --junctions-device: the workers' tables (one per context, each over the batches that worker classified) merged on the
// host -- mates add up, the intron is the smallest --, then --junctions' lines in its order.  A table that was full is an error and
// leaves an empty file, never a shorter table
bool write_junctions_device(const Options &opt, std::vector<shk_ctx *> &ctxs, const std::vector<std::string> &legend_ID)
{
  std::map<std::tuple<uint32_t, uint32_t, uint32_t>, std::pair<uint32_t, uint64_t>> table;   // (gene, donor, acceptor) -> intron, mates
  std::vector<shk_junction> rows;
  for (size_t g = 0; g < ctxs.size(); ++g) {
    uint64_t n = 0;
    int rc = shk_junctions_get(ctxs[g], nullptr, 0, &n);
    rows.resize((size_t)n);
    if (rc == SHK_OK && n) rc = shk_junctions_get(ctxs[g], rows.data(), n, &n);
    if (rc != SHK_OK) {
      std::cerr << "shark: the junction table of worker " << g << " could not be read: " << shk_strerror(rc) << " " << shk_last_error(ctxs[g])
                << (rc == SHK_ERR_INDEX_TOO_LARGE ? " (run again with a larger --junctions-capacity)" : "") << std::endl;
      fclose(opt.junctions_file);
      return false;
    }
    for (const shk_junction &j : rows) {
      auto it = table.emplace(std::make_tuple(j.gene, j.donor, j.acceptor), std::make_pair(j.intron, (uint64_t)0)).first;
      it->second.first = std::min(it->second.first, j.intron);
      it->second.second += j.mates;
    }
  }
  std::string text;
  for (const auto &kv : table) {
    const uint32_t g = std::get<0>(kv.first);
    text += g < legend_ID.size() ? legend_ID[g] : std::string();
    text += ' '; text += std::to_string(std::get<1>(kv.first));
    text += ' '; text += std::to_string(std::get<2>(kv.first));
    text += ' '; text += std::to_string(kv.second.first);
    text += ' '; text += std::to_string(kv.second.second);
    text += '\n';
  }
  bool ok = fwrite(text.data(), 1, text.size(), opt.junctions_file) == text.size();
  ok = (fclose(opt.junctions_file) == 0) && ok;
  if (!ok) std::cerr << "shark: cannot write the junctions file " << opt.junctions_path << std::endl;
  return ok;
}

// --pileup: the workers' counters (one array per context, each over the batches that worker classified) summed on the host -- the
// counts are additive over contexts --, then one line per record base with at least one observation: <gene> <x> <A> <C> <G> <T>,
// genes in id order, x ascending
bool write_pileup(const Options &opt, std::vector<shk_ctx *> &ctxs, const std::vector<std::string> &legend_ID)
{
  shk_index_info info{};
  shk_index_info_get(ctxs[0], &info);
  const uint32_t n_genes = (uint32_t)info.nidx;
  std::vector<uint64_t> gene_start((size_t)n_genes + 1, 0);
  int rc = shk_depth_layout(ctxs[0], gene_start.data(), n_genes);
  if (rc != SHK_OK) {
    std::cerr << "shark: the pileup layout could not be read: " << shk_strerror(rc) << " " << shk_last_error(ctxs[0]) << std::endl;
    fclose(opt.pileup_file);
    return false;
  }
  std::vector<uint32_t> counts((size_t)gene_start[n_genes] * 4, 0), part;
  for (size_t g = 0; g < ctxs.size() && rc == SHK_OK; ++g) {
    std::vector<uint32_t> &into = g == 0 ? counts : part;
    into.assign(counts.size(), 0);
    rc = shk_pileup_get_all(ctxs[g], into.data(), into.size(), 0);
    if (g != 0 && rc == SHK_OK)
      for (size_t x = 0; x < counts.size(); ++x) counts[x] += part[x];
    if (rc != SHK_OK) std::cerr << "shark: the pileup of worker " << g << " could not be read: " << shk_strerror(rc) << " " << shk_last_error(ctxs[g]) << std::endl;
  }
  if (rc != SHK_OK) {
    fclose(opt.pileup_file);
    return false;
  }
  std::string text;
  bool ok = true;
  for (uint32_t g = 0; g < n_genes; ++g) {
    const uint32_t *c = counts.data() + gene_start[g] * 4;
    const uint64_t len = gene_start[g + 1] - gene_start[g];
    const std::string &name = g < legend_ID.size() ? legend_ID[g] : std::string();
    for (uint64_t x = 0; x < len; ++x) {
      const uint32_t *b = c + x * 4;
      if (!(b[0] | b[1] | b[2] | b[3])) continue;
      text += name;
      text += ' '; text += std::to_string(x);
      for (int i = 0; i < 4; ++i) { text += ' '; text += std::to_string(b[i]); }
      text += '\n';
    }
    if (text.size() > (1u << 20) || g + 1 == n_genes) {
      ok = ok && fwrite(text.data(), 1, text.size(), opt.pileup_file) == text.size();
      text.clear();
    }
  }
  ok = (fclose(opt.pileup_file) == 0) && ok;
  if (!ok) std::cerr << "shark: cannot write the pileup file " << opt.pileup_path << std::endl;
  return ok;
}

// --fragments: the workers' fragments states (one per context, each over the batches that worker classified) summed on the host -- both
// arrays are additive over contexts --, then six lines `class <name> <count>`, one line `frag <len> <count>` per non-empty bin below the
// last and `frag >=<n_bins - 1> <count>` for the last, the overflow bin
bool write_fragments(const Options &opt, std::vector<shk_ctx *> &ctxs)
{
  static const char *const names[6] = {"none", "mate1", "mate2", "inward", "outward", "tandem"};
  const uint32_t n_bins = opt.fragments_bins;
  std::vector<uint64_t> hist(n_bins, 0), part(n_bins, 0);
  uint64_t classes[6] = {0, 0, 0, 0, 0, 0}, cpart[6];
  for (size_t g = 0; g < ctxs.size(); ++g) {
    const int rc = shk_fragments_get(ctxs[g], part.data(), n_bins, cpart);
    if (rc != SHK_OK) {
      std::cerr << "shark: the fragments state of worker " << g << " could not be read: " << shk_strerror(rc) << " " << shk_last_error(ctxs[g]) << std::endl;
      fclose(opt.fragments_file);
      return false;
    }
    for (uint32_t b = 0; b < n_bins; ++b) hist[b] += part[b];
    for (int c = 0; c < 6; ++c) classes[c] += cpart[c];
  }
  std::string text;
  for (int c = 0; c < 6; ++c) text += std::string("class ") + names[c] + " " + std::to_string(classes[c]) + "\n";
  for (uint32_t b = 0; b + 1 < n_bins; ++b)
    if (hist[b]) text += "frag " + std::to_string(b) + " " + std::to_string(hist[b]) + "\n";
  text += "frag >=" + std::to_string(n_bins - 1) + " " + std::to_string(hist[n_bins - 1]) + "\n";
  bool ok = fwrite(text.data(), 1, text.size(), opt.fragments_file) == text.size();
  ok = (fclose(opt.fragments_file) == 0) && ok;
  if (!ok) std::cerr << "shark: cannot write the fragments file " << opt.fragments_path << std::endl;
  return ok;
}

// --indels: the workers' tables (one per context, each over the batches that worker classified) and their counters added into worker 0's
// on its device (shk_indels_get, shk_indels_stats, shk_indels_add), then worker 0 is asked once for the events with --indels-min-mates
// mates: one line each (indel_host.hpp) in the library's order.  The counters go to the log.  A table that was full -- a worker's or the
// sum -- is an error and leaves an empty file, never a shorter table
bool write_indels(const Options &opt, std::vector<shk_ctx *> &ctxs, const std::vector<std::string> &legend_ID)
{
  int rc = SHK_OK;
  size_t at = 0;
  std::vector<shk_indel> rows;
  uint64_t n = 0;
  for (size_t g = 1; g < ctxs.size() && rc == SHK_OK; ++g) {
    at = g;
    shk_indel_stats st{};
    rc = shk_indels_get(ctxs[g], 0, nullptr, 0, &n);
    rows.resize((size_t)n);
    if (rc == SHK_OK && n) rc = shk_indels_get(ctxs[g], 0, rows.data(), n, &n);
    if (rc == SHK_OK) rc = shk_indels_stats(ctxs[g], &st);
    if (rc == SHK_OK) {
      at = 0;
      rc = shk_indels_add(ctxs[0], rows.data(), n, &st);
    }
  }
  shk_indel_stats st{};
  if (rc == SHK_OK) {
    at = 0;
    rc = shk_indels_get(ctxs[0], opt.indels_min_mates, nullptr, 0, &n);
    rows.resize((size_t)n);
    if (rc == SHK_OK && n) rc = shk_indels_get(ctxs[0], opt.indels_min_mates, rows.data(), n, &n);
    if (rc == SHK_OK) rc = shk_indels_stats(ctxs[0], &st);
  }
  if (rc != SHK_OK) {
    std::cerr << "shark: the indel table of worker " << at << " could not be read: " << shk_strerror(rc) << " " << shk_last_error(ctxs[at])
              << (rc == SHK_ERR_INDEX_TOO_LARGE ? " (run again with a larger --indels-capacity)" : "") << std::endl;
    fclose(opt.indels_file);
    return false;
  }
  pelapsed("Indels: " + std::to_string(st.mates) + " aligned mates, " + std::to_string(st.deletions) + " deletions, " + std::to_string(st.insertions) +
           " insertions, " + std::to_string(st.complex_gaps) + " complex gaps, " + std::to_string(st.long_insertions) + " long and " +
           std::to_string(st.nonbase_insertions) + " non-base insertions; " + std::to_string(n) + " events written");
  std::string text;
  static const std::string no_name;
  for (const shk_indel &e : rows) shk::indel_line(e, e.gene < legend_ID.size() ? legend_ID[e.gene] : no_name, text);
  bool ok = fwrite(text.data(), 1, text.size(), opt.indels_file) == text.size();
  ok = (fclose(opt.indels_file) == 0) && ok;
  if (!ok) std::cerr << "shark: cannot write the indels file " << opt.indels_path << std::endl;
  return ok;
}

// --variants: a variant call is not linear in the counters, so the workers' states are summed first -- every other worker's array and
// mate counter added into worker 0's on its device (shk_pileup_get_all, shk_pileup_add) -- and worker 0 is asked once.  One line per
// site: <gene> <x> <ref> <alt> <A> <C> <G> <T>, genes in id order, x ascending (the order the library hands them out in).  Runs behind
// write_pileup: what it does to worker 0's state nobody reads afterwards
bool write_variants(const Options &opt, std::vector<shk_ctx *> &ctxs, const std::vector<std::string> &legend_ID)
{
  shk_index_info info{};
  shk_index_info_get(ctxs[0], &info);
  std::vector<uint64_t> gene_start((size_t)info.nidx + 1, 0);
  int rc = ctxs.size() > 1 ? shk_depth_layout(ctxs[0], gene_start.data(), (uint32_t)info.nidx) : SHK_OK;
  std::vector<uint32_t> part;
  for (size_t g = 1; g < ctxs.size() && rc == SHK_OK; ++g) {
    uint64_t mates = 0;
    part.assign((size_t)gene_start[info.nidx] * 4, 0);
    // (shk_pileup_mates stores the number even behind its guard; get_all refuses there, and so would the sum)
    rc = shk_pileup_get_all(ctxs[g], part.data(), part.size(), 0);
    if (rc == SHK_OK) rc = shk_pileup_mates(ctxs[g], &mates);
    if (rc != SHK_OK) { std::cerr << "shark: the pileup of worker " << g << " could not be read: " << shk_strerror(rc) << " " << shk_last_error(ctxs[g]) << std::endl; break; }
    rc = shk_pileup_add(ctxs[0], part.data(), part.size(), mates, 0);
  }
  uint64_t n = 0;
  std::vector<shk_variant> sites;
  if (rc == SHK_OK) rc = shk_variants_get(ctxs[0], &opt.variants_params, nullptr, 0, &n);
  if (rc == SHK_OK && n) {
    sites.resize((size_t)n);
    rc = shk_variants_get(ctxs[0], &opt.variants_params, sites.data(), sites.size(), &n);
  }
  if (rc != SHK_OK) {
    std::cerr << "shark: the variants could not be read: " << shk_strerror(rc) << " " << shk_last_error(ctxs[0]) << std::endl;
    fclose(opt.variants_file);
    return false;
  }
  std::string text;
  for (const shk_variant &v : sites) {
    text += v.gene < legend_ID.size() ? legend_ID[v.gene] : std::string();
    text += ' '; text += std::to_string(v.x);
    text += ' '; text += "ACGT"[v.ref & 3u];
    text += ' '; text += "ACGT"[v.alt & 3u];
    for (int i = 0; i < 4; ++i) { text += ' '; text += std::to_string(v.n[i]); }
    text += '\n';
  }
  bool ok = fwrite(text.data(), 1, text.size(), opt.variants_file) == text.size();
  ok = (fclose(opt.variants_file) == 0) && ok;
  if (!ok) std::cerr << "shark: cannot write the variants file " << opt.variants_path << std::endl;
  return ok;
}

}  // namespace

int main(int argc, char *argv[])
{
  Options opt_parsed = parse_arguments(argc, argv);
  if (!opt_parsed.batch_given) opt_parsed.batch = auto_batch(opt_parsed.sample1_path, opt_parsed.batch);
  // (--evidence: the file is created only once the samples are known to be readable -- a run that fails on its inputs leaves an
  //  earlier evidence file alone)
  if (opt_parsed.evidence_path != "" && samples_can_be_opened(opt_parsed, false)) opt_parsed.evidence_file = fopen(opt_parsed.evidence_path.c_str(), "w");
  if (opt_parsed.candidates_path != "" && samples_can_be_opened(opt_parsed, false)) opt_parsed.candidates_file = fopen(opt_parsed.candidates_path.c_str(), "w");   // (--candidates: likewise)
  if (opt_parsed.placements_path != "" && samples_can_be_opened(opt_parsed, false)) opt_parsed.placements_file = fopen(opt_parsed.placements_path.c_str(), "w");   // (--placements: likewise)
  if (opt_parsed.depth_path != "" && samples_can_be_opened(opt_parsed, false)) opt_parsed.depth_file = fopen(opt_parsed.depth_path.c_str(), "w");   // (--depth: likewise)
  if (opt_parsed.segments_path != "" && samples_can_be_opened(opt_parsed, false)) opt_parsed.segments_file = fopen(opt_parsed.segments_path.c_str(), "w");   // (--segments: likewise)
  if (opt_parsed.junctions_path != "" && samples_can_be_opened(opt_parsed, false)) opt_parsed.junctions_file = fopen(opt_parsed.junctions_path.c_str(), "w");   // (--junctions: likewise)
  if (opt_parsed.pileup_path != "" && samples_can_be_opened(opt_parsed, false)) opt_parsed.pileup_file = fopen(opt_parsed.pileup_path.c_str(), "w");   // (--pileup: likewise)
  if (opt_parsed.variants_path != "" && samples_can_be_opened(opt_parsed, false)) opt_parsed.variants_file = fopen(opt_parsed.variants_path.c_str(), "w");   // (--variants: likewise)
  if (opt_parsed.sam_path != "" && samples_can_be_opened(opt_parsed, false)) opt_parsed.sam_file = fopen(opt_parsed.sam_path.c_str(), "w");   // (--sam: likewise)
  if (opt_parsed.fragments_path != "" && samples_can_be_opened(opt_parsed, false)) opt_parsed.fragments_file = fopen(opt_parsed.fragments_path.c_str(), "w");   // (--fragments: likewise)
  if (opt_parsed.indels_path != "" && samples_can_be_opened(opt_parsed, false)) opt_parsed.indels_file = fopen(opt_parsed.indels_path.c_str(), "w");   // (--indels: likewise)
  const Options opt = opt_parsed;
  if (opt.verbose) timeline.on();
  timeline("arguments parsed");
  if (opt.verbose) {
    std::cerr << "shark (MI355X): reference " << opt.fasta_path << ", sample " << opt.sample1_path;
    if (opt.paired_flag) std::cerr << " + " << opt.sample2_path;
    std::cerr << "; k=" << opt.k << " c=" << opt.c << " q=" << opt.min_quality << (opt.single ? " single" : "") << " bf=" << (opt.bf_size >> 33)
              << "GB gpus=" << opt.gpus << " devices=";
    for (size_t g = 0; g < opt.devices.size(); ++g) std::cerr << (g ? "," : "") << opt.devices[g];
    std::cerr << "\n" << std::endl;
  }
  if (!samples_can_be_opened(opt)) return EXIT_FAILURE;
  if (opt.evidence_path != "" && !opt.evidence_file) {   // (the samples are there: it is the evidence file that could not be opened)
    std::cerr << "shark: cannot open the evidence file " << opt.evidence_path << std::endl;
    return EXIT_FAILURE;
  }
  if (opt.candidates_path != "" && !opt.candidates_file) {
    std::cerr << "shark: cannot open the candidates file " << opt.candidates_path << std::endl;
    return EXIT_FAILURE;
  }
  if (opt.placements_path != "" && !opt.placements_file) {
    std::cerr << "shark: cannot open the placements file " << opt.placements_path << std::endl;
    return EXIT_FAILURE;
  }

  if (opt.depth_path != "" && !opt.depth_file) {
    std::cerr << "shark: cannot open the depth file " << opt.depth_path << std::endl;
    return EXIT_FAILURE;
  }

  if (opt.segments_path != "" && !opt.segments_file) {
    std::cerr << "shark: cannot open the segments file " << opt.segments_path << std::endl;
    return EXIT_FAILURE;
  }
  if (opt.junctions_path != "" && !opt.junctions_file) {
    std::cerr << "shark: cannot open the junctions file " << opt.junctions_path << std::endl;
    return EXIT_FAILURE;
  }
  if (opt.pileup_path != "" && !opt.pileup_file) {
    std::cerr << "shark: cannot open the pileup file " << opt.pileup_path << std::endl;
    return EXIT_FAILURE;
  }
  if (opt.variants_path != "" && !opt.variants_file) {
    std::cerr << "shark: cannot open the variants file " << opt.variants_path << std::endl;
    return EXIT_FAILURE;
  }
  if (opt.sam_path != "" && !opt.sam_file) {
    std::cerr << "shark: cannot open the SAM file " << opt.sam_path << std::endl;
    return EXIT_FAILURE;
  }
  if (opt.fragments_path != "" && !opt.fragments_file) {
    std::cerr << "shark: cannot open the fragments file " << opt.fragments_path << std::endl;
    return EXIT_FAILURE;
  }
  if (opt.indels_path != "" && !opt.indels_file) {
    std::cerr << "shark: cannot open the indels file " << opt.indels_path << std::endl;
    return EXIT_FAILURE;
  }

  BatchPool &pool = *new BatchPool;     // (never destroyed: the process leaves through _exit)
  GpuStart gpu(opt, pool);              // the contexts come up on a thread of their own from here on
  std::vector<std::string> legend_ID;   // gene names in file order (FastaSplitter.hpp:48); filled by build_index, read by the output stage
  if (const int rc = run_sample(opt, gpu, pool, legend_ID)) return rc;
  timeline("outputs closed");
  pelapsed("Sample completed");
  if (opt.depth_file && !write_depth(opt, gpu.ctxs, legend_ID)) return EXIT_FAILURE;
  if (opt.junctions_file && opt.junctions_device && !write_junctions_device(opt, gpu.ctxs, legend_ID)) return EXIT_FAILURE;
  if (opt.pileup_file && !write_pileup(opt, gpu.ctxs, legend_ID)) return EXIT_FAILURE;
  if (opt.variants_file && !write_variants(opt, gpu.ctxs, legend_ID)) return EXIT_FAILURE;
  if (opt.fragments_file && !write_fragments(opt, gpu.ctxs)) return EXIT_FAILURE;
  if (opt.indels_file && !write_indels(opt, gpu.ctxs, legend_ID)) return EXIT_FAILURE;

  if ((opt.gene_counts_path != "" || (opt.verbose && opt.gpus > 1)) && !gene_counts(opt, gpu.ctxs, legend_ID)) return EXIT_FAILURE;
  if (opt.verbose) {
    // (what the process still holds is what its end has to give back: resident and peak resident memory)
    std::ifstream st("/proc/self/status");
    std::string line;
    while (std::getline(st, line))
      if (line.compare(0, 6, "VmRSS:") == 0 || line.compare(0, 6, "VmHWM:") == 0 || line.compare(0, 8, "RssAnon:") == 0 || line.compare(0, 9, "RssShmem:") == 0)
        std::cerr << "[shark/mem] " << line << std::endl;
  }
  gpu.join();
  for (auto *ctx : gpu.ctxs) shk_destroy(ctx);
  timeline("contexts destroyed");
  pelapsed("Association done");
  // everything is written and closed; leaving through _exit skips the teardown of the HIP runtime and of the worker threads'
  // statics, which costs more than a tenth of a second and changes nothing
  fflush(stdout);
  fflush(stderr);
  // (a profiler writes its results from exit handlers: under one -- ROCP_TOOL_LIBRARIES, or an LD_PRELOAD that names a rocprofiler
  //  library -- or when asked to (SHARK_CLEAN_EXIT=1), leave the ordinary way.  Any other preloaded library, an allocator say, does
  //  not change how the process leaves.  The contexts are destroyed above: exit handlers find no live context.)
  bool clean_exit = false;
  if (const char *v = getenv("ROCP_TOOL_LIBRARIES")) clean_exit = v[0] != 0;
  if (const char *v = getenv("SHARK_CLEAN_EXIT")) clean_exit = clean_exit || (v[0] != 0 && v[0] != '0');
  if (const char *v = getenv("LD_PRELOAD")) clean_exit = clean_exit || strstr(v, "rocprof") != nullptr || strstr(v, "roctracer") != nullptr;
  if (clean_exit) exit(0);
  _exit(0);
}
