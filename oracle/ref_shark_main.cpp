/*
 * ref_shark_main.cpp -- wrapper translation unit that compiles the
 * reference's own main.cpp, unchanged and in place, into oracle/_ref/shark_ref
 * (test infrastructure; see the `ref` target of oracle/Makefile).  sdsl-lite
 * is replaced by our stand-in under oracle/sdsl_standin/.
 *
 * The one addition: `-b` takes whole GiB only (a multiple of 2^33 bits), so a
 * test-only variable REF_BF_BITS, when set, overrides the filter size in bits
 * after the arguments are parsed.  argument_parser.hpp is included first; its
 * include guard keeps main.cpp from including it a second time, and the macro
 * below sends main()'s call to the wrapper.
 */
#include <cstdlib>
#include <sys/types.h>

#include "argument_parser.hpp"

static void ref_parse_arguments(int argc, char **argv)
{
  parse_arguments(argc, argv);
  if (const char *bits = std::getenv("REF_BF_BITS"))
    opt::bf_size = std::strtoull(bits, nullptr, 10);
}

#define parse_arguments ref_parse_arguments
#include "main.cpp"
