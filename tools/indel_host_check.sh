#!/bin/bash
# The host-only parts of indels mode (shark_amd/csrc/indel_host.hpp: shk_indels_add's entry validation, `shark --indels`' line writer)
# as a stand-alone program under AddressSanitizer and UndefinedBehaviorSanitizer.  CPU only: no device, no library, nothing preloaded.
set -e
cd "$(dirname "$0")/.."
T=$(mktemp -d)
trap 'rm -rf "$T"' EXIT
g++ -std=c++17 -O1 -g -Wall -fsanitize=address,undefined -fno-sanitize-recover=all -o "$T/indel_host_check" shark_amd/csrc/indel_host_check_tool.cpp
"$T/indel_host_check"
