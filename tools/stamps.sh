#!/bin/bash
# The diagnostic build behind profiles/r05_headline_stamps.json: classify_uni_u5.hip with -DSHK_STAMPS=1 (s_memtime stamps at the phase
# boundaries of the three-pairs kernel, classify_uni.hpp) linked with the product's other objects into tools/variants/<name>.so.
#   bash tools/stamps.sh [name [extra compiler flags]]      (name: stamps)
#   SHK_LIB_PATH=$PWD/tools/variants/stamps.so python3 tools/headline_stamps.py
# The objects are the Makefile's own list (make print-objs), whatever the library has grown to: only classify_uni_u5.o is replaced.
set -e
name=${1:-stamps}; shift || true
cd "$(dirname "$0")/../shark_amd/csrc"
HIPCC=${HIPCC:-/opt/rocm/bin/hipcc}
make -j8 > /dev/null
objs=$(make -s --no-print-directory print-objs)
case " $objs " in *" classify_uni_u5.o "*) ;; *) echo "classify_uni_u5.o is not among the library's objects: $objs" >&2; exit 1 ;; esac
mkdir -p ../../tools/variants
stamped=../../tools/variants/classify_uni_u5_$name.o
$HIPCC --offload-arch=gfx950 -O3 -std=c++17 -fPIC -Wall -Wno-unused-result -Wno-unused-value -Wno-pass-failed -fno-gpu-rdc -DSHK_STAMPS=1 "$@" \
  -c classify_uni_u5.hip -o $stamped
$HIPCC --offload-arch=gfx950 -shared -fPIC -o ../../tools/variants/$name.so $(echo " $objs " | sed "s| classify_uni_u5.o | $stamped |") -ldl
echo tools/variants/$name.so
