#!/bin/bash
# Build libsphx from the sources of a COMMIT as a variant library:  tools/ab_build_commit.sh NAME COMMIT [-DFOO ...]
# (same-box A/B against the working tree's library: SPHX_LIB=yasph2d_amd/variants/libsphx_NAME.so)
# The commit's whole yasph2d_amd/csrc and include go to a temporary directory and are built there by the commit's own Makefile, with
# its CXXFLAGS plus the extra flags: every object is the commit's, nothing comes from the working tree.  AB_KEEP_SRC=1 keeps the
# directory (with --save-temps among the flags its device assembly is what tools/isa_compare.py reads).
set -e
root="$(cd "$(dirname "$0")/.." && pwd)"
name=$1; commit=$2; shift 2
d=$(mktemp -d "${TMPDIR:-/tmp}/ab_src_$name.XXXXXX")
[ -n "$AB_KEEP_SRC" ] && echo "sources kept in $d" || trap 'rm -rf "$d"' EXIT
git -C "$root" archive "$commit" yasph2d_amd/csrc include | tar -x -C "$d"
flags="$(sed -n 's/^CXXFLAGS *?= *//p' "$d/yasph2d_amd/csrc/Makefile") $*"
make -C "$d/yasph2d_amd/csrc" ARCH=gfx950 CXXFLAGS="$flags" ../libsphx.so
mkdir -p "$root/yasph2d_amd/variants"
cp "$d/yasph2d_amd/libsphx.so" "$root/yasph2d_amd/variants/libsphx_$name.so"
echo "built yasph2d_amd/variants/libsphx_$name.so from $commit"
