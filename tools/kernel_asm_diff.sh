#!/usr/bin/env bash
# kernel_asm_diff.sh [REV] -- are the kernels of this tree the kernels of REV (default HEAD)?  Needs no GPU.
# Every .hip of the Makefile's SRCS is compiled twice, from REV's sources and from the working tree's, with the Makefile's flags for that file plus
# --offload-device-only -S -fuse-cuid=none (without the last, two compilations differ in the __hip_cuid_* symbol alone), and the two gfx950 assembly files are compared.
# One line per file on stdout ("same" / "DIFFERENT"); exit status 1 if any differs.  A refactor of host code must print 31 x same.
set -euo pipefail
REV=${1:-HEAD}
ROOT=$(cd "$(dirname "$0")/.." && pwd)
HIPCC=${HIPCC:-/opt/rocm/bin/hipcc}
JOBS=${JOBS:-8}
TMP=$(mktemp -d)
trap 'rm -rf "$TMP"' EXIT
mkdir -p "$TMP/old" "$TMP/asm_old" "$TMP/asm_new"
git -C "$ROOT" archive "$REV" nerfpp_amd/csrc include | tar -x -C "$TMP/old"
SRCS=$(make -s -C "$ROOT/nerfpp_amd/csrc" -pn 2>/dev/null | sed -n 's/^SRCS = //p' | head -1)
flags_of() { make -s -C "$1" -pn 2>/dev/null | sed -n "s/^FLAGS_$2 = //p" | head -1; }
compile() {   # tree, source, output
    local csrc=$1/nerfpp_amd/csrc name=${2%.hip}
    (cd "$csrc" && $HIPCC -std=c++17 -O3 -fPIC --offload-arch=gfx950 -ffp-contract=off -fvisibility=hidden -I../../include -I. -Wall -Wno-unused-function $(flags_of "$csrc" "$name") \
        --offload-device-only -S -fuse-cuid=none "$2" -o "$3")
}
export -f compile flags_of
export HIPCC TMP ROOT
printf '%s\n' $SRCS | xargs -P "$JOBS" -I{} bash -c 'compile "$TMP/old" {} "$TMP/asm_old/{}.s" && compile "$ROOT" {} "$TMP/asm_new/{}.s"'
rc=0
for f in $SRCS; do
    if cmp -s "$TMP/asm_old/$f.s" "$TMP/asm_new/$f.s"; then echo "$f: same ($(wc -l < "$TMP/asm_new/$f.s") lines)"; else echo "$f: DIFFERENT"; rc=1; fi
done
echo "compared $(echo $SRCS | wc -w) files against $(git -C "$ROOT" rev-parse --short "$REV")"
exit $rc
