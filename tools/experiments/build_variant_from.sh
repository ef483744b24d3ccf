#!/bin/bash
# build_variant_from.sh NAME GIT_REV [-DFLAG ...]: libstatmc_hip.so from a git revision (A/B runs of two source versions on
# one box) -> tools/experiments/variants/NAME.so.  The revision's own statmc_amd/build.py compiles it: every source in its
# SOURCES against its headers, with its FLAGS (+ the extra flags) and KERNEL_FLAGS where its build() adds them.
set -e
ROOT=$(cd "$(dirname "$0")/../.." && pwd)
NAME=$1; REV=$2; shift; shift
OUT=$ROOT/tools/experiments/variants
SRC=$OUT/src_$NAME
rm -rf $SRC; mkdir -p $SRC
git -C $ROOT archive $REV statmc_amd/build.py statmc_amd/csrc include | tar -x -C $SRC
python3 - $SRC/statmc_amd "$@" <<'PY'
import sys
sys.path.insert(0, sys.argv[1])
import build
build.FLAGS += sys.argv[2:]
build.build(force=True)
PY
cp $SRC/statmc_amd/libstatmc_hip.so $OUT/$NAME.so
rm -rf $SRC
echo $OUT/$NAME.so
