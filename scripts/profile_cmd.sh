#!/bin/bash
# Run on the GPU box (via gpurun): rocprofv3 kernel-trace summary of an arbitrary command.
#   scripts/profile_cmd.sh <tag> <command...>   ->  $OUT/kstats_<tag>.txt
set -u
OUT=$(realpath -m "${OUT:-out}")
tag=$1; shift
REPO=$PWD
mkdir -p $OUT
cd /tmp && export TMPDIR=/tmp
rm -rf /tmp/prof_$tag
( cd $REPO && rocprofv3 --kernel-trace --stats -d /tmp/prof_$tag -o p -- "$@" > $OUT/prof_$tag.out 2> $OUT/prof_$tag.err )
cd $REPO
db=$(find /tmp/prof_$tag -name "*.db" | head -1)
python scripts/kstats.py "$db" 30 > $OUT/kstats_$tag.txt 2>&1
