#!/bin/bash
# usage: tools/pmc_run.sh <tag> <counters...> -- <python script args>
# collects PMC counters in their own pass (kernel-trace only), output under $OUT/<tag> (OUT: see tools/profile_round.sh)
tag=$1; shift
ctrs=()
while [ "$1" != "--" ]; do ctrs+=("$1"); shift; done
shift
export TMPDIR=/tmp && cd "$(dirname "$0")/.." || exit 1
OUT=${OUT:?OUT names the directory the results are collected in}
timeout 600 rocprofv3 --kernel-trace --pmc "${ctrs[@]}" -d $OUT/$tag -o $tag -- python3 "$@" > $OUT/$tag.log 2>&1
echo "rc=$?"
