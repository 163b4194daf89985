#!/bin/bash
# usage (on the GPU box): tests/prof_bench.sh <tag>   -> $PROF_OUT/<tag>_{bench.json,stats,fetch,write} (PROF_OUT: default prof_out/ in the repository)
cd /tmp && export TMPDIR=/tmp
R=$GRAFT_REPO_ROOT
tag=$1
O=${PROF_OUT:-$R/prof_out}
mkdir -p $O
rm -rf $O/${tag}_stats $O/${tag}_fetch $O/${tag}_write   # (stale runs would be summarised too)
python3 $R/bench.py --full --steps 2 --warmup 1 > $O/${tag}_bench.json 2> $O/${tag}_bench.err
rocprofv3 --kernel-trace --stats --output-format csv -d $O/${tag}_stats -- python3 $R/bench.py --steps 2 --warmup 1 --no-cpu-baseline --no-checks --no-host-path --no-v1 --no-copy-probe --bzip2-mib 0 --lzma-entries 0 > $O/${tag}_stats.log 2>&1
rocprofv3 --pmc FETCH_SIZE --output-format csv -d $O/${tag}_fetch -- python3 $R/bench.py --steps 1 --warmup 0 --no-cpu-baseline --no-checks --no-host-path --no-v1 --no-copy-probe --bzip2-mib 0 --lzma-entries 0 > $O/${tag}_fetch.log 2>&1
rocprofv3 --pmc WRITE_SIZE --output-format csv -d $O/${tag}_write -- python3 $R/bench.py --steps 1 --warmup 0 --no-cpu-baseline --no-checks --no-host-path --no-v1 --no-copy-probe --bzip2-mib 0 --lzma-entries 0 > $O/${tag}_write.log 2>&1
