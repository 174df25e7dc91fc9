#!/bin/bash
# helper run on the GPU box: tests + smoke + bench lines + rocprofv3 kernel-trace summaries (copied into profiles/<round> afterwards)
set -u
OUT=${OUT:-out}                 # results, under the repository root
tag=${1:-t}
mkdir -p $OUT
(timeout 900 python -m pytest tests -m gpu -q 2>&1 | tail -40) > $OUT/${tag}_tests.log 2>&1
(timeout 300 python -c "import __graft_entry__ as g; g.smoke()" 2>&1 | tail -5) > $OUT/${tag}_smoke.log 2>&1
(timeout 900 python bench.py --full 2>$OUT/${tag}_bench_default.err | tail -1) > $OUT/${tag}_bench_default.json
(timeout 600 python bench.py --full --precision f16 --no-cpu-baseline --no-also 2>/dev/null | tail -1) > $OUT/${tag}_bench_hashnerf_f16.json
(timeout 600 python bench.py --full --steps 3 --warmup 1 --precision f32 --no-cpu-baseline --no-also 2>/dev/null | tail -1) > $OUT/${tag}_bench_hashnerf_f32.json
(timeout 600 python bench.py --full --workload classic --steps 5 --warmup 1 --no-also 2>/dev/null | tail -1) > $OUT/${tag}_bench_classic_f16x3.json
(timeout 600 python bench.py --full --workload classic --precision f16 --steps 5 --warmup 1 --no-also --no-cpu-baseline 2>/dev/null | tail -1) > $OUT/${tag}_bench_classic_f16.json
(timeout 300 python bench.py --full --force-dist --collective cabi --scaling strong --no-also --no-cpu-baseline 2>/dev/null | tail -1) > $OUT/${tag}_bench_strong_cabi_world1.json
ROOTD=$PWD
cd /tmp && export TMPDIR=/tmp
(timeout 600 rocprofv3 --kernel-trace --stats --output-format csv -d $ROOTD/$OUT/${tag}_prof -- python3 $ROOTD/bench.py --full --steps 3 --warmup 1 --no-cpu-baseline --no-also --no-parity 2>&1 | tail -5) > $ROOTD/$OUT/${tag}_prof.log 2>&1
(timeout 600 rocprofv3 --kernel-trace --stats --output-format csv -d $ROOTD/$OUT/${tag}_prof_classic -- python3 $ROOTD/bench.py --full --workload classic --steps 3 --warmup 1 --no-cpu-baseline --no-also --no-parity 2>&1 | tail -5) > $ROOTD/$OUT/${tag}_prof_classic.log 2>&1
(timeout 600 rocprofv3 --kernel-trace --stats --output-format csv -d $ROOTD/$OUT/${tag}_prof_train -- python3 $ROOTD/tools/scratch/train_prof.py 16384 f16 binned --fast-only 2>&1 | tail -8) > $ROOTD/$OUT/${tag}_prof_train.log 2>&1
cd $ROOTD
for d in prof prof_classic prof_train; do f=$(ls $OUT/${tag}_$d/*/*_kernel_stats.csv 2>/dev/null | head -1); [ -n "$f" ] && cp $f $OUT/${tag}_${d}_kernel_stats.csv; rm -rf $OUT/${tag}_$d; done
tail -4 $OUT/${tag}_tests.log
