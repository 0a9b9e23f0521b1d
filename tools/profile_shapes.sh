# rocprofv3 kernel stats of the two side configurations (batch 1, and batch 16 x 500-phoneme chunks)
set -e
R=$GRAFT_REPO_ROOT
OUT=${OUT:-$R/profile_out}  # results directory (made absolute: the rocprofv3 passes run from /tmp)
mkdir -p $OUT && OUT=$(cd $OUT && pwd)
cd /tmp && export TMPDIR=/tmp
rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/prof_b1 -- python3 $R/bench.py --full --steps 10 --warmup 2 --batch 1 --cpu-utts 0 --free-run 0 --pcie 0 --serve 0 --reduced 0 > $OUT/prof_b1_bench.json 2> $OUT/prof_b1.log
rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/prof_long -- python3 $R/bench.py --full --steps 3 --warmup 1 --batch 16 --phonemes 500 --cpu-utts 0 --free-run 0 --pcie 0 --serve 0 --reduced 0 > $OUT/prof_long_bench.json 2> $OUT/prof_long.log
cd $R
python tools/summarize_rocprof.py $OUT/prof_b1 $OUT/prof_b1_bench.json $OUT/kernel_stats_b1.txt
python tools/summarize_rocprof.py $OUT/prof_long $OUT/prof_long_bench.json $OUT/kernel_stats_long.txt
head -12 $OUT/kernel_stats_b1.txt | cut -c1-140
head -12 $OUT/kernel_stats_long.txt | cut -c1-140
