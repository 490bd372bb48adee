# rocprof A/B of the single-MSM form (PLK_MSM_HALF=0/1) inside the full bench
# (output directory: $OUT, default bench_out)
set -e
export TMPDIR=/tmp
O=${OUT:-bench_out}/hp
mkdir -p $O
for h in 0 1 0 1; do
PLK_MSM_HALF=$h timeout -k 10 300 rocprofv3 --kernel-trace --stats -d $O/t -o run -- python3 bench.py --full --steps 20 --no-cpu-baseline > /dev/null 2>&1
python3 tools/kstats.py $O/t/run_results.db | grep "msm_dlog" | sed "s/^/half=$h /"
rm -rf $O/t
done
