# Refreshes the committed evidence of a round on the GPU box: PMC traffic, rocprofv3 kernel statistics of the bench command,
# the bench line itself.  Usage, from the repository root on the GPU box: bash tools/refresh_profiles.sh r05 OUT
# (OUT: the directory the kernel statistics and the bench lines of this refresh are written to)
R=${1:-r04}
OUT=${2:?usage: bash tools/refresh_profiles.sh ROUND OUT}
cd /tmp && export TMPDIR=/tmp && cd $GRAFT_REPO_ROOT
mkdir -p gpurun_out/refresh
bash tools/collect_traffic.sh > gpurun_out/refresh/collect.log 2>&1 || true
cp gpurun_out/pmc_traffic.json gpurun_out/refresh/${R}_pmc_traffic.json 2>/dev/null || true
cp gpurun_out/pmc_traffic.json profiles/${R}_pmc_traffic.json 2>/dev/null || true
echo "traffic done"
mkdir -p "$OUT"
rm -rf "$OUT/profAll"
timeout -k 10 600 rocprofv3 --kernel-trace --stats --output-format csv -d "$OUT/profAll" -- python3 bench.py --full --no-cpu-baseline > "$OUT/bench_all_prof.json" 2> "$OUT/bench_all_prof.err"
python tools/prof_summary.py "$OUT/profAll" 40 > "$OUT/${R}_bench_all_kernel_stats.txt"
cp "$OUT"/profAll/*/*kernel_stats.csv "$OUT/${R}_bench_all_kernel_stats.csv"
rm -rf "$OUT/profAll"
# graph D, the primary line, twice: SINGLE stream (full-batch launches, one after the other: avg us x launches of a family reproduces the
# line's depthwise_frac / pointwise_frac by hand) and the TWO-stream form the timed step runs (half batches overlapped); graphs X and T once
for cfg in "D_single:--workload D --steps 10 --warmup 2 --profile-clean --profile-streams single" \
           "D_two:--workload D --steps 10 --warmup 2 --profile-clean --profile-streams two" \
           "X:--workload X --steps 3 --warmup 1 --profile-clean --no-cpu-baseline" \
           "T:--workload T --steps 3 --warmup 1 --profile-clean --no-cpu-baseline --no-graph"; do
  tag=${cfg%%:*}; args=${cfg#*:}
  rm -rf "$OUT/prof_$tag"
  timeout -k 10 400 rocprofv3 --kernel-trace --stats --output-format csv -d "$OUT/prof_$tag" -- python3 bench.py $args > "$OUT/bench${tag}_prof.json" 2> "$OUT/bench${tag}_prof.err"
  if [ "${tag#D_}" != "$tag" ]; then name=${R}_benchD_kernel_stats_${tag#D_}; else name=${R}_bench${tag}_kernel_stats; fi
  python tools/prof_summary.py "$OUT/prof_$tag" 40 > "$OUT/$name.txt"
  cp "$OUT/prof_$tag"/*/*kernel_stats.csv "$OUT/$name.csv"
  rm -rf "$OUT/prof_$tag"
done
echo "profiles done"
timeout -k 10 900 python bench.py --full > "$OUT/${R}_bench_all.json" 2> "$OUT/bench_all.err"; echo "bench rc=$?"
grep "\[bench\]" "$OUT/bench_all.err" | tail -3
tail -c 400 "$OUT/${R}_bench_all.json"
