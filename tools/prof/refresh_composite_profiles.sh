# usage: refresh_composite_profiles.sh <out_dir> : the reference-topology profiles, the GPU tier and the --full bench line into <out_dir>
OUT=${1:?usage: refresh_composite_profiles.sh <out_dir>}
mkdir -p "$OUT"
bash tools/prof/comp_profile.sh "$OUT" 64 > /dev/null 2>&1
OMP_NUM_THREADS=4 python tools/prof/gpu_comp_prof.py 16 20 4 300 24 8 solve > "$OUT/composite_workload_24amb.txt" 2>&1
OMP_NUM_THREADS=4 python tools/prof/gpu_comp_prof.py 16 20 4 300 40 8 solve > "$OUT/composite_workload_40amb.txt" 2>&1
bash tools/prof/comp_timeline.sh 10 > "$OUT/composite_single_timeline.txt" 2>&1
(timeout 1200 python -m pytest tests -m gpu -x -q 2>&1 | tail -6) > "$OUT/gputest.log"
timeout 600 python bench.py --full > "$OUT/bench_default.json" 2> /dev/null
