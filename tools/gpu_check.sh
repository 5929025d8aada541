#!/bin/bash
# One-call GPU check of a kernel family after an edit (run through gpurun): its parity tests, a fuzz slice, its micro-benchmark.
#   tools/gpu_check.sh orb|sgbm|ba|match [fuzz seconds] [fuzz seed]
cd "$GRAFT_REPO_ROOT"
FAM=${1:-orb}; SECS=${2:-60}; SEED=${3:-1}
K=""; F2=""   # K: which tests of tests/test_gpu_ties.py (tie-dense ORB / ANMS / matcher tests; the periodic SGBM ones have "sgbm" in their names); F2: its fuzz kind
case $FAM in
  orb)   T="tests/test_gpu_orb.py tests/test_gpu_edge_cases.py tests/test_gpu_pipeline.py"; F=orb;   B="tools/bench_orb.py --batch 256 --reps 10"; K="not sgbm"; F2=orb_ties;;
  sgbm)  T="tests/test_gpu_sgbm.py";                                                        F=sgbm;  B="tools/bench_sgbm.py --batch 32 --reps 4";  K="sgbm";     F2=sgbm_periodic;;
  ba)    T="tests/test_gpu_lm.py tests/test_gpu_pipeline.py";                                F=ba;    B="tools/bench_ba.py --windows 256 --reps 8";;
  match) T="tests/test_gpu_match.py";                                                        F=match; B="tools/bench_match.py";;
esac
( timeout 900 python -m pytest $T -q -m gpu ) 2>&1 | tail -2
[ -n "$K" ] && ( timeout 900 python -m pytest tests/test_gpu_ties.py -q -m gpu -k "$K" ) 2>&1 | tail -2
( timeout $((SECS + 120)) python tests/fuzz_parity.py --seconds $SECS --seed $SEED --only $F ) 2>&1 | tail -1
[ -n "$F2" ] && ( timeout $((SECS / 2 + 120)) python tests/fuzz_parity.py --seconds $((SECS / 2)) --seed $SEED --only $F2 ) 2>&1 | tail -1
( timeout 300 python $B ) 2>&1 | grep -v amdgpu.ids | tail -2
