#!/bin/bash
# Round-6 rocprofv3 evidence (run through gpurun): for each of three bench configurations a kernel trace + stats, FETCH_SIZE and WRITE_SIZE
# passes (separate --pmc runs, no other trace domains) and one SQ pass; summaries under gpurun_out/prof_r06_<cfg>/ (copy the ones to be
# judged into profiles/).  --in-flight 1: kernels of two batches in flight share the chip and have no duration / counters of their own.
# usage: tools/profile_r06.sh [cfg ...]   cfg in: tracks config4 sgbm
set -u
cd /tmp && export TMPDIR=/tmp; cd "$GRAFT_REPO_ROOT"
STEPS=3
COMMON="--full --steps $STEPS --warmup 1 --repeats 1 --in-flight 1 --no-plain-schedule --no-cpu-baseline --no-config4 --no-reference-pipeline --no-config4-step --no-live-dropin --render-workers 0 --unique-frames 128 --inputs resident"
for CFG in ${@:-tracks config4 sgbm}; do
  case $CFG in
    tracks)  ARGS="$COMMON";                                   BATCH=1024;;
    config4) ARGS="$COMMON --ba-windows synthetic --batch 256"; BATCH=256;;
    sgbm)    ARGS="$COMMON --depth sgbm --pose ransac --batch 256"; BATCH=256;;
  esac
  OUT=gpurun_out/prof_r06_$CFG; mkdir -p $OUT
  timeout 500 rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/trace -o bench -- python bench.py $ARGS > $OUT/bench.json 2> $OUT/trace.log
  timeout 500 rocprofv3 --pmc FETCH_SIZE --kernel-trace --output-format csv -d $OUT/pmc_fetch -o bench -- python bench.py $ARGS > /dev/null 2> $OUT/pmc_fetch.log
  timeout 500 rocprofv3 --pmc WRITE_SIZE --kernel-trace --output-format csv -d $OUT/pmc_write -o bench -- python bench.py $ARGS > /dev/null 2> $OUT/pmc_write.log
  python tools/summarize_pmc.py $OUT > $OUT/summary.txt 2>&1
  timeout 500 rocprofv3 --pmc SQ_WAVE_CYCLES SQ_WAIT_ANY SQ_ACTIVE_INST_ANY SQ_ACTIVE_INST_VALU SQ_INSTS_VALU SQ_BUSY_CYCLES SQ_WAVES --kernel-trace --output-format csv \
      -d $OUT/sq -o bench -- python bench.py $ARGS > /dev/null 2> $OUT/sq.log
  python - "$OUT" <<'PY'
import csv, glob, os, sys
from collections import defaultdict
root = sys.argv[1]
f = glob.glob(os.path.join(root, "sq", "*counter_collection.csv"))
acc = defaultdict(lambda: defaultdict(float)); n = defaultdict(int)
if f:
    for r in csv.DictReader(open(f[0])):
        k = r["Kernel_Name"].split("(")[0].replace("void ", "").replace("vslam::", "")
        acc[k][r["Counter_Name"]] += float(r["Counter_Value"])
        if r["Counter_Name"] == "SQ_WAVES": n[k] += 1
lines = []
for k, c in sorted(acc.items(), key=lambda kv: -kv[1].get("SQ_WAVE_CYCLES", 0)):
    if "at::" in k or "rocclr" in k: continue
    wc = c.get("SQ_WAVE_CYCLES", 0) or 1
    lines.append("%-40s disp %4d  wave_cycles %.3e  active_any %5.1f%%  active_valu %5.1f%%  wait_any %5.1f%%  valu_insts %.3e" % (
        k[:40], n[k], wc, 100 * c.get("SQ_ACTIVE_INST_ANY", 0) / wc, 100 * c.get("SQ_ACTIVE_INST_VALU", 0) / wc, 100 * c.get("SQ_WAIT_ANY", 0) / wc, c.get("SQ_INSTS_VALU", 0)))
open(os.path.join(root, "sq_summary.txt"), "w").write("\n".join(lines) + "\n")
PY
  TOTAL_STEPS=$((STEPS * 2 + 1))   # warmup + one timed repeat + the profiled repeat
  case $CFG in
    tracks)  python tools/make_counter_json.py $OUT traffic_tracks.json $BATCH $TOTAL_STEPS "ba_resident_kernel,lm_window_kernel<false,pose_only_wave_kernel" lm_kernels.hip,ba_resident.hip,lm_device.h lm_window_kernel > $OUT/traffic.log 2>&1
             # [r6] the ORB family's counter traffic per step (2 x 1024 images): profiles/traffic_orb.json, reported by bench.py in the family's other_rooflines entry
             python tools/make_counter_json.py $OUT traffic_orb.json $BATCH $TOTAL_STEPS "orb_" orb_kernels.hip "orb_* (family)" >> $OUT/traffic.log 2>&1;;
    config4) python tools/make_counter_json.py $OUT traffic.json $BATCH $TOTAL_STEPS "ba_resident_kernel,lm_window_kernel<false,pose_only_wave_kernel" lm_kernels.hip,ba_resident.hip,lm_device.h lm_window_kernel > $OUT/traffic.log 2>&1;;
    sgbm)    python tools/make_counter_json.py $OUT traffic_sgbm.json $BATCH $TOTAL_STEPS "sgbm_" sgbm_kernels.hip "sgbm_* (family)" > $OUT/traffic.log 2>&1;;
  esac
  cp profiles/traffic*.json $OUT/ 2>/dev/null   # (the JSONs this run just wrote into profiles/ on the box travel back under gpurun_out/)
  cat $OUT/summary.txt | head -40; cat $OUT/sq_summary.txt | head -24; cat $OUT/traffic.log | tail -16
done
# ORB: SQ_INSTS_VALU per image from the tracks run
python - <<'PY'
import hashlib, json, os, re
root = os.environ.get("GRAFT_REPO_ROOT", ".")
p = os.path.join(root, "gpurun_out", "prof_r06_tracks", "sq_summary.txt")
if os.path.exists(p):
    per = {}
    n_img = 2048 * 7   # 2 x 1024 images per step, 7 steps in the profiled command
    for line in open(p):
        name = line.split()[0]
        m = re.search(r"valu_insts ([0-9.e+]+)", line)
        if name.startswith("orb_") and m:
            per[re.sub(r"<.*", "", name)] = float(m.group(1)) / n_img
    sha = hashlib.sha256(open(os.path.join(root, "stereo-visual-slam_amd", "csrc", "orb_kernels.hip"), "rb").read()).hexdigest()[:16]
    out = {"anms": 1500, "valu_wave_insts_per_image": per, "source_sha16": {"orb_kernels.hip": sha},
           "source": "rocprofv3 --pmc SQ_INSTS_VALU (tools/profile_r06.sh, default bench step, 14336 images of 1241x376)"}
    json.dump(out, open(os.path.join(root, "profiles", "orb_valu.json"), "w"), indent=1)
    json.dump(out, open(os.path.join(root, "gpurun_out", "prof_r06_tracks", "orb_valu.json"), "w"), indent=1)
    print(json.dumps(out, indent=1))
PY
