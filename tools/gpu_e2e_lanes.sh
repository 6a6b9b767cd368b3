#!/bin/bash
# e2e with 1..6 lanes on one GPU (tools/e2e_lanes_probe.py)
cd ${GRAFT_REPO_ROOT:-.}
out=${OUT_DIR:-runs}/e2e_lanes
mkdir -p $out
timeout 1500 python tools/e2e_lanes_probe.py > $out/probe.jsonl 2> $out/probe.err
echo "rc=$?"; cut -c1-700 $out/probe.jsonl; tail -5 $out/probe.err | cut -c1-300
timeout 900 python bench.py --full --extras e2e > $out/bench.json 2> $out/bench.err
echo "bench rc=$?"
python3 - $out/bench.json <<'PY'
import json, sys
d = json.loads(open(sys.argv[1]).read().strip().split("\n")[-1])
e = d.get("e2e", {})
print({k: e.get(k) for k in ("wall_s", "lanes", "gpu_busy_s", "gpu_busy_over_wall", "gpu_busy_sum_of_phases_s", "lanes_rows_equal_single_lane", "lane_pipeline_s", "single_lane", "motif_rows", "planted_recovered")})
print(d.get("extra_errors"), d["value"])
PY
