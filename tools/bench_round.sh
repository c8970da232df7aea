#!/bin/bash
# bench_round.sh <tag> <output directory> — the round's bench lines on one box: the driver-style cfg3 line, three short repeats, the secondary
# workloads (cfg2, cfg3 in place, 512x512x1024 in place) and the per-rank slab shapes of cfg4@4, cfg4@8 and cfg5@8 through the
# multi-rank code path on one rank (library RCCL transport, ring to itself).  Every line with --full (copy probe, knob A/Bs, and the
# CPU baseline on the first).  Output: <output directory>/<tag>_bench_*.json(l).
set -uo pipefail
TAG="${1:-r04}"
O="${2:?usage: bench_round.sh <tag> <output directory>}"
ROOT="${GRAFT_REPO_ROOT:-$(cd "$(dirname "${BASH_SOURCE[0]}")/.." && pwd)}"
cd "$ROOT"; mkdir -p "$O"
python bench.py --full > "$O/${TAG}_bench_cfg3.json" 2> "$O/${TAG}_bench_cfg3.err" || { tail -3 "$O/${TAG}_bench_cfg3.err"; exit 1; }
: > "$O/${TAG}_bench_cfg3_repeats.jsonl"
for i in 1 2 3; do python bench.py --full --steps 25 --warmup 5 --no-cpu-baseline 2>/dev/null >> "$O/${TAG}_bench_cfg3_repeats.jsonl"; done
: > "$O/${TAG}_bench_secondary.jsonl"
python bench.py --full --workload cfg2 --steps 100 --warmup 20 --no-cpu-baseline 2>/dev/null >> "$O/${TAG}_bench_secondary.jsonl"
python bench.py --full --in-place --steps 25 --warmup 5 --no-cpu-baseline 2>/dev/null >> "$O/${TAG}_bench_secondary.jsonl"
python bench.py --full --in-place --workload 512x512x1024 --steps 15 --warmup 3 --no-cpu-baseline 2>/dev/null >> "$O/${TAG}_bench_secondary.jsonl"
: > "$O/${TAG}_bench_slab_shapes.jsonl"
python bench.py --full --force-slab --steps 25 --warmup 5 --no-cpu-baseline 2>/dev/null >> "$O/${TAG}_bench_slab_shapes.jsonl"
python bench.py --full --force-slab --workload 512x512x256 --steps 50 --warmup 10 --no-cpu-baseline 2>/dev/null >> "$O/${TAG}_bench_slab_shapes.jsonl"
python bench.py --full --force-slab --workload 512x512x128 --steps 50 --warmup 10 --no-cpu-baseline 2>/dev/null >> "$O/${TAG}_bench_slab_shapes.jsonl"
python bench.py --full --force-slab --workload 1024x1024x128 --steps 25 --warmup 5 --no-cpu-baseline 2>/dev/null >> "$O/${TAG}_bench_slab_shapes.jsonl"
python3 - "$TAG" "$O" <<'PY'
import json, os, sys
tag, out = sys.argv[1], sys.argv[2]
for f in (f"{tag}_bench_cfg3.json", f"{tag}_bench_cfg3_repeats.jsonl", f"{tag}_bench_secondary.jsonl", f"{tag}_bench_slab_shapes.jsonl"):
    for l in open(os.path.join(out, f)):
        if l.strip().startswith("{"):
            d = json.loads(l)
            print(f'{d["value"]:9.1f} MLUPS {d["ms_per_step"]:8.3f} ms  {d["config"]["workload"][:70]:70s} {d["config"]["phases_ms_per_step"]} step_frac {d["config"]["step_roofline_frac"]} bulk_frac {d["roofline"]["frac"]} dev_GB {d["config"]["device_bytes"] / 1e9:.1f}')
PY
