#!/bin/bash
# Round-end check on the GPU box: GPU tests, smoke(), bench.py --full, the rocprofv3 passes, config 5.
#   bash tools/gpu_round_check.sh r01g   -> $KW_OUT_DIR/<tag>_* (default bench_out/)
set -o pipefail
TAG=${1:-r01g}
cd "${GRAFT_REPO_ROOT:-/root/repo}"
export KW_OUT_DIR=${KW_OUT_DIR:-bench_out}
OUT=$KW_OUT_DIR
mkdir -p "$OUT"
export TMPDIR=/tmp
timeout -k 10 500 python -u -m pytest tests -m gpu -x -v -s --timeout 120 --timeout-method thread > "$OUT"/${TAG}_pytest_gpu.log 2>&1 && echo TESTS_OK &&
timeout -k 10 240 python -c "import __graft_entry__ as g; g.smoke()" > "$OUT"/${TAG}_smoke.log 2>&1 && echo SMOKE_OK &&
timeout -k 10 600 python bench.py --full > "$OUT"/${TAG}_bench.json 2> "$OUT"/${TAG}_bench.err && cat "$OUT"/${TAG}_bench.json &&
bash tools/profile.sh ${TAG} &&
timeout -k 10 200 python tools/bench_configs.py --config 5 --clips 64 > "$OUT"/${TAG}_config5.json 2> "$OUT"/${TAG}_config5.err && cat "$OUT"/${TAG}_config5.json
