#!/usr/bin/env bash
# The end-of-change run on the GPU box: whole -m gpu suite, the --full bench line, kernel statistics of the one-stream step
# under rocprofv3, smoke().  usage: bash tools/gpu_round_check.sh <output dir>; results under <output dir>/
[ $# -ge 1 ] || { echo "usage: gpu_round_check.sh <output dir>" >&2; exit 2; }
O=$(mkdir -p "$1" && cd "$1" && pwd) || exit 1
R=$PWD
python -m pytest tests -m gpu -x -q 2>&1 | tail -3 > $O/gputest.txt
python bench.py --full --steps 20 --warmup 5 > $O/bench.json 2> $O/bench.err
( cd /tmp && export TMPDIR=/tmp && rocprofv3 --kernel-trace --stats --output-format csv -d $O/prof_bench -o b -- python $R/bench.py --steps 10 --warmup 2 --two-streams 0 > $O/prof_bench.log 2>&1 )
python -c "import __graft_entry__ as g; g.smoke()" > $O/smoke.txt 2>&1
cat $O/gputest.txt; tail -2 $O/smoke.txt; O=$O python - <<'PY'
import json, os
d=json.loads(open(os.path.join(os.environ["O"], "bench.json")).read().strip().splitlines()[-1])
print(d["value"], d["ms_per_step"], d["roofline"]["achieved"], d["roofline"]["frac"], d["roofline"]["back_to_back"], d["config"]["extras"]["one_stream"], d["config"]["extras"]["hip_graph"]["images_per_s"])
PY
head -12 $O/prof_bench/b_kernel_stats.csv | cut -c1-150
