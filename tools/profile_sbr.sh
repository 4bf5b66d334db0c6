#!/bin/bash
# C3 / C4 evidence for profiles/: bench JSONs and rocprofv3 kernel stats of the same commands.
cd /tmp && export TMPDIR=/tmp
R=$GRAFT_REPO_ROOT
O=${OUT_DIR:-$R/out}
mkdir -p $O
for w in c3 c4; do
  python $R/bench.py --workload $w --full > $O/bench_$w.json 2> $O/bench_$w.err
  timeout 300 rocprofv3 --kernel-trace --stats -d /tmp/ks_$w -o r -- python $R/bench.py --workload $w --steps 60 --warmup 6 --no-cpu-baseline > /dev/null 2>&1
  python $R/tools/rocprof_summary.py stats $(find /tmp/ks_$w -name "*.db") > $O/${w}_kernel_stats.txt
  head -8 $O/${w}_kernel_stats.txt
  python -c "import json; d=json.load(open('$O/bench_$w.json')); print(d['value'], d['ms_per_step'], d['roofline']['frac'], d['cpu_baseline']['value'])"
done
