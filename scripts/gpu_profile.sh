#!/bin/bash
# rocprofv3 evidence for the bench's dominant kernels: kernel trace + stats, then HBM counters in separate passes
#   scripts/gpu_profile.sh DIR && python scripts/summarize_profiles.py rNN DIR
P=${1:?usage: scripts/gpu_profile.sh OUTPUT_DIR}
mkdir -p $P && P=$(cd $P && pwd)
export HSA_ENABLE_IPC_MODE_LEGACY=0
REPO=$PWD
cd /tmp && export TMPDIR=/tmp
for layout in contiguous default; do
  rocprofv3 --kernel-trace --stats --output-format csv -d $P/${layout}_trace -o bench -- \
     python $REPO/bench.py --full --steps 5 --warmup 3 --cpu-sample 0 --no-extras --layout $layout > $P/${layout}_trace.log 2>&1
  rocprofv3 --kernel-trace --pmc FETCH_SIZE --output-format csv -d $P/${layout}_fetch -o bench -- \
     python $REPO/bench.py --full --steps 2 --warmup 1 --cpu-sample 0 --no-extras --layout $layout > $P/${layout}_fetch.log 2>&1
  rocprofv3 --kernel-trace --pmc WRITE_SIZE --output-format csv -d $P/${layout}_write -o bench -- \
     python $REPO/bench.py --full --steps 2 --warmup 1 --cpu-sample 0 --no-extras --layout $layout > $P/${layout}_write.log 2>&1
done
cd $REPO
find $P -type f | head -50
for f in $(find $P -name "*kernel_stats.csv"); do echo "== $f"; head -8 $f; done
# drop the big per-dispatch traces, keep per-kernel summaries of the counter passes
python - "$P" <<'PY'
import csv, glob, collections, sys
P = sys.argv[1]
for f in glob.glob(P + "/*_fetch/**/*counter_collection.csv", recursive=True) + glob.glob(P + "/*_write/**/*counter_collection.csv", recursive=True):
    agg = collections.defaultdict(lambda: [0, 0.0])
    for row in csv.DictReader(open(f)):
        k = (row.get("Kernel_Name"), row.get("Counter_Name"))
        agg[k][0] += 1
        agg[k][1] += float(row.get("Counter_Value", 0))
    out = f.replace("counter_collection.csv", "counter_summary.csv")
    with open(out, "w") as o:
        o.write("kernel,counter,dispatches,sum,mean_per_dispatch\n")
        for (k, c), (n, s) in sorted(agg.items(), key=lambda kv: -kv[1][1]):
            o.write('"%s",%s,%d,%.1f,%.1f\n' % (k, c, n, s, s / n))
    print("==", out)
    print(open(out).read()[:1500])
PY
find $P -name "*kernel_trace.csv" -size +2M -delete
find $P -name "*counter_collection.csv" -size +2M -delete
