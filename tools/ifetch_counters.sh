#!/bin/bash
# tools/ifetch_counters.sh  (run ON THE GPU BOX): instruction-fetch counters of the bench kernels, one rocprofv3 --pmc pass
# per counter set (kernel trace only, as tools/valu_counters.sh), with one lane and with the bench's default two.  Prints
# per-kernel averages per launch and the shares DESIGN.md section 9 quotes: misses / requests of the instruction cache, and
# against wave cycles the fetches in flight (SQ_IFETCH x InstrFetchLatency), the misses at a price, and the issue waits.
# Counter collection serialises the dispatches it instruments, so the two-lane pass shows the same kernels with the other
# lane's host work around them, not two kernels sharing a compute unit: what side-by-side residency costs is in the
# un-instrumented two-lane step time (ab_summary.txt).
ROOT=$(cd "$(dirname "$0")/.." && pwd)
cd /tmp && export TMPDIR=/tmp
(cd "$ROOT" && python -c "import bench; print('sources', bench.kernel_sources_sha256(), ' sela_amd/csrc/* include/*')")
for LANES in 1 2; do
  CMD="python $ROOT/bench.py --steps 6 --warmup 2 --no-cpu-baseline --no-host-legs --no-extra-legs --lanes $LANES"
  N=0
  for SET in "SQC_ICACHE_REQ SQC_ICACHE_HITS SQC_ICACHE_MISSES SQC_ICACHE_MISSES_DUPLICATE" \
             "SQ_IFETCH InstrFetchLatency SQ_WAVE_CYCLES SQ_BUSY_CYCLES" \
             "SQ_WAIT_INST_ANY SQ_WAIT_ANY SQ_ACTIVE_INST_ANY SQ_INSTS_VALU"; do
    N=$((N + 1))
    D=/tmp/if_${LANES}_$N
    rm -rf $D
    timeout -k 10 200 rocprofv3 --pmc $SET --kernel-trace --output-format csv -d $D -o pmc -- $CMD > $D.log 2>&1
    RC=$?
    if [ $RC -ne 0 ]; then
      echo "lanes $LANES: pass '$SET' ended with $RC"; tail -5 $D.log | cut -c1-300
      case $RC in 124|137|134|139) exit $RC ;; esac
    fi
  done
  python - $LANES <<'PY'
import csv, glob, sys, collections
lanes = sys.argv[1]
acc = collections.defaultdict(lambda: collections.defaultdict(list))
for f in glob.glob(f"/tmp/if_{lanes}_*/**/*counter_collection.csv", recursive=True):
    for r in csv.DictReader(open(f)):
        k = r["Kernel_Name"].split("(")[0].replace("void ", "")
        if "sela::" in k:
            acc[k][r["Counter_Name"]].append(float(r["Counter_Value"]))
for k, d in sorted(acc.items()):
    m = {c: sum(v) / len(v) for c, v in d.items()}
    print(f"lanes {lanes}:", k, {c: round(v, 2) if c == "InstrFetchLatency" else round(v) for c, v in m.items()})
    if m.get("SQC_ICACHE_REQ"):
        print(f"lanes {lanes}:   instruction cache: misses / requests = {m.get('SQC_ICACHE_MISSES', float('nan')) / m['SQC_ICACHE_REQ']:.5f}"
              f"  (duplicates of a pending miss / requests = {m.get('SQC_ICACHE_MISSES_DUPLICATE', float('nan')) / m['SQC_ICACHE_REQ']:.5f})")
    if m.get("SQ_WAVE_CYCLES"):
        w = 4 * m["SQ_WAVE_CYCLES"]  # (SQ_WAVE_CYCLES, SQ_WAIT_* count units of four cycles; InstrFetchLatency is in cycles)
        if "SQ_IFETCH" in m and "InstrFetchLatency" in m:
            print(f"lanes {lanes}:   fetches in flight: SQ_IFETCH x InstrFetchLatency / wave cycles = {m['SQ_IFETCH'] * m['InstrFetchLatency'] / w:.4f}"
                  "  (hits included; fetches run ahead of the wave, so this bounds from above what fetch can have held)")
        if "SQC_ICACHE_MISSES" in m:
            print(f"lanes {lanes}:   misses x 1000 cycles / wave cycles = {m['SQC_ICACHE_MISSES'] * 1000 / w:.6f}"
                  "  (every miss priced at a generous 1000 cycles of ONE wave)")
        for c in ("SQ_WAIT_INST_ANY", "SQ_WAIT_ANY"):
            if c in m:
                print(f"lanes {lanes}:   {c} / SQ_WAVE_CYCLES = {m[c] / m['SQ_WAVE_CYCLES']:.4f}")
PY
done
