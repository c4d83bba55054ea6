#!/bin/bash
# On the GPU box: which runtime calls (memsets, copies, launches) one eager static-shape sharded step makes at one rank --
# a HIP API + kernel + memory-copy trace of scripts/shard_static_prof.py (one program, no counters), summarised per call name
# (and per memset / copy size).  The summary runs only if the traced program succeeded.
set -euo pipefail
R=$(cd "$(dirname "$0")/.." && pwd)
cd /tmp && export TMPDIR=/tmp
T=$(mktemp -d /tmp/sht.XXXXXX)
N=${N:-100} AHEAD=${AHEAD:-2} timeout -k 10 600 rocprofv3 --hip-trace --kernel-trace --memory-copy-trace --output-format csv -d $T -- python3 $R/scripts/shard_static_prof.py > $T.log 2>&1 \
  || { rc=$?; echo "the traced program FAILED: status $rc; no summary"; tail -30 $T.log; exit $rc; }
if grep -q "an illegal memory access was encountered" $T.log; then echo "the traced program reported a GPU fault; no summary"; tail -30 $T.log; exit 1; fi
tail -1 $T.log
python3 - $T <<'PY'
import csv, glob, collections, sys
steps = 100 + 8
for f in glob.glob(sys.argv[1] + '/**/*hip_api_trace.csv', recursive=True):
    c = collections.Counter(r['Function'] for r in csv.DictReader(open(f)))
    print('HIP API calls per step:')
    for k, v in c.most_common(25):
        print('  %-40s %7.2f' % (k, v / steps))
for f in glob.glob(sys.argv[1] + '/**/*memory_copy_trace.csv', recursive=True):
    rows = list(csv.DictReader(open(f)))
    c = collections.Counter((r.get('Direction', '?'), ) for r in rows)
    print('memory copies per step:', {k: round(v / steps, 2) for k, v in c.items()})
    print(rows[len(rows) // 2] if rows else None)
PY
python3 - $T <<'PY'
import csv, glob, sys
for f in glob.glob(sys.argv[1] + '/**/*hip_api_trace.csv', recursive=True):
    rows = list(csv.DictReader(open(f)))
    print(list(rows[0].keys()))
    rows.sort(key=lambda r: int(r['Start_Timestamp']))
    skip = ('hipGetDevice', 'hipGetLastError', '__hipPushCallConfiguration', '__hipPopCallConfiguration', 'hipSetDevice', 'hipThreadExchangeStreamCaptureMode', 'hipDevicePrimaryCtxGetState', 'hipStreamIsCapturing')
    seq = [(r['Function'], r.get('Thread_Id', '?')) for r in rows if r['Function'] not in skip and not r['Function'].startswith('__hipRegister')]
    mid = len(seq) * 2 // 3
    tids = sorted(set(t for _, t in seq))
    for fn, t in seq[mid:mid + 90]:
        print('  T%d %s' % (tids.index(t), fn))
PY
