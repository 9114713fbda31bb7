#!/usr/bin/env python3
"""A/B already-built libraries against the PRODUCT line of bench.py on the GPU box (developer tool): interleaved rounds of
`bench.py --steps 20 --warmup 5` with its calibrated sub-batch streams (tools/ab.py times one launch on one stream instead).

    python tools/ab_bench.py name1=path1.so name2=path2.so ...   [env AB_ARGS="--config 4" AB_ROUNDS=5]

The same library under two names measures the old-vs-old spread.  A run that fails ends the comparison: nothing more is started
on the GPU after it, and the exit status is 1."""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
libs = [a.split("=", 1) for a in sys.argv[1:]]
res = {n: [] for n, _ in libs}
failed = False
for rnd in range(int(os.environ.get("AB_ROUNDS", "3"))):
    for name, so in libs:
        o = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "20", "--warmup", "5", "--no-cpu-baseline",
                            "--no-lockstep-probe", "--no-other-configs"] + os.environ.get("AB_ARGS", "").split(),
                           env=dict(os.environ, DCMRTA_HIP_LIB=os.path.abspath(so)), capture_output=True, text=True, timeout=900)
        line = [l for l in o.stdout.splitlines() if l.startswith("{")]
        if o.returncode != 0 or not line:
            print(name, "FAILED, exit status", o.returncode, o.stderr[-300:])
            failed = True
            break
        d = json.loads(line[-1])
        res[name].append((d["value"], d["config"].get("streams_per_gpu")))
    if failed:
        break
for name, v in res.items():
    print(f"{name:12s} " + " ".join(f"{x[0] / 1e9:.4f}" for x in v) + "  e9 steps/s, streams " + str(sorted({x[1] for x in v})))
print("GPU_MAX_HW_QUEUES of the runs:", os.environ.get("GPU_MAX_HW_QUEUES", "unset (bench.py's default: 8)"))
sys.exit(1 if failed else 0)
