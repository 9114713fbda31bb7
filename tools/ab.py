#!/usr/bin/env python3
"""A/B already-built libraries against bench.py on the GPU box (developer tool): interleaved rounds, one 4096-env launch per pass.

    python tools/ab.py name1=path1.so name2=path2.so ...   [env AB_ARGS="--agents 15 --tasks 35" AB_ROUNDS=5]

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
        o = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "20", "--warmup", "3", "--no-cpu-baseline",
                            "--no-lockstep-probe", "--streams", "1"] + os.environ.get("AB_ARGS", "").split(),
                           env=dict(os.environ, DCMRTA_HIP_LIB=os.path.abspath(so)), capture_output=True, text=True, timeout=600)
        line = [l for l in o.stdout.splitlines() if l.startswith("{")]
        if o.returncode != 0 or not line:
            print(name, "FAILED, exit status", o.returncode, o.stderr[-400:])
            failed = True
            break
        res[name].append(json.loads(line[-1])["roofline"]["avg_launch_ms"])
    if failed:
        break
for name, v in res.items():
    print(f"{name:16s} launch ms: " + " ".join(f"{x:.4f}" for x in v) + (f"   mean {sum(v) / len(v):.4f}" if v else ""))
sys.exit(1 if failed else 0)
