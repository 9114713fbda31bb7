#!/usr/bin/env python3
"""Time of filling a handle with fresh instances: on the device (BatchedTaskEnv.generate_instances) against the host path
(load_instances(**generate_batch(...)): one numpy Generator per env, then four host-to-device copies).

    python tools/instgen_time.py [--reps 10] [--warmup 2]

Each figure is the median of `reps` calls after `warmup`, host clock around work that ends in a synchronise of the stream.  The
instances of both paths are compared (array_equal) before anything is timed.  Prints one JSON line per shape and exits with status 1
when the device path is not faster than the host path at every shape; needs a HIP device."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from dcmrta_amd.batched_env import BatchedTaskEnv  # noqa: E402
from dcmrta_amd.instances import generate_batch, generate_batch_ranges  # noqa: E402

# name, B, agents_range, tasks_range
SHAPES = [("4096x20A50T", 4096, 20, 50), ("8192x50A200T", 8192, 50, 200), ("ragged4096x(10-20)A(20-50)T", 4096, (10, 20), (20, 50))]


def median_s(fn, reps, warmup, device):
    out = []
    for i in range(warmup + reps):
        torch.cuda.synchronize(device)
        t = time.perf_counter()
        fn()
        torch.cuda.synchronize(device)
        if i >= warmup:
            out.append(time.perf_counter() - t)
    return statistics.median(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--device", default="cuda:0")
    args = ap.parse_args()
    if args.reps < 1:
        ap.error("--reps must be >= 1")
    slower = []
    for name, B, ar, tr in SHAPES:
        ragged = isinstance(ar, tuple)
        A, T = (ar[1], tr[1]) if ragged else (ar, tr)
        env, twin = BatchedTaskEnv(B, A, T, device=args.device), BatchedTaskEnv(B, A, T, device=args.device)
        host = (lambda: generate_batch_ranges(range(B), ar, tr)) if ragged else (lambda: generate_batch(B, A, T))
        want, got = host(), env.generate_instances(0, ar, tr).instances()
        for k, v in want.items():
            assert np.array_equal(got[k].cpu().numpy(), v), (name, k)
        dev_s = median_s(lambda: env.generate_instances(0, ar, tr), args.reps, args.warmup, args.device)
        host_s = median_s(lambda: twin.load_instances(**host()), args.reps, args.warmup, args.device)
        print(json.dumps(dict(shape=name, device_ms=round(dev_s * 1e3, 4), host_ms=round(host_s * 1e3, 3),
                              speedup=round(host_s / dev_s, 1), reps=args.reps)), flush=True)
        if dev_s >= host_s:
            slower.append(name)
    if slower:
        sys.exit("device path not faster than the host path at: " + ", ".join(slower))


if __name__ == "__main__":
    main()
