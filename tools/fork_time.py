#!/usr/bin/env python3
"""What fanning B envs out to B x K branches costs: dcm_fork_envs against the way without it.

    fork          dcm_fork_envs into a handle of B x K envs, branch i <- env i // K (the map Lookahead.values() uses), no new seeds
    blob          the same fan-out through the snapshot calls: clone_state() of the B envs, a row gather of each of the blob's four
                  sections to B x K rows (torch.index_select + cat), restore_state() into the B x K handle -- two extra full copies

    python tools/fork_time.py [--envs 4096] [--fan 51] [--agents 20] [--tasks 50] [--reps 20] [--warmup 3]

Both are timed with device events around one fan-out, a figure is the median of `reps` runs after `warmup`, and the rate counts what a
fan-out has to move at the least: every branch's record, summary row, abandonment log and count row read once and written once,
2 x B x K x (rec_bytes + 64 + 32 A + align16(2 A T)) bytes.  The two ways are checked to leave the same bytes.  Prints one JSON line;
sets no threshold; needs a HIP device."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from dcmrta_amd.batched_env import BatchedTaskEnv  # noqa: E402
from dcmrta_amd.choice import env_seeds  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--fan", type=int, default=51, help="branches per env (T + 1 for a lookahead)")
    ap.add_argument("--agents", type=int, default=20)
    ap.add_argument("--tasks", type=int, default=50)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--device", default="cuda:0")
    args = ap.parse_args()
    if min(args.envs, args.fan, args.reps) < 1:
        ap.error("--envs, --fan and --reps must be >= 1")
    B, K, A, T = args.envs, args.fan, args.agents, args.tasks
    src = BatchedTaskEnv(B, A, T, device=args.device)
    src.generate_instances(0)
    src.reset(env_seeds(1, 0, B), observe=False)
    src.rollout("random", write_obs=False, max_decisions=20)                    # somewhere in mid-episode
    dst = BatchedTaskEnv(B * K, A, T, device=args.device)
    dst.generate_instances(0)
    dst.reset(0, observe=False)
    dev = src.device
    index = (torch.arange(B * K, dtype=torch.int64, device=dev) // K)
    index32 = index.to(torch.int32)
    rec, pitch = src.record_bytes(), (2 * A * T + 15) // 16 * 16
    row_bytes = [rec, 64, 32 * A, pitch]                                        # the blob's sections, per env
    moved = 2 * B * K * sum(row_bytes)

    def fork():
        dst.fork_from(src, index32)

    def blob():
        parts, at = [], 0
        snap = src.clone_state()
        for w in row_bytes:
            parts.append(snap[at:at + B * w].view(B, w).index_select(0, index).reshape(-1))
            at += B * w
        dst.restore_state(torch.cat(parts))

    def median_ms(call):
        ms = []
        for i in range(args.warmup + args.reps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            call()
            b.record()
            torch.cuda.synchronize(dev)
            if i >= args.warmup:
                ms.append(a.elapsed_time(b))
        return statistics.median(ms)

    blob()
    want = dst.clone_state()
    dst.reset(0, observe=False)
    fork()
    assert torch.equal(dst.clone_state(), want), "the two fan-outs leave different bytes"
    del want
    fork_ms, blob_ms = median_ms(fork), median_ms(blob)
    print(json.dumps(dict(shape=f"{B}x{A}A{T}T -> {B * K}", bytes_per_env=sum(row_bytes), moved_bytes=moved, reps=args.reps,
                          fork_ms=round(fork_ms, 4), fork_GBps=round(moved / fork_ms / 1e6, 1),
                          blob_ms=round(blob_ms, 4), blob_GBps=round(moved / blob_ms / 1e6, 1))), flush=True)
    src.close()
    dst.close()


if __name__ == "__main__":
    main()
