#!/usr/bin/env python3
"""What the rollout log of the persistent launches costs: BatchedTaskEnv.rollout(policy, episodes=3) with enable_rollout_log off
against on, for "random", "first" and "nearest", at 4096 x 20A/50T (the register-resident forms: k_rollout_fast / k_hp_rollout_fast
against k_lg_rollout_fast) and at 8192 x 50A/200T (k_rollout_fast_mc / k_hp_rollout_random against the general logging form
k_lg_rollout_random).

    python tools/rollout_log_time.py [--reps 10] [--warmup 2] [--cap 64]

Each call starts from generate_instances + reset (outside the timed region), so every timed call plays the same episodes; a figure is
the median of `reps` calls after `warmup`, host clock around one call that ends in a synchronise of the stream.  The on/off ratio mixes
effects: with the log on "random" at 4096 envs also loses the wave-priority instantiation of k_rollout_fast (the logging forms have
none), and at 50A/200T it leaves the multi-chunk register-resident kernel for the general one; only the greedy policies compare a kernel
with its own logging twin.  Prints one JSON line per shape, policy and mode, the "on" line with the on/off ratio; checks that the log
changed no step count; sets no threshold; needs a HIP device."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from dcmrta_amd.batched_env import BatchedTaskEnv  # noqa: E402
from dcmrta_amd.choice import env_seeds  # noqa: E402

SHAPES = ((4096, 20, 50), (8192, 50, 200))
EPISODES = 3


def timed_rollouts(env, seeds, policy, reps, warmup):
    """(median seconds, decisions of one call) of rollout(policy, EPISODES) from a fresh generate_instances + reset."""
    out, steps = [], 0
    for i in range(warmup + reps):
        env.generate_instances(0)
        env.reset(seeds, observe=False)
        torch.cuda.synchronize(env.device)
        t = time.perf_counter()
        s = env.rollout(policy, episodes=EPISODES)
        torch.cuda.synchronize(env.device)
        if i >= warmup:
            out.append(time.perf_counter() - t)
        steps = int(s.sum())
    return statistics.median(out), steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--cap", type=int, default=64)
    ap.add_argument("--device", default="cuda:0")
    args = ap.parse_args()
    if args.reps < 1 or args.cap < 1:
        ap.error("--reps and --cap must be >= 1")
    for B, A, T in SHAPES:
        env = BatchedTaskEnv(B, A, T, device=args.device)
        seeds = env_seeds(1, 0, B)
        for policy in ("random", "first", "nearest"):
            off = None
            for mode in ("off", "on"):
                env.enable_rollout_log(args.cap if mode == "on" else 0)
                sec, steps = timed_rollouts(env, seeds, policy, args.reps, args.warmup)
                row = dict(shape=f"{B}x{A}A{T}T", policy=policy, log=mode, episodes=EPISODES, ms=round(sec * 1e3, 4), decisions=steps,
                           ns_per_decision=round(sec * 1e9 / steps, 4), reps=args.reps)
                if mode == "off":
                    off = (sec, steps)
                else:
                    assert steps == off[1], (policy, steps, off[1])
                    ln = env.rollout_routes()[2]
                    row.update(on_over_off=round(sec / off[0], 4), cap=args.cap, longest_route=int(ln.max()))
                print(json.dumps(row), flush=True)
        env.close()


if __name__ == "__main__":
    main()
