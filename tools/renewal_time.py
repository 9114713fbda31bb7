#!/usr/bin/env python3
"""What instance renewal costs the persistent rollout: rollout_random(episodes=3) at 4096 x 20A/50T and rollout_random(episodes=2) at
8192 x 50A/200T, with renewal off (every episode on the instance the record holds) and on (a fresh instance at every restart,
BatchedTaskEnv.set_instance_renewal(B)).  Then size renewal at the reference's own ranges: 4096 envs, agents (10, 20) x tasks (20, 50) on a
renew_sizes=True handle, rollout_random(episodes=3), renewal off (a ragged batch replaying its instances: the kernels an unflagged
handle runs) against on (new sizes with every new instance).

    python tools/renewal_time.py [--reps 10] [--warmup 2]

Each call starts from generate_instances + reset (outside the timed region), so every timed call plays the same episodes; a figure is
the median of `reps` calls after `warmup`, host clock around one call that ends in a synchronise of the stream.  A renewal is one
seeding of the generator plus ceil((2 + A + 2 T) / 64) + ceil(T / 128) jump-ahead steps per episode; the episodes played differ between
the two modes (other instances from the second episode on), so the ratio is reported together with the decisions each mode took.
Prints one JSON line per shape, the ragged one with its time per decision in both modes; sets no threshold; needs a HIP device."""
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

# name, B, A, T, episodes
SHAPES = [("4096x20A50T", 4096, 20, 50, 3), ("8192x50A200T", 8192, 50, 200, 2)]
# name, B, agents range, tasks range, episodes: size renewal (parameters.py:15-16)
RAGGED = [("4096x(10,20)Ax(20,50)T", 4096, (10, 20), (20, 50), 3)]


def timed_rollouts(env, seeds, stride, episodes, reps, warmup, agents_range=None, tasks_range=None):
    """(median seconds, decisions of one call) of rollout_random(episodes) from a fresh generate_instances + reset."""
    out, steps = [], 0
    for i in range(warmup + reps):
        env.generate_instances(0, agents_range=agents_range, tasks_range=tasks_range)
        env.set_instance_renewal(stride)
        env.reset(seeds, observe=False)
        torch.cuda.synchronize(env.device)
        t = time.perf_counter()
        s = env.rollout_random(episodes=episodes)
        torch.cuda.synchronize(env.device)
        if i >= warmup:
            out.append(time.perf_counter() - t)
        steps = int(s.sum())
    return statistics.median(out), steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--device", default="cuda:0")
    args = ap.parse_args()
    if args.reps < 1:
        ap.error("--reps must be >= 1")
    for name, B, A, T, episodes in SHAPES:
        env = BatchedTaskEnv(B, A, T, device=args.device)
        seeds = env_seeds(1, 0, B)
        off_s, off_steps = timed_rollouts(env, seeds, 0, episodes, args.reps, args.warmup)
        on_s, on_steps = timed_rollouts(env, seeds, B, episodes, args.reps, args.warmup)
        assert int(env.instance_index().min()) == episodes - 1 == int(env.instance_index().max())
        print(json.dumps(dict(shape=name, episodes=episodes, off_ms=round(off_s * 1e3, 4), on_ms=round(on_s * 1e3, 4),
                              ratio=round(on_s / off_s, 4), off_decisions=off_steps, on_decisions=on_steps,
                              ratio_per_decision=round((on_s / on_steps) / (off_s / off_steps), 4), reps=args.reps)), flush=True)
    for name, B, ar, tr, episodes in RAGGED:
        env = BatchedTaskEnv(B, ar[1], tr[1], device=args.device, renew_sizes=True)
        seeds = env_seeds(1, 0, B)
        off_s, off_steps = timed_rollouts(env, seeds, 0, episodes, args.reps, args.warmup, ar, tr)
        on_s, on_steps = timed_rollouts(env, seeds, B, episodes, args.reps, args.warmup, ar, tr)
        assert int(env.instance_index().min()) == episodes - 1 == int(env.instance_index().max())
        print(json.dumps(dict(shape=name, episodes=episodes, off_ms=round(off_s * 1e3, 4), on_ms=round(on_s * 1e3, 4),
                              ratio=round(on_s / off_s, 4), off_decisions=off_steps, on_decisions=on_steps,
                              off_ns_per_decision=round(off_s * 1e9 / off_steps, 4), on_ns_per_decision=round(on_s * 1e9 / on_steps, 4),
                              ratio_per_decision=round((on_s / on_steps) / (off_s / off_steps), 4), reps=args.reps)), flush=True)


if __name__ == "__main__":
    main()
