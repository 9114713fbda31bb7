#!/usr/bin/env python3
"""What the device policies of the persistent rollout cost and give: BatchedTaskEnv.rollout(policy, episodes=3) at 4096 x 20A/50T for
"random", "first" and "nearest", each with renewal off (every episode on the instance the record holds) and on (a fresh instance at
every restart, set_instance_renewal(B)).

    python tools/policy_time.py [--reps 10] [--warmup 2]

Each call starts from generate_instances + reset (outside the timed region), so every timed call plays the same episodes; a figure is
the median of `reps` calls after `warmup`, host clock around one call that ends in a synchronise of the stream.  The episodes differ
between policies in length and in their mix of paths (the greedy ones finish tasks, the random one mostly runs into MAX_TIME), so the
time is reported with the decisions taken and per decision; for the greedy policies also the mean number of finished tasks and the
mean makespan of the last episode (summary rows).  "random" runs the wave-priority instantiation of k_rollout_fast at this batch size,
the greedy policies k_hp_rollout_fast, which has none.  Prints one JSON line per policy and mode; sets no threshold; needs a HIP device.

    python tools/policy_time.py --explore [--rounds 5]

times the epsilon-greedy forms (dcm_rollout_explore) against the forms they equal at the two ends, within this build, interleaved,
`rounds` alternations of `reps` calls each: explore_q32 = 0 against rollout("nearest") (k_ex_rollout_fast / k_hp_rollout_fast), and
explore_q32 = 2^32 against the random policy's unprioritised form -- with the rollout log set (k_lg_rollout_fast, 4096 envs) and,
without it, at 4095 envs, where rollout("random") takes k_rollout_fast without wave priorities.  One JSON line per pair.

    python tools/policy_time.py --individual [--events] [--reps 1 --warmup 1]

plays the same calls under individual selection (Worker.run_test_IS): the handle is created with individual_selection=True and
every call is rollout(policy, individual=True) -- k_is_rollout_random / k_isrn_rollout_random for every policy, where a decision is
one agent's step.  --events (with or without --individual) takes the time between two device events around the call instead of the
host clock; every line also gives decisions per second."""
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

B, A, T, EPISODES = 4096, 20, 50, 3


def timed_rollouts(env, seeds, policy, stride, reps, warmup, individual=False, events=False):
    """(median seconds, decisions of one call) of rollout(policy, EPISODES) from a fresh generate_instances + reset."""
    out, steps = [], 0
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for i in range(warmup + reps):
        env.generate_instances(0)
        env.set_instance_renewal(stride)
        env.reset(seeds, observe=False)
        torch.cuda.synchronize(env.device)
        t = time.perf_counter()
        start.record()
        s = env.rollout(policy, episodes=EPISODES, individual=individual)
        stop.record()
        torch.cuda.synchronize(env.device)
        if i >= warmup:
            out.append(start.elapsed_time(stop) * 1e-3 if events else time.perf_counter() - t)
        steps = int(s.sum())
    return statistics.median(out), steps


def explore_pairs(args):
    """The epsilon-greedy forms at explore_q32 = 0 / 2^32 against their twins: the same episodes on both sides of a pair."""
    def one(env, seeds, policy, kw):
        env.generate_instances(0)
        env.reset(seeds, observe=False)
        torch.cuda.synchronize(env.device)
        t = time.perf_counter()
        s = env.rollout(policy, episodes=EPISODES, **kw)
        torch.cuda.synchronize(env.device)
        return time.perf_counter() - t, int(s.sum())

    # (name, envs, rollout log, side a = (policy, keywords), side b)
    pairs = [("eps0_vs_nearest", B, False, ("nearest", {}), ("nearest", dict(explore_q32=0))),
             ("eps0_vs_nearest_logged", B, True, ("nearest", {}), ("nearest", dict(explore_q32=0))),
             ("eps1_vs_random_logged", B, True, ("random", {}), ("nearest", dict(explore_q32=1 << 32))),
             ("eps1_vs_random_4095", B - 1, False, ("random", {}), ("nearest", dict(explore_q32=1 << 32)))]
    for name, n, logged, a, b in pairs:
        env = BatchedTaskEnv(n, A, T, device=args.device)
        if logged:
            env.enable_rollout_log(32)
        seeds = env_seeds(1, 0, n)
        for side in (a, b):
            for _ in range(args.warmup):
                one(env, seeds, *side)
        ms, steps = {0: [], 1: []}, {}
        for _ in range(args.rounds):
            for i, side in enumerate((a, b)):
                r = [one(env, seeds, *side) for _ in range(args.reps)]
                ms[i].append(round(statistics.median(x[0] for x in r) * 1e3, 4))
                steps[i] = r[-1][1]
        assert steps[0] == steps[1], (name, steps)          # the two sides play the same episodes
        ma, mb = statistics.mean(ms[0]), statistics.mean(ms[1])
        print(json.dumps(dict(pair=name, shape=f"{n}x{A}A{T}T", episodes=EPISODES, rollout_log=logged, decisions=steps[0], twin_ms=ms[0],
                              explore_ms=ms[1], twin_mean_ms=round(ma, 4), explore_mean_ms=round(mb, 4),
                              explore_over_twin=round(mb / ma, 4), reps=args.reps, rounds=args.rounds)), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--device", default="cuda:0")
    ap.add_argument("--explore", action="store_true", help="time the epsilon-greedy forms against their twins instead")
    ap.add_argument("--rounds", type=int, default=5, help="--explore: alternations per pair")
    ap.add_argument("--individual", action="store_true", help="individual selection: individual_selection=True handle, rollout(individual=True)")
    ap.add_argument("--events", action="store_true", help="device events around the call instead of the host clock")
    args = ap.parse_args()
    if args.reps < 1:
        ap.error("--reps must be >= 1")
    if args.explore:
        return explore_pairs(args)
    env = BatchedTaskEnv(B, A, T, device=args.device, individual_selection=args.individual)
    seeds = env_seeds(1, 0, B)
    for policy in ("random", "first", "nearest"):
        for mode, stride in (("off", 0), ("on", B)):
            with torch.cuda.device(env.device):
                sec, steps = timed_rollouts(env, seeds, policy, stride, args.reps, args.warmup, individual=args.individual, events=args.events)
            assert int(env.instance_index().min()) == int(env.instance_index().max()) == (EPISODES - 1 if stride else 0)
            row = dict(shape=f"{B}x{A}A{T}T", policy=policy, individual=args.individual, renewal=mode, episodes=EPISODES,
                       clock="device events" if args.events else "host", ms=round(sec * 1e3, 4), decisions=steps,
                       ns_per_decision=round(sec * 1e9 / steps, 4), decisions_per_s=round(steps / sec, 1), reps=args.reps)
            sm = env.summary()
            row.update(mean_finished_tasks=round(float(sm[:, 1].mean()), 3), mean_makespan=round(float(sm[:, 3].mean()), 3))
            print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
