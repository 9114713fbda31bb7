#!/usr/bin/env python3
"""What the best log costs and what it saves: B x 20A/50T under rollout("nearest", explore=eps, write_obs=False), E episodes per env,
three ways:

    best     one launch of E episodes with the best log set (k_bs_rollout_fast)
    rollout  the same launch with only the rollout log set (k_ex_rollout_fast)
    chain    the way to the same result without the best log: E launches of one episode, a summary read-back to the host after each

    python tools/best_log_time.py [--envs 4096] [--episodes 8] [--eps 0.05] [--reps 20] [--warmup 3] [--cap 64]

Every timed run starts from the same reset (outside the timed region), so all runs play the same episodes.  `best` and `rollout` are
timed with device events around the one launch; `chain` has host work inside (the read-backs), so it is timed with the host clock
between two synchronisations, and so are the other two a second time, for a like-for-like comparison (`*_host_ms`).  A figure is the
median of `reps` runs after `warmup`.  Checks that the three ways took the same number of decisions and that the best log's kept
rewards are the chain's maxima; prints one JSON line; sets no threshold; needs a HIP device."""
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
from dcmrta_amd.choice import env_seeds  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--episodes", type=int, default=8)
    ap.add_argument("--eps", type=float, default=0.05)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--cap", type=int, default=64)
    ap.add_argument("--device", default="cuda:0")
    args = ap.parse_args()
    if min(args.envs, args.episodes, args.reps, args.cap) < 1:
        ap.error("--envs, --episodes, --reps and --cap must be >= 1")
    B, E = args.envs, args.episodes
    env = BatchedTaskEnv(B, 20, 50, device=args.device)
    env.generate_instances(0)
    seeds = env_seeds(1, 0, B)
    play = lambda n: env.rollout("nearest", episodes=n, write_obs=False, explore=args.eps)

    def one_launch():
        return int(play(E).sum()), None

    def chain():
        steps, rows = 0, []
        for _ in range(E):
            steps += int(play(1).sum())
            rows.append(env.summary().cpu().numpy())
        return steps, np.stack(rows)

    def timed(run, events):
        dev_ms, host_ms, out = [], [], None
        for i in range(args.warmup + args.reps):
            env.reset(seeds, observe=False)
            torch.cuda.synchronize(env.device)
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t = time.perf_counter()
            a.record()
            out = run()
            b.record()
            torch.cuda.synchronize(env.device)
            if i >= args.warmup:
                host_ms.append((time.perf_counter() - t) * 1e3)
                dev_ms.append(a.elapsed_time(b))
        return (statistics.median(dev_ms) if events else None), statistics.median(host_ms), out

    env.enable_rollout_log(args.cap)
    env.enable_best_log()
    best_ms, best_host, (best_steps, _) = timed(one_launch, True)
    kept = env.best_summary().cpu().numpy()
    kept_ep = env.best_episode().cpu().numpy()
    env.enable_best_log(False)
    roll_ms, roll_host, (roll_steps, _) = timed(one_launch, True)
    _, chain_host, (chain_steps, rows) = timed(chain, False)
    assert best_steps == roll_steps == chain_steps, (best_steps, roll_steps, chain_steps)
    order = lambda r: (r[1], r[0])                                              # (finished tasks, reward)
    for b in range(B):
        k = max(range(E), key=lambda i: (order(rows[i, b]), -i))                # the earliest of the best
        assert k == kept_ep[b] and rows[k, b].tobytes() == kept[b].tobytes(), (b, k, int(kept_ep[b]))
    print(json.dumps(dict(shape=f"{B}x20A50T", policy="nearest", eps=args.eps, episodes=E, cap=args.cap, reps=args.reps, decisions=best_steps,
                          best_ms=round(best_ms, 4), rollout_ms=round(roll_ms, 4), best_over_rollout=round(best_ms / roll_ms, 4),
                          best_host_ms=round(best_host, 4), rollout_host_ms=round(roll_host, 4), chain_host_ms=round(chain_host, 4),
                          chain_over_best=round(chain_host / best_host, 4),
                          kept_not_last=int((kept_ep != E - 1).sum()), mean_kept_episode=round(float(kept_ep.mean()), 3))), flush=True)
    env.close()


if __name__ == "__main__":
    main()
