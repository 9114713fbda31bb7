#!/usr/bin/env python3
"""What picking the best plan costs on the device and on the host: B x 20A/50T envs whose best log holds E episodes of
rollout("nearest", explore=eps), reduced per group of `group` envs.

    reduce        BatchedTaskEnv.reduce_best(group): allocation and fill of the outputs + the kernel k_reduce_best
    kernel        dcm_reduce_best alone, into buffers allocated once
    host_rows     the host's way for ONE group of B envs, as tools/sample_plan.py did it before reduce_best: best_summary().cpu(), a
                  Python max over B rows, then the winner's rows of best_routes() (three indexed device-to-host copies)
    host_all      the same pick, then best_plan(b): the whole best_routes() buffers to the host for one env's rows

    python tools/reduce_best_time.py [--envs 4096] [--groups 4096 64] [--episodes 2] [--eps 0.05] [--cap 64] [--reps 20] [--warmup 3] [--calls 200]

`reduce` and `kernel` are timed with device events around `calls` back-to-back calls (one call is far below the events' resolution)
and reported per call; the host paths end in a synchronising copy and are timed with the host clock, one pick per run.  A figure is
the median of `reps` runs after `warmup`.  Checks that the device's winner of the one-group reduction is the host's; prints one JSON
line; sets no threshold; needs a HIP device."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from dcmrta_amd.batched_env import BatchedTaskEnv  # noqa: E402
from dcmrta_amd.choice import env_seeds  # noqa: E402
from dcmrta_amd._lib import check  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--groups", type=int, nargs="+", default=[4096, 64])
    ap.add_argument("--episodes", type=int, default=2)
    ap.add_argument("--eps", type=float, default=0.05)
    ap.add_argument("--cap", type=int, default=64)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--device", default="cuda:0")
    args = ap.parse_args()
    if min([args.envs, args.episodes, args.cap, args.reps, args.calls] + args.groups) < 1:
        ap.error("--envs, --groups, --episodes, --cap, --reps and --calls must be >= 1")
    B = args.envs
    env = BatchedTaskEnv(B, 20, 50, device=args.device)
    env.generate_instances(0)
    env.enable_rollout_log(args.cap)
    env.enable_best_log()
    env.reset(env_seeds(1, 0, B), observe=False)
    env.rollout("nearest", episodes=args.episodes, write_obs=False, explore=args.eps)
    torch.cuda.synchronize(env.device)

    def median_of(run):
        ms = []
        for i in range(args.warmup + args.reps):
            t = run()
            if i >= args.warmup:
                ms.append(t)
        return statistics.median(ms)

    def events(call):
        def run():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(args.calls):
                call()
            b.record()
            torch.cuda.synchronize(env.device)
            return a.elapsed_time(b) / args.calls
        return median_of(run)

    def host(pick):
        def run():
            torch.cuda.synchronize(env.device)
            t = time.perf_counter()
            pick()
            return (time.perf_counter() - t) * 1e3
        return median_of(run)

    def host_winner():
        sm = env.best_summary().cpu().numpy()
        return max(range(B), key=lambda b: (int(sm[b, 1]), float(sm[b, 0])))

    def host_rows():
        b = host_winner()
        return b, [x[b].cpu().numpy() for x in env.best_routes()]

    def host_all():
        b = host_winner()
        return b, env.best_plan(b)

    out = dict(shape=f"{B}x20A50T", episodes=args.episodes, eps=args.eps, cap=args.cap, reps=args.reps, calls=args.calls, groups={})
    for group in args.groups:
        red = env.reduce_best(group=group)
        ptrs = [C.c_void_p(red[k].data_ptr()) for k in ("env", "summary", "episode", "len", "task", "arrival")]
        raw = lambda: check(env._lib.dcm_reduce_best(env._h, group, *ptrs, env._stream()))
        out["groups"][str(group)] = dict(n_groups=int(red["env"].shape[0]), reduce_us=round(1e3 * events(lambda: env.reduce_best(group=group)), 3),
                                         kernel_us=round(1e3 * events(raw), 3))
    whole = env.reduce_best(group=B)
    winner = int(whole["env"][0])
    assert winner == host_winner(), (winner, host_winner())
    assert env.group_plan(whole, 0) == env.best_plan(winner)
    out.update(host_rows_ms=round(host(host_rows), 4), host_all_ms=round(host(host_all), 4),
               best_log_bytes=sum(x.numel() * x.element_size() for x in env.best_routes()),
               plan_bytes=sum(whole[k].numel() * whole[k].element_size() for k in ("len", "task", "arrival")))
    print(json.dumps(out), flush=True)
    env.close()


if __name__ == "__main__":
    main()
