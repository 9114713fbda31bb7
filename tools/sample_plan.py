#!/usr/bin/env python3
"""Plans by sampling: play an instance many times under the epsilon-greedy `nearest` policy and keep the best episode -- for N instances
in ONE handle and one launch.

    python tools/sample_plan.py [--agents 20 --tasks 50 --instance-seed 7000 | --golden I] [--instances 1] [--envs 4096] [--eps 0.05]
                                [--seed 11] [--episodes 1] [--cap 64] [--out plan.yaml]

Instance n -- generate_instance(agents, tasks, instance_seed + n), or the (I + n)-th of tests/golden/instances_20A50T.npz -- is
replicated over `envs` envs with seeds env_seed(seed, b), b < envs: envs [n * envs, (n + 1) * envs) of one handle of N * envs envs.
Every env plays `episodes` episodes of rollout("nearest", explore=eps) in the one launch (the decision counter keeps running across
restarts, so they differ) with the rollout log and the best log set: each env keeps its best episode on the device -- the largest pair
(number of finished tasks, reward = -makespan) -- and reduce_best(group=envs) picks each instance's best env and gathers its routes
there too.  Only the reduced buffers are read back: N summary rows and N plans, not the best log of N * envs envs.
Prints one JSON line: each instance's pair next to the pair of the pure `nearest` policy (one env: every episode of it on an instance
ends alike), and writes each winner's routes as the file Worker.generate_route writes, which load_routes / execute_routes replay.
With one instance the line has the scalar entries it always had and the file is --out; with N > 1 `instance`, `nearest`, `sampled`,
`distinct_returns`, `out` (and `best_episode`) are lists of N and the files are plan_<n>.yaml next to --out.  With --episodes E > 1 the
line also carries `episodes` and the kept episode's ordinal `best_episode`.
--individual: the same sampling under individual selection (Worker.run_test_IS): the handles are created with individual_selection=True
and every launch is rollout(..., individual=True).  That form has no best log, so it takes --episodes 1 and the winner is picked from
the summary rows on the host (the largest pair, ties to the lowest env) and its plan read from the rollout log.
Needs a HIP device."""
import argparse
import json
import os
import sys

import numpy as np
import torch
import yaml

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from dcmrta_amd.batched_env import BatchedTaskEnv, group_plan  # noqa: E402
from dcmrta_amd.choice import env_seeds, explore_q32  # noqa: E402
from dcmrta_amd.instances import generate_instance  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--agents", type=int, default=20)
    ap.add_argument("--tasks", type=int, default=50)
    ap.add_argument("--instance-seed", type=int, default=7000)
    ap.add_argument("--golden", type=int, default=None, help="take the I-th instance of tests/golden/instances_20A50T.npz instead")
    ap.add_argument("--instances", type=int, default=1, help="N instances (instance seed / golden index + n), each on its own --envs envs of the one handle")
    ap.add_argument("--envs", type=int, default=4096, help="envs per instance")
    ap.add_argument("--eps", type=float, default=0.05)
    ap.add_argument("--seed", type=int, default=11, help="base of the env seeds env_seed(seed, b)")
    ap.add_argument("--episodes", type=int, default=1, help="episodes per env in the one launch; every env keeps its best on the device")
    ap.add_argument("--cap", type=int, default=64, help="entries per agent of the rollout log")
    ap.add_argument("--out", default="plan.yaml", help="the plan file; with --instances N > 1, plan_<n>.yaml in its directory")
    ap.add_argument("--individual", action="store_true", help="individual selection: individual_selection=True handles, rollout(individual=True)")
    ap.add_argument("--device", default="cuda:0")
    args = ap.parse_args()
    if args.envs < 1:
        ap.error("--envs must be >= 1")
    if args.episodes < 1:
        ap.error("--episodes must be >= 1")
    if args.instances < 1:
        ap.error("--instances must be >= 1")
    if args.individual and args.episodes != 1:
        ap.error("--individual has no best log to keep an env's best episode: --episodes must be 1")
    N, K = args.instances, args.envs
    if args.golden is not None:
        z = np.load(os.path.join(ROOT, "tests", "golden", "instances_20A50T.npz"))
        if not 0 <= args.golden <= len(z["depot"]) - N:
            ap.error("--golden must be in 0..%d" % (len(z["depot"]) - N))
        insts = [{k: z[k][args.golden + n] for k in ("depot", "task_xy", "req", "dur")} for n in range(N)]
        A, T, sources = int(z["A"]), insts[0]["task_xy"].shape[0], ["golden %d" % (args.golden + n) for n in range(N)]
    else:
        insts = [generate_instance(args.agents, args.tasks, args.instance_seed + n) for n in range(N)]
        A, T = args.agents, args.tasks
        sources = ["generate_instance(%d, %d, %d)" % (A, T, args.instance_seed + n) for n in range(N)]
    # every instance `times` times, instance by instance
    rep = lambda times: [np.stack([np.asarray(inst[k]) for inst in insts for _ in range(times)]) for k in ("depot", "task_xy", "req", "dur")]
    pair = lambda row: (int(row[1]), float(row[0]))                             # (finished tasks, reward) of a summary row

    greedy = BatchedTaskEnv(N, A, T, device=args.device, individual_selection=args.individual).load_instances(*rep(1))
    greedy.reset(np.tile(env_seeds(args.seed, 0, 1), N), observe=False)
    greedy.rollout("nearest", episodes=1, write_obs=False, individual=args.individual)
    g = [pair(row) for row in greedy.summary().cpu().numpy()]

    env = BatchedTaskEnv(N * K, A, T, device=args.device, individual_selection=args.individual).load_instances(*rep(K))
    env.enable_rollout_log(args.cap)
    if not args.individual:
        env.enable_best_log()
    env.reset(np.tile(env_seeds(args.seed, 0, K), N), observe=False)
    steps = env.rollout("nearest", episodes=args.episodes, write_obs=False, explore=args.eps, individual=args.individual)
    outs = [args.out] if N == 1 else [os.path.join(os.path.dirname(args.out), "plan_%d.yaml" % n) for n in range(N)]
    if args.individual:
        # no best log: one episode per env, so the summary rows ARE the samples; the winner's plan is its rows of the rollout log
        rows, flags = env.summary().cpu().numpy(), env.status()["flags"].cpu().numpy()
        if ((flags & (8 | 16 | 32 | 256)) != 0).any():                          # DCM_FLAG_BAD_ACTION / OVERFLOW / BAD_LEADER / BAD_INSTANCE
            sys.exit("an env ended its episode with an error flag")
        distinct = [int(np.unique(rows[n * K:(n + 1) * K, 0]).size) for n in range(N)]
        winners = [n * K + max(range(K), key=lambda b, n=n: (pair(rows[n * K + b]), -b)) for n in range(N)]
        kept, sm = [0] * N, rows[winners]
        plans = [env.rollout_plan(w) for w in winners]                          # ValueError if a route is longer than --cap
    else:
        red = env.reduce_best(group=K)                                          # [N, ...]: all that leaves the device
        distinct = [int(torch.unique(env.best_summary()[n * K:(n + 1) * K, 0]).numel()) for n in range(N)]
        red = {k: v.cpu() for k, v in red.items()}
        winners, kept, sm = red["env"].tolist(), red["episode"].tolist(), red["summary"].numpy()
        if min(winners) < 0:
            sys.exit("no env of instance %d finished an episode without an error flag" % winners.index(min(winners)))
        plans = [group_plan(red, n) for n in range(N)]                          # ValueError if a route is longer than --cap
    for path, plan in zip(outs, plans):
        with open(path, "w") as f:
            yaml.dump({a: r for a, r in enumerate(plan)}, f, sort_keys=False)   # worker.py:246-248
    sampled = [dict(finished=pair(sm[n])[0], reward=pair(sm[n])[1], env=int(winners[n]) - n * K) for n in range(N)]
    nearest = [dict(finished=f, reward=r) for f, r in g]
    one = lambda xs: xs[0] if N == 1 else xs
    line = dict(instance=one(sources), envs=K, eps=args.eps, explore_q32=explore_q32(args.eps), decisions=int(steps.sum()),
                nearest=one(nearest), sampled=one(sampled), distinct_returns=one(distinct), out=one(outs))
    if args.individual:
        line.update(individual=True)
    if N > 1:
        line.update(instances=N)
    if args.episodes > 1:
        line.update(episodes=args.episodes, best_episode=one([int(k) for k in kept]))
    print(json.dumps(line))


if __name__ == "__main__":
    main()
