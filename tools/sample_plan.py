#!/usr/bin/env python3
"""A plan by sampling: play one instance many times under the epsilon-greedy `nearest` policy and keep the best episode.

    python tools/sample_plan.py [--agents 20 --tasks 50 --instance-seed 7000 | --golden I] [--envs 4096] [--eps 0.05] [--seed 11]
                                [--episodes 1] [--cap 64] [--out plan.yaml]

The instance -- generate_instance(agents, tasks, instance_seed), or the I-th of tests/golden/instances_20A50T.npz -- is replicated over
`envs` envs with seeds env_seed(seed, b).  Every env plays ONE episode of rollout("nearest", explore=eps) with the rollout log set; the
best env is the one with the largest pair (number of finished tasks, reward = -makespan).  Prints that pair next to the pair of the
pure `nearest` policy (one env: every episode of it on an instance ends alike) as one JSON line, and writes the best env's routes with
routes_to_yaml (the file Worker.generate_route writes, which load_routes / execute_routes replay).
With --episodes E > 1 every env plays E episodes in the ONE launch -- the decision counter keeps running across restarts, so they
differ -- with the best log set (enable_best_log): each env keeps its best episode on the device, the best env is picked from
best_summary, its best_plan is written, and the JSON line also carries `episodes` and the kept episode's ordinal `best_episode`.
Needs a HIP device."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from dcmrta_amd.batched_env import BatchedTaskEnv  # noqa: E402
from dcmrta_amd.choice import env_seeds, explore_q32  # noqa: E402
from dcmrta_amd.instances import generate_instance  # noqa: E402
from dcmrta_amd.trajectory import routes_to_yaml  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--agents", type=int, default=20)
    ap.add_argument("--tasks", type=int, default=50)
    ap.add_argument("--instance-seed", type=int, default=7000)
    ap.add_argument("--golden", type=int, default=None, help="take the I-th instance of tests/golden/instances_20A50T.npz instead")
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--eps", type=float, default=0.05)
    ap.add_argument("--seed", type=int, default=11, help="base of the env seeds env_seed(seed, b)")
    ap.add_argument("--episodes", type=int, default=1, help="episodes per env in the one launch; > 1 keeps each env's best on the device")
    ap.add_argument("--cap", type=int, default=64, help="entries per agent of the rollout log")
    ap.add_argument("--out", default="plan.yaml")
    ap.add_argument("--device", default="cuda:0")
    args = ap.parse_args()
    if args.envs < 1:
        ap.error("--envs must be >= 1")
    if args.episodes < 1:
        ap.error("--episodes must be >= 1")
    if args.golden is not None:
        z = np.load(os.path.join(ROOT, "tests", "golden", "instances_20A50T.npz"))
        if not 0 <= args.golden < len(z["depot"]):
            ap.error("--golden must be in 0..%d" % (len(z["depot"]) - 1))
        inst = {k: z[k][args.golden] for k in ("depot", "task_xy", "req", "dur")}
        A, T, source = int(z["A"]), inst["task_xy"].shape[0], "golden %d" % args.golden
    else:
        inst = generate_instance(args.agents, args.tasks, args.instance_seed)
        A, T, source = args.agents, args.tasks, "generate_instance(%d, %d, %d)" % (args.agents, args.tasks, args.instance_seed)
    rep = lambda n: [np.stack([np.asarray(inst[k])] * n) for k in ("depot", "task_xy", "req", "dur")]
    pair = lambda row: (int(row[1]), float(row[0]))                             # (finished tasks, reward) of a summary row

    greedy = BatchedTaskEnv(1, A, T, device=args.device).load_instances(*rep(1))
    greedy.reset(env_seeds(args.seed, 0, 1), observe=False)
    greedy.rollout("nearest", episodes=1, write_obs=False)
    g = pair(greedy.summary().cpu().numpy()[0])

    env = BatchedTaskEnv(args.envs, A, T, device=args.device).load_instances(*rep(args.envs))
    env.enable_rollout_log(args.cap)
    many = args.episodes > 1
    if many:
        env.enable_best_log()
    env.reset(env_seeds(args.seed, 0, args.envs), observe=False)
    steps = env.rollout("nearest", episodes=args.episodes, write_obs=False, explore=args.eps)
    sm = (env.best_summary() if many else env.summary()).cpu().numpy()
    best = max(range(args.envs), key=lambda b: pair(sm[b]))
    routes_to_yaml(env, args.out, best, log="best" if many else "rollout")      # ValueError if a route is longer than --cap
    s = pair(sm[best])
    line = dict(instance=source, envs=args.envs, eps=args.eps, explore_q32=explore_q32(args.eps), decisions=int(steps.sum()),
                nearest=dict(finished=g[0], reward=g[1]), sampled=dict(finished=s[0], reward=s[1], env=int(best)),
                distinct_returns=int(len(set(sm[:, 0].tolist()))), out=args.out)
    if many:
        line.update(episodes=args.episodes, best_episode=int(env.best_episode()[best]))
    print(json.dumps(line))


if __name__ == "__main__":
    main()
