#!/usr/bin/env python3
"""Plans by lookahead: the rollout algorithm over the `nearest` policy -- at every decision value every action by a `nearest` rollout
and take the best -- for N instances in one handle.

    python tools/lookahead_plan.py [--agents 20 --tasks 50 --instance-seed 7000 | --golden I] [--instances 4] [--seed 11] [--cap 64]
                                   [--out plan.yaml] [--device [--width W]]

Instance n -- generate_instance(agents, tasks, instance_seed + n), or the (I + n)-th of tests/golden/instances_20A50T.npz -- is env n
of one handle of N envs, all with the seed env_seed(seed, 0), as in tools/sample_plan.py.  Lookahead.plan() forks the N envs into
N (T + 1) branches at every decision (dcm_fork_envs), steps branch a with action a, plays the branches to their ends under `nearest` in
one persistent launch and steps each env with the action whose episode finishes the most tasks, then has the largest reward; the
handle's route log holds the plan.  The choice protocol makes this exact: a plan never ends below the `nearest` episode of its seed.
Prints one JSON line: each instance's (finished, reward) under `nearest` and under the lookahead plan, the number of lookahead
launches (one fork + one step + one persistent launch of N (T + 1) envs each) and the decisions those launches played -- what to
give the sampler of tools/sample_plan.py for a comparison at equal decisions spent -- and writes each plan as the file
Worker.generate_route writes (--out with one instance, plan_<n>.yaml next to it otherwise).  Needs a HIP device.
--device (bare, no value): the same plans from ONE persistent launch, rollout("nearest", lookahead=True) (dcm_rollout_lookahead): every
env's wave values its own actions one after the other and takes the best, nothing returns to the host, and the plan is read from the
rollout log.  Same rewards, same plan files; the JSON line then has lookahead_launches = 1, branches = 0 and decisions = the decisions
of the plan itself (the inner episodes' are not counted on the device).  `--device cuda:N` with a value keeps its old meaning, the GPU
of the host-driven run; --torch-device names the GPU for either.
--width W (with bare --device): every decision values only the W unmasked tasks nearest to the leader (dcm_rollout_lookahead_width;
0, the default: all of them).  Another, cheaper plan: the JSON line gains width and inner_decisions, the base-policy decisions the
inner episodes played."""
import argparse
import json
import os
import sys

import numpy as np
import yaml

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from dcmrta_amd.batched_env import BatchedTaskEnv  # noqa: E402
from dcmrta_amd.choice import env_seeds  # noqa: E402
from dcmrta_amd.instances import generate_instance  # noqa: E402
from dcmrta_amd.lookahead import Lookahead  # noqa: E402
from dcmrta_amd.trajectory import route_lists  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--agents", type=int, default=20)
    ap.add_argument("--tasks", type=int, default=50)
    ap.add_argument("--instance-seed", type=int, default=7000)
    ap.add_argument("--golden", type=int, default=None, help="take the I-th instance of tests/golden/instances_20A50T.npz instead")
    ap.add_argument("--instances", type=int, default=4, help="N instances (instance seed / golden index + n), one env each")
    ap.add_argument("--seed", type=int, default=11, help="base of the env seed env_seed(seed, 0)")
    ap.add_argument("--cap", type=int, default=64, help="entries per agent of the route log")
    ap.add_argument("--out", default="plan.yaml", help="the plan file; with --instances N > 1, plan_<n>.yaml in its directory")
    ap.add_argument("--device", nargs="?", default=None, const=True,
                    help="bare: plan with one persistent launch (the device form); with a value: the GPU, as --torch-device")
    ap.add_argument("--torch-device", default="cuda:0")
    ap.add_argument("--width", type=int, default=None, help="with bare --device: value only the W nearest unmasked tasks (0: all)")
    args = ap.parse_args()
    if args.instances < 1:
        ap.error("--instances must be >= 1")
    on_device = args.device is True
    if args.width is not None and (not on_device or args.width < 0):
        ap.error("--width W >= 0 belongs to the device form: give a bare --device")
    args.device = args.torch_device if args.device in (None, True) else args.device
    N = args.instances
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
    batch = [np.stack([np.asarray(inst[k]) for inst in insts]) for k in ("depot", "task_xy", "req", "dur")]
    seeds = np.tile(env_seeds(args.seed, 0, 1), N)
    pair = lambda row: dict(finished=int(row[1]), reward=float(row[0]))         # of a summary row

    greedy = BatchedTaskEnv(N, A, T, device=args.device).load_instances(*batch)
    greedy.reset(seeds, observe=False)
    greedy.rollout("nearest", episodes=1, write_obs=False)
    nearest = [pair(row) for row in greedy.summary().cpu().numpy()]

    env = BatchedTaskEnv(N, A, T, device=args.device).load_instances(*batch)
    extra = {}
    if on_device:
        env.enable_rollout_log(args.cap)
        env.reset(seeds, observe=False)
        launches, branches = 1, 0
        if args.width is None:
            decisions = int(env.rollout("nearest", episodes=1, write_obs=False, lookahead=True).sum())
        else:
            steps, inner = env.rollout("nearest", episodes=1, write_obs=False, lookahead=True, width=args.width, return_inner=True)
            decisions, extra = int(steps.sum()), dict(width=args.width, inner_decisions=int(inner.sum()))
        routes_of = env.rollout_routes
    else:
        env.enable_route_log(args.cap)
        env.reset(seeds, observe=False)
        la = Lookahead(env, "nearest")
        launches, branches = la.plan(), N * (T + 1)
        decisions = int(la.decisions)
        routes_of = env.routes
    plan = [pair(row) for row in env.summary().cpu().numpy()]
    task, arrival, length = (x.cpu().numpy() for x in routes_of())
    outs = [args.out] if N == 1 else [os.path.join(os.path.dirname(args.out), "plan_%d.yaml" % n) for n in range(N)]
    for n, path in enumerate(outs):
        with open(path, "w") as f:                                              # route_lists: ValueError if a route is longer than --cap
            routes = [[t + 1 for t in r] for r, _ in route_lists(task[n], arrival[n], length[n], "--cap")]
            yaml.dump({a: r for a, r in enumerate(routes)}, f, sort_keys=False)  # worker.py:246-248
    one = lambda xs: xs[0] if N == 1 else xs
    print(json.dumps(dict(instance=one(sources), instances=N, nearest=one(nearest), lookahead=one(plan), lookahead_launches=launches,
                          branches=branches, decisions=decisions, improved=sum((p["finished"], p["reward"]) > (g["finished"], g["reward"])
                                                                                  for p, g in zip(plan, nearest)), out=one(outs), **extra)))


if __name__ == "__main__":
    main()
