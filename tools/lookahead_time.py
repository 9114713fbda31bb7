#!/usr/bin/env python3
"""The rollout algorithm two ways, timed: the host-driven Lookahead.plan() against the device form rollout(policy, lookahead=True).

    host          Lookahead.plan(): per decision one fork into B (T + 1) branches, one step of the branches, one persistent launch of the
                  base policy over them, one step of the B envs and one host synchronisation
    device        one persistent launch (dcm_rollout_lookahead): every env's wave values its own unmasked actions one after the other

    python tools/lookahead_time.py [--envs 4 1024] [--agents 20] [--tasks 50] [--policy nearest] [--reps 1] [--width W ...]

Env b plays generate_instance(agents, tasks, 7000 + b) under env_seeds(11, 0, B)[b].  Each way is timed with device events around one
whole plan (reset excluded), after ONE warm-up plan on the same handles; with --reps > 1 the figure is the median.  The two ways are
checked to leave the same summary rows and the same number of decisions.  Per batch size one JSON line: both times, the decisions of
the plans themselves (`decisions`, the same for both), the host form's launches and the decisions its branches played
(`branch_decisions`; the device form plays the unmasked branches only: `inner_decisions`, the sum of its inner_out, taken in a launch
of its own through dcm_rollout_lookahead_width so that the timed launch stays the old entry's).
--width W [W ...]: per W one more JSON line for the device form alone, rollout(policy, lookahead=True, width=W): its time, its decisions,
the summed inner decisions and the mean reward of the plans (a width-limited plan is another plan: nothing is compared).  Sets no
threshold; needs a HIP device."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from dcmrta_amd.batched_env import BatchedTaskEnv  # noqa: E402
from dcmrta_amd.choice import env_seeds  # noqa: E402
from dcmrta_amd.lookahead import Lookahead  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, nargs="+", default=[4, 1024])
    ap.add_argument("--agents", type=int, default=20)
    ap.add_argument("--tasks", type=int, default=50)
    ap.add_argument("--policy", default="nearest", choices=sorted(BatchedTaskEnv.POLICIES))
    ap.add_argument("--reps", type=int, default=1)
    ap.add_argument("--width", type=int, nargs="+", default=[], help="also time the device form with these candidate-list widths")
    ap.add_argument("--torch-device", default="cuda:0")
    args = ap.parse_args()
    A, T, dev = args.agents, args.tasks, args.torch_device

    def timed(plan, reset):
        ms = []
        for i in range(1 + args.reps):                                          # one warm-up
            reset()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            out = plan()
            b.record()
            torch.cuda.synchronize(dev)
            if i:
                ms.append(a.elapsed_time(b))
        return statistics.median(ms), out

    for B in args.envs:
        seeds = env_seeds(11, 0, B)
        host = BatchedTaskEnv(B, A, T, device=dev)
        host.generate_instances(7000)
        la = Lookahead(host, args.policy)

        def host_reset():
            host.reset(seeds, observe=False)
            la.launches = 0
            la.decisions.zero_()
        host_ms, launches = timed(la.plan, host_reset)
        device = BatchedTaskEnv(B, A, T, device=dev)
        device.generate_instances(7000)
        device_ms, steps = timed(lambda: device.rollout(args.policy, episodes=1, write_obs=False, lookahead=True),
                                 lambda: device.reset(seeds, observe=False))
        assert torch.equal(host.summary(), device.summary()), "the two forms leave different summary rows"
        assert torch.equal(host.status()["decisions"], steps), "the two forms took different numbers of decisions"
        device.reset(seeds, observe=False)
        inner = device.rollout(args.policy, episodes=1, write_obs=False, lookahead=True, return_inner=True)[1]
        print(json.dumps(dict(shape=f"{B}x{A}A{T}T", policy=args.policy, reps=args.reps, decisions=int(steps.sum()),
                              longest_episode=int(steps.max()), host_ms=round(host_ms, 2), host_launches=int(launches),
                              branch_decisions=int(la.decisions), device_ms=round(device_ms, 2), inner_decisions=int(inner.sum()),
                              reward_mean=round(float(device.summary()[:, 0].mean()), 3),
                              device_over_host=round(device_ms / host_ms, 3))), flush=True)
        for W in args.width:
            ms, (steps, inner) = timed(lambda: device.rollout(args.policy, episodes=1, write_obs=False, lookahead=True, width=W, return_inner=True),
                                       lambda: device.reset(seeds, observe=False))
            print(json.dumps(dict(shape=f"{B}x{A}A{T}T", policy=args.policy, reps=args.reps, width=W, decisions=int(steps.sum()),
                                  longest_episode=int(steps.max()), device_ms=round(ms, 2), inner_decisions=int(inner.sum()),
                                  reward_mean=round(float(device.summary()[:, 0].mean()), 3))), flush=True)
        la.close()
        host.close()
        device.close()


if __name__ == "__main__":
    main()
