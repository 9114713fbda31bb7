#!/usr/bin/env python3
"""Route-replay history golden (run in the build container, where the reference is importable):

    python tests/golden/make_golden_replay_history.py   ->  tests/golden/replay_history.npz

For every CTAS-D test-set instance, the reference's execute_by_route (env/task_env.py:562-593) static and with
reactive_planning = True (make_golden.replay, the runs behind ctasd_replay.npz / reactive_replay.npz), then generate_traj
(:375-418) as plot_animation calls it (:431-439).  Stored per mode (prefix "static_" / "reactive_"):

  idx                      instances of the mode (the reactive run raises TypeError on reactive_replay.npz["raised"]: skipped)
  route                    i16[n, A, L]  agent['route'] (task id, -1 = depot), padded with -2
  arrival                  f64[n, A, L]  agent['arrival_time'], padded with 0
  route_len                i32[n, A]
  members                  i16[n, T, M]  task['members'] in list order, -1 padded
  feasible                 u8[n, T]      task['feasible_assignment']
  time_start, time_finish  f64[n, T]     what generate_traj reads of feasible tasks
  current_time             f64[n]        (asserted == the makespan of ctasd_replay.npz / reactive_replay.npz)
  traj_len                 i64[n, A]     rows of agent['trajectory'] (float64 [rows, 3])
  traj_sha256              str[n, A]     sha256 of that array's C-order bytes

Only numbers and digests are stored; no reference source.
"""
import hashlib
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as mg  # noqa: E402

MODES = (("static", False, "ctasd_replay.npz"), ("reactive", True, "reactive_replay.npz"))
# instances on which the reference's generate_traj does not complete, per mode, with the reason (none so far)
EXCLUDE = {"static": {}, "reactive": {}}


def traj_digest(traj):
    arr = np.ascontiguousarray(np.vstack(traj) if len(traj) else np.zeros((0, 3)), dtype=np.float64)
    assert arr.ndim == 2 and arr.shape[1] == 3
    return arr.shape[0], hashlib.sha256(arr.tobytes()).hexdigest()


def record(env):
    A, T = env.agents_num, env.tasks_num
    routes = [([int(x) for x in env.agent_dic[a]["route"]], [float(x) for x in env.agent_dic[a]["arrival_time"]]) for a in range(A)]
    members = [[int(m) for m in env.task_dic[t]["members"]] for t in range(T)]
    feasible = [bool(env.task_dic[t]["feasible_assignment"]) for t in range(T)]
    ts = [float(env.task_dic[t]["time_start"]) for t in range(T)]
    tf = [float(env.task_dic[t]["time_finish"]) for t in range(T)]
    current_time = float(env.current_time)
    env.generate_traj()                                     # plot_animation :431-439 (before stack_trajectory)
    digests = [traj_digest(env.agent_dic[a]["trajectory"]) for a in range(A)]
    return dict(routes=routes, members=members, feasible=feasible, ts=ts, tf=tf, current_time=current_time, digests=digests)


def main():
    out = {}
    for mode, reactive, known in MODES:
        ref = np.load(os.path.join(HERE, known))
        ref_idx = ref["idx"].tolist()
        rows, idx = [], []
        for i in range(50):
            if i in EXCLUDE[mode]:
                continue
            try:
                env = mg.replay(i, mg.ctasd_routes(i), reactive)
            except TypeError:                               # env/task_env.py:220 (pre_set_route None)
                assert i in ref["raised"].tolist(), (mode, i)
                continue
            r = record(env)
            assert r["current_time"] == float(ref["makespan"][ref_idx.index(i)]), (mode, i, r["current_time"])
            rows.append(r)
            idx.append(i)
        assert idx == [i for i in ref_idx if i not in EXCLUDE[mode]], mode
        assert len(idx) >= (40 if mode == "static" else 30), (mode, len(idx))
        n, A, T = len(rows), len(rows[0]["routes"]), len(rows[0]["members"])
        L = max(len(rt) for r in rows for rt, _ in r["routes"])
        M = max([len(m) for r in rows for m in r["members"]] + [1])
        route = np.full((n, A, L), -2, np.int16)
        arrival = np.zeros((n, A, L), np.float64)
        route_len = np.zeros((n, A), np.int32)
        members = np.full((n, T, M), -1, np.int16)
        traj_len = np.zeros((n, A), np.int64)
        traj_sha = np.full((n, A), "", dtype="<U64")
        for k, r in enumerate(rows):
            for a, (rt, ar) in enumerate(r["routes"]):
                route_len[k, a] = len(rt)
                route[k, a, :len(rt)] = rt
                arrival[k, a, :len(ar)] = ar
                traj_len[k, a], traj_sha[k, a] = r["digests"][a]
            for t, m in enumerate(r["members"]):
                members[k, t, :len(m)] = m
        out.update({f"{mode}_idx": np.array(idx, np.int32), f"{mode}_route": route, f"{mode}_arrival": arrival,
                    f"{mode}_route_len": route_len, f"{mode}_members": members,
                    f"{mode}_feasible": np.array([r["feasible"] for r in rows], np.uint8),
                    f"{mode}_time_start": np.array([r["ts"] for r in rows], np.float64),
                    f"{mode}_time_finish": np.array([r["tf"] for r in rows], np.float64),
                    f"{mode}_current_time": np.array([r["current_time"] for r in rows], np.float64),
                    f"{mode}_traj_len": traj_len, f"{mode}_traj_sha256": traj_sha})
        print(mode, "instances", n, "max route", L, "max members", M, "trajectory rows", int(traj_len.sum()), flush=True)
    np.savez_compressed(os.path.join(HERE, "replay_history.npz"), **out)


if __name__ == "__main__":
    main()
