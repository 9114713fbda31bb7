"""Member removal of the register-resident kernels (Fast<>::task_update, the table-driven compaction of csrc/removal_table.hpp)
against the oracle, decision by decision.

Shapes: 256 envs of 6A/3T with requirements drawn from {3, 4, 5} -- five-member lists need five agents, three tasks keep every
removal on task lanes 0..2 with the agents' lanes on top of them -- and 64 envs of 20A/50T.  max_waiting_time is small, so both
removal rules fire often.  The oracle is walked with its step-wise API (the loop of worker.py:45-87 restated below; checked here
against the oracle's own rollout), which shows the member lists in front of and behind every task_update call.  From that walk
alone -- no kernel involved -- the inputs are shown to contain: a removal at each of the slots 0..4 of a five-member list, a
waiting-rule call that removes two non-adjacent members (the remove-while-iterating skip, env/task_env.py:268-271), a spread-rule
call with two or more leavers, and an agent removed by two tasks in one episode.  max_waiting_time and the seeds below were chosen
with that walk on the CPU.

On the GPU: the lockstep path (k_step_fast, which runs the same Fast<> text) is compared with the walk after every decision --
member lists in order, abandonment counts per (agent, task), the tasks' state, the observation -- and one persistent
rollout_random(episodes=3) launch (k_rollout_fast) with the oracle's three episodes: steps, the return log and summary(), bit for bit."""
import numpy as np
import pytest

import helpers as H

MAX_TIME = 100.0
#                 A,  T,   B, max_waiting_time, instance seed, choice seed, requirements
CASES = {"6A3T": (6, 3, 256, 1.5, 11, 5, (3, 4, 5)),
         "20A50T": (20, 50, 64, 2.0, 7, 3, None)}

_walks = {}


def instances(name):
    from dcmrta_amd.choice import env_seeds
    from dcmrta_amd.instances import generate_batch
    A, T, B, mwt, iseed, cseed, reqs = CASES[name]
    inst = generate_batch(B, A, T, base_seed=iseed)
    if reqs:
        inst["req"] = np.random.default_rng(iseed).choice(np.array(reqs, np.int32), size=(B, T)).astype(np.int32)
    return inst, env_seeds(cseed, 0, B)


def _load(oracle_lib, name, inst, b):
    A, T, _, mwt = CASES[name][:4]
    return oracle_lib.OracleEnv(A, T, max_waiting_time=mwt, max_time=MAX_TIME).load(inst["depot"][b], inst["task_xy"][b], inst["req"][b],
                                                                                 inst["dur"][b])


def walk_episode(o, req, seed_e):
    """One episode of the oracle through its step-wise API.  Returns (snaps, removals): the state in front of every decision, and one
    entry (task, rule, members before, positions that left) per task and task_update call that removed somebody."""
    from dcmrta_amd.choice import below, draw
    A, T = o.A, o.T
    members = [np.zeros(0, np.int32) for _ in range(T)]
    ab = np.zeros((A, T), np.int32)
    nab = np.zeros(T, np.int32)
    removals, snaps = [], []
    state = {}

    def task_update():
        o.task_update()
        f = o.final()
        for t in np.flatnonzero(f["n_abandoned"] != nab):
            old, new = members[t], o.members(t)
            left = [j for j, a in enumerate(old) if a not in new]
            assert len(left) == f["n_abandoned"][t] - nab[t] and len(new) == len(old) - len(left)
            removals.append((int(t), "spread" if req[t] - len(old) <= 0 else "wait", old.copy(), left))      # env/task_env.py:254
            for j in left:
                ab[old[j], t] += 1
            members[t] = new
        nab[:] = f["n_abandoned"]
        state.update(f)

    finished, d, empty = False, 0, 0
    while not finished and o.now < MAX_TIME:                               # worker.py:45
        ids, t = o.next_decision()                                         # :47
        groups = o.get_unique_group(ids) if len(ids) else []              # :48
        o.now = t                                                          # :49
        task_update()                                                      # :50
        o.agent_update()                                                   # :51
        if not groups:
            empty += 1
            if empty > 4:
                break
        else:
            empty = 0
        for group in groups:                                               # :52
            while group:                                                   # :53
                leader = group[below(draw(seed_e, d, 0), len(group))]      # :54
                mask, ag, tk = o.mask(), o.agent_status(leader), o.task_status(leader)
                snaps.append(dict(leader=leader, now=o.now, mask=mask, agents_obs=ag, tasks_obs=tk,
                                  members=list(members), abandoned=ab.copy(),       # (the arrays are replaced, never written)
                                  **{k: state[k] for k in ("n_members", "n_abandoned", "feasible", "finished", "time_start", "time_finish")}))
                action = H.host_random_action(mask, seed_e, d)
                snaps[-1]["action"] = action
                vacancy = int(tk[action, 0]) if action >= 1 else len(group)            # :327 (the status may be stale)
                group.remove(leader)                                       # :328
                step = [leader]
                if vacancy > 1:                                            # :330-333
                    for j in range(min(vacancy - 1, len(group))):
                        step.append(group.pop(below(draw(seed_e, d, 2 + j), len(group))))
                for m in step:
                    o.agent_step(m, action)                                # :338-340
                if action >= 1:
                    members[action - 1] = o.members(action - 1)
                task_update()                                              # :74
                o.agent_update()                                           # :76
                d += 1
        finished = o.check_finished()                                      # :85
    return snaps, removals


def walks(oracle_lib, name):
    """(instances, seeds, per-env snapshots, per-env removals, the oracle's own three episodes): computed once, read-only afterwards"""
    if name not in _walks:
        inst, seeds = instances(name)
        B = CASES[name][2]
        snaps, rem, eps = [], [], []
        for b in range(B):
            s, r = walk_episode(_load(oracle_lib, name, inst, b), inst["req"][b], int(seeds[b]))
            snaps.append(s); rem.append(r)
            three, d0 = [], 0
            for ep in range(3):
                three.append(_load(oracle_lib, name, inst, b).rollout(int(seeds[b]), d0, oracle_lib.POLICY_RANDOM, cap_steps=20000,
                                                                     record=(ep == 0)))
                d0 += three[-1]["n_steps"]
            eps.append(three)
        _walks[name] = (inst, seeds, snaps, rem, eps)
    return _walks[name]


def coverage(rem):
    """what the removals of a batch (per env: walk_episode's list) show"""
    slots5, wait_skip, spread_multi, two_tasks = set(), 0, 0, 0
    for env_rem in rem:
        by_agent = {}
        for t, rule, old, left in env_rem:
            if len(old) == 5:
                slots5.update(left)
            if rule == "wait" and any(q - p >= 2 for p, q in zip(left, left[1:])):
                wait_skip += 1
            if rule == "spread" and len(left) >= 2:
                spread_multi += 1
            for j in left:
                by_agent.setdefault(int(old[j]), set()).add(t)
        two_tasks += sum(1 for ts in by_agent.values() if len(ts) >= 2)
    return dict(slots5=slots5, wait_skip=wait_skip, spread_multi=spread_multi, two_tasks=two_tasks,
                calls=sum(len(r) for r in rem))


@pytest.mark.parametrize("name", list(CASES))
def test_the_walk_is_the_oracles_episode(oracle_lib, name):
    """The step-wise loop above against the oracle's own rollout of the first episode: every decision's record"""
    _, _, snaps, _, eps = walks(oracle_lib, name)
    for b, (s, three) in enumerate(zip(snaps, eps)):
        r = three[0]
        assert len(s) == r["n_steps"], (name, b)
        for k in ("leader", "action", "now", "mask", "agents_obs", "tasks_obs"):
            assert np.array_equal(np.array([x[k] for x in s]).reshape(r[k].shape), r[k]), (name, b, k)


def test_inputs_show_every_removal_case(oracle_lib):
    """The coverage condition, from the oracle alone"""
    cov = {name: coverage(walks(oracle_lib, name)[3]) for name in CASES}
    print(cov)
    c = cov["6A3T"]
    assert c["slots5"] == {0, 1, 2, 3, 4}, c           # a removal at every slot of a five-member list
    assert c["wait_skip"] >= 1, c                      # the waiting rule removes two non-adjacent members in one call (Q1)
    assert c["spread_multi"] >= 1, c                   # the spread rule with two or more leavers
    assert c["two_tasks"] >= 1, c                      # an agent removed by two tasks in one episode
    assert cov["20A50T"]["calls"] >= 64 * 10, cov["20A50T"]


def _env(gpu_device, name, inst):
    from dcmrta_amd.batched_env import BatchedTaskEnv
    A, T, B, mwt = CASES[name][:4]
    return BatchedTaskEnv(B, A, T, device=gpu_device, max_waiting_time=mwt).load_instances(**inst)


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CASES))
def test_lockstep_after_every_decision(gpu_device, oracle_lib, name):
    import torch
    A, T, B = CASES[name][:3]
    inst, seeds, snaps, _, eps = walks(oracle_lib, name)
    env = _env(gpu_device, name, inst)
    obs = env.reset(seeds)
    count = np.zeros(B, np.int64)
    for _ in range(max(len(s) for s in snaps) + 1):
        active = obs.active.cpu().numpy().astype(bool)
        assert np.array_equal(active, count < np.array([len(s) for s in snaps])), (name, count)
        if not active.any():
            break
        ag, tk, mk, ld = (x.cpu().numpy() for x in (obs.agents, obs.tasks, obs.mask, obs.leader))
        now = env.status()["now"].cpu().numpy()
        mem = env.task_members().cpu().numpy()
        abc = env.abandoned_counts().cpu().numpy()
        ts = {k: v.cpu().numpy() for k, v in env.tasks_state().items()}
        actions = np.zeros(B, np.int32)
        for b in np.flatnonzero(active):
            s = snaps[b][count[b]]
            tag = f"{name} env {b} decision {count[b]}"
            assert int(ld[b]) == s["leader"] and now[b] == s["now"], tag
            for t in range(T):
                want = np.full(mem.shape[2], -1, np.int16)
                want[:len(s["members"][t])] = s["members"][t]
                assert np.array_equal(mem[b, t], want), (tag, "members of task", t, mem[b, t], s["members"][t])
            assert np.array_equal(abc[b], s["abandoned"]), (tag, "abandonment counts")
            for k in ("n_members", "n_abandoned", "feasible", "finished", "time_start", "time_finish"):
                assert np.array_equal(ts[k][b].astype(s[k].dtype), s[k]), (tag, k, ts[k][b], s[k])
            assert np.array_equal(mk[b].astype(np.uint8), s["mask"]), (tag, "mask")
            assert np.array_equal(ag[b], s["agents_obs"]) and np.array_equal(tk[b], s["tasks_obs"]), (tag, "observation")
            actions[b] = s["action"]
            count[b] += 1
        obs = env.step(torch.from_numpy(actions).to(gpu_device))
    else:
        raise AssertionError("the lockstep loop did not end")
    sm = env.summary().cpu().numpy()
    for b in range(B):
        r = eps[b][0]
        assert sm[b, 0] == r["reward"] and int(sm[b, 1]) == int(r["finished"].sum()), (name, b)
        assert np.array_equal(sm[b, 2:8], r["metrics"]), (name, b, sm[b], r["metrics"])
    env.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CASES))
def test_three_episodes_in_one_launch(gpu_device, oracle_lib, name):
    B = CASES[name][2]
    inst, seeds, _, _, eps = walks(oracle_lib, name)
    env = _env(gpu_device, name, inst)
    ring = env.enable_return_log(3)
    env.reset(seeds, observe=False)
    steps = env.rollout_random(episodes=3).cpu().numpy()
    got, sm = ring.cpu().numpy(), env.summary().cpu().numpy()
    assert np.array_equal(steps, np.array([sum(r["n_steps"] for r in three) for three in eps])), name
    for b, three in enumerate(eps):
        assert [got[b, i] for i in range(3)] == [r["reward"] for r in three], (name, b)
        last = three[2]
        assert sm[b, 0] == last["reward"] and int(sm[b, 1]) == int(last["finished"].sum()), (name, b)
        assert np.array_equal(sm[b, 2:8], last["metrics"]), (name, b, sm[b], last["metrics"])
    env.close()
