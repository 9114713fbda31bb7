"""Member removal of the register-resident kernels (Fast<>::task_update, the table-driven compaction of csrc/removal_table.hpp)
against the oracle, decision by decision.

Shapes: 256 envs of 6A/3T with requirements drawn from {3, 4, 5} -- five-member lists need five agents, three tasks keep every
removal on task lanes 0..2 with the agents' lanes on top of them -- and 64 envs of 20A/50T.  max_waiting_time is small, so both
removal rules fire often.  The oracle is walked with its step-wise API (removal_ref.walk_episode: the loop of worker.py:45-87 restated; checked here
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

import oracle_ref as O
from removal_ref import MAX_TIME, coverage, walk_episode

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


def walks(oracle_lib, name):
    """(instances, seeds, per-env snapshots, per-env removals, the oracle's own three episodes): computed once, read-only afterwards"""
    if name not in _walks:
        inst, seeds = instances(name)
        A, T, B, mwt = CASES[name][:4]
        snaps, rem, eps = [], [], []
        for b in range(B):
            s, r = walk_episode(_load(oracle_lib, name, inst, b), inst["req"][b], int(seeds[b]))
            snaps.append(s); rem.append(r)
            eps.append(O.episodes_first_recorded(A, T, O.one(inst, b), seeds[b], "random", 3, mwt))
        _walks[name] = (inst, seeds, snaps, rem, eps)
    return _walks[name]


@pytest.mark.parametrize("name", list(CASES))
def test_the_walk_is_the_oracles_episode(oracle_lib, name):
    """The step-wise loop of removal_ref.walk_episode against the oracle's own rollout of the first episode: every decision's record"""
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
