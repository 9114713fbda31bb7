"""The wave-uniform conditions of Fast<> and of the decision loop of k_rollout_fast (common.hpp, "Wave-uniform conditions": the draw
behind `nv`, `go` / `quiet` / `unsettled` in apply and task_update, `apart` in next_event, the latch's `turn` / `ahead` / `more`, the empty-group
fix-up as arithmetic) against the oracle, at every place a persistent launch can stop.

Shapes: 64 envs of 20A/50T; 64 envs of a ragged 10-20A / 20-50T batch on a 20A/50T handle (the runtime-size layout); 64 envs of 8A/6T with
every requirement 5, where the first decision of every episode -- eight agents in one group at the depot, a task with four vacancies
behind the leader -- draws four followers.  max_waiting_time 2, so both removal rules fire.  Seeds below were chosen on the CPU with the
oracle so that its own run of these inputs (two episodes per env, recorded) holds what the conditions decide on; the first test checks
that from the oracle alone.

On the GPU each batch plays its two episodes through rollout_random(episodes=2) twice over: once under per-env random budgets of 1..47
decisions per launch (never beyond the env's second episode, so the restart between the episodes falls inside a launch and every env
stops in the middle of episodes, at their ends and on the decision in front of an event), once with a budget of 1 for the first 40
decisions.  After every stop: the steps taken, the three observation buffers (the observation in front of the last decision taken;
pad rows of a ragged batch included), summary() (the last finished episode's row) and status() (flags, decision counter) bit for bit
against the oracle's records, through tests/oracle_ref.py."""
import numpy as np
import pytest

import oracle_ref as O

MWT = 2.0
EPISODES = 2
B = 64
#                A,  T, instance seed(s), choice seed
CASES = {"20A50T": (20, 50, 7, 3),
         "ragged": (20, 50, 300, 9),
         "8A6T_req5": (8, 6, 21, 5)}
_inputs, _oracle = {}, {}


def inputs(name):
    from dcmrta_amd.choice import env_seeds
    from dcmrta_amd.instances import generate_batch, generate_batch_ranges
    if name not in _inputs:
        A, T, iseed, cseed = CASES[name]
        if name == "ragged":
            inst = generate_batch_ranges(range(iseed, iseed + B), (10, 20), (20, 50))
        else:
            inst = generate_batch(B, A, T, base_seed=iseed)
            if name == "8A6T_req5":
                inst["req"] = np.full((B, T), 5, np.int32)
        _inputs[name] = (inst, env_seeds(cseed, 0, B))
    return _inputs[name]


def sizes(name, b):
    inst = inputs(name)[0]
    return (int(inst["n_agents"][b]), int(inst["n_tasks"][b])) if "n_agents" in inst else CASES[name][:2]


def oracle_episodes(name):
    """The two recorded oracle episodes of every env (computed once, read-only afterwards)"""
    if name not in _oracle:
        inst, seeds = inputs(name)
        _oracle[name] = []
        for b in range(B):
            a, t = sizes(name, b)
            eps = O.episodes(a, t, O.one(inst, b, t), seeds[b], "random", EPISODES, MWT, record=True)
            for r in eps:                                                   # (the records are views of the oracle's 20000-row buffers)
                for k in ("nfol", "action", "now", "mask", "agents_obs", "tasks_obs"):
                    r[k] = r[k].copy()
                for k in ("leader", "followers"):
                    del r[k]
            _oracle[name].append(eps)
    return _oracle[name]


def coverage(name, oracle_lib):
    """What the oracle's own run of a batch holds: decisions with two or more followers, events with several deciders, depot actions that
    take the rest of a group along (both episodes, from the records), members removed under each rule (first episodes, from the step-wise
    walk of removal_ref, which names the rule), first decisions with four followers"""
    from removal_ref import walk_episode
    inst, seeds = inputs(name)
    c = dict(followers2=0, several=0, depot_rest=0, spread=0, wait=0, first4=0)
    for b, eps in enumerate(oracle_episodes(name)):
        a, t = sizes(name, b)
        for r in eps:
            c["followers2"] += int((r["nfol"] >= 2).sum())
            c["depot_rest"] += int(((r["action"] == 0) & (r["nfol"] >= 1)).sum())
            c["first4"] += int(r["nfol"][0] == 4)
            deciders = 1 + r["nfol"].astype(np.int64)
            starts = np.flatnonzero(np.r_[True, r["now"][1:] != r["now"][:-1]])
            c["several"] += int((np.add.reduceat(deciders, starts) >= 2).sum())
        one = O.one(inst, b, t)
        o = oracle_lib.OracleEnv(a, t, max_waiting_time=MWT).load(one["depot"], one["task_xy"], one["req"], one["dur"])
        snaps, rem = walk_episode(o, one["req"], int(seeds[b]))
        assert len(snaps) == eps[0]["n_steps"], (name, b, "the walk is not the oracle's episode")
        for _, rule, _, left in rem:
            c[rule] += len(left)
    return c


def test_inputs_hold_what_the_conditions_decide_on(oracle_lib):
    cov = {name: coverage(name, oracle_lib) for name in CASES}
    print(cov)
    tot = {k: sum(c[k] for c in cov.values()) for k in next(iter(cov.values()))}
    assert tot["followers2"] >= 100, tot                 # decisions with two or more followers
    assert tot["several"] >= 20, tot                     # events with several deciders
    assert tot["spread"] >= 10 and tot["wait"] >= 10, tot    # member removals under each of the two rules
    assert tot["depot_rest"] >= 1, tot                   # a depot action with a non-empty rest of the group
    assert cov["8A6T_req5"]["first4"] == EPISODES * B, cov["8A6T_req5"]     # the first decision of every episode draws four followers


def _env(gpu_device, name):
    from dcmrta_amd.batched_env import BatchedTaskEnv
    A, T = CASES[name][:2]
    inst, seeds = inputs(name)
    env = BatchedTaskEnv(B, A, T, device=gpu_device, max_waiting_time=MWT).load_instances(**inst)
    env.reset(seeds, observe=False)
    return env


def _check_stop(env, name, tag, taken, want, g):
    """After a launch: `taken` (the steps it returned) against the budgets `want`, and env b's readable state against the oracle's records
    at g[b] decisions since the reset"""
    A, T = CASES[name][:2]
    eps = oracle_episodes(name)
    assert np.array_equal(taken, want), (tag, "steps", np.flatnonzero(taken != want)[:8])
    o, st = env.obs(), env.status()
    ag, tk, mk = (x.cpu().numpy() for x in (o.agents, o.tasks, o.mask))
    flags, dec, sm = st["flags"].cpu().numpy(), st["decisions"].cpu().numpy(), env.summary().cpu().numpy()
    for b in range(B):
        a, t = sizes(name, b)
        n0, n1 = eps[b][0]["n_steps"], eps[b][1]["n_steps"]
        j, k = (0, g[b]) if g[b] <= n0 else (1, g[b] - n0)                  # the episode the env is in, the decisions taken in it
        done = k == (n0, n1)[j]
        t2 = (tag, "env", b, "episode", j, "decision", int(k))
        assert dec[b] == g[b], (t2, "decision counter", int(dec[b]))
        r = eps[b][j]
        # flags: DONE, with it FINISHED iff every task is finished and every agent back, TRUNCATED iff the oracle's guard fired; no error (bit 128 is informational)
        want_flags = (1 | (2 if r["finished"].all() and r["returned"].all() else 0) | (4 if r["truncated"] else 0)) if done else 0
        assert (int(flags[b]) & ~128) == want_flags, (t2, "flags", int(flags[b]), want_flags)
        if want[b] > 0:                                                     # the observation in front of the last decision taken
            assert np.array_equal(mk[b, :t + 1].astype(np.uint8), r["mask"][k - 1]) and np.all(mk[b, t + 1:] == 1), (t2, "mask")
            assert np.array_equal(ag[b, :a].view(np.uint32), r["agents_obs"][k - 1].view(np.uint32)) and np.all(ag[b, a:] == -1.0), (t2, "agents")
            assert np.array_equal(tk[b, :t + 1].view(np.uint32), r["tasks_obs"][k - 1].view(np.uint32)) and np.all(tk[b, t + 1:] == -1.0), (t2, "tasks")
        last = j if done else j - 1                                         # the last finished episode: its row stays readable
        if last >= 0:
            assert np.array_equal(sm[b].view(np.uint64), O.summary_row(eps[b][last]).view(np.uint64)), (t2, "summary", sm[b])


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CASES))
def test_random_budgets_through_two_episodes(gpu_device, oracle_lib, name):
    eps = oracle_episodes(name)
    total = np.array([e[0]["n_steps"] + e[1]["n_steps"] for e in eps], np.int64)
    env = _env(gpu_device, name)
    rng = np.random.default_rng(1)
    g = np.zeros(B, np.int64)
    for launch in range(10000):
        if (g == total).all():
            break
        want = np.minimum(rng.integers(1, 48, B), total - g)               # (0 for an env that is through: it must stay where it is)
        taken = env.rollout_random(episodes=EPISODES, max_decisions=want).cpu().numpy()
        g += want
        _check_stop(env, name, f"{name} launch {launch}", taken, want, g)
    assert (g == total).all() and launch >= 5, (name, launch)
    assert np.array_equal(env.episodes().cpu().numpy(), np.full(B, EPISODES)), name
    env.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CASES))
def test_budget_of_one_for_the_first_40_decisions(gpu_device, oracle_lib, name):
    eps = oracle_episodes(name)
    total = np.array([e[0]["n_steps"] + e[1]["n_steps"] for e in eps], np.int64)
    env = _env(gpu_device, name)
    g = np.zeros(B, np.int64)
    for launch in range(40):
        want = np.minimum(1, total - g)
        taken = env.rollout_random(episodes=EPISODES, max_decisions=want).cpu().numpy()
        g += want
        _check_stop(env, name, f"{name} budget 1, launch {launch}", taken, want, g)
    env.close()
