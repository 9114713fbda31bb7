"""The distance square root of the register-resident kernels (csrc/common.hpp, dist2_inrange: sqrt without the range scaling that
arguments below 2^-767 need) and the rule that keeps them off handles that hold such an argument (plan::Shape::inrange, checked on
the device when instances are loaded: csrc/dcmrta_env.hip, k_points_inrange).

Batches of 64 envs of 3A/4T with hand-made coordinates, played by rollout("random", episodes=2) -- decisions, both returns, summary()
-- by budget-1 launches of the persistent kernel, whose observation buffers then hold what each decision saw, and by a few step()
calls with the oracle's actions (the lockstep kernel: leader, mask, both observation tables in front of every decision).  The oracle
is the reference throughout (oracle_ref.two_episodes: the first episode recorded).  Cases:

    zero        two tasks on one point and a task on the depot: distances of exactly 0 (the class select of the sequence)
    ulp         coordinates that differ by 2^-53, the smallest difference two generated coordinates can have: squares of 2^-106
    tiny        in env 5 two points 2^-400 apart -- a square of 2^-800, below 2^-767: the handle must say it runs the general kernels,
                and match the oracle with them
    generated   a default batch made on the device: the register-resident kernels

and: a loaded batch of uniform [0, 1) coordinates runs the register-resident kernels, a ragged one works either way."""
import numpy as np
import pytest

import oracle_ref as O

A, T, B = 3, 4, 64
FAST, GENERAL = ("k_rollout_fast", "k_step_fast"), ("k_rollout_random", "k_step")
LOCKSTEP_DECISIONS, BUDGET_ONE_DECISIONS = 6, 6

_cases = {}


def _base():
    from dcmrta_amd.instances import generate_batch
    return {k: v.copy() for k, v in generate_batch(B, A, T, base_seed=23).items()}


def _make(name):
    inst = _base()
    xy, depot = inst["task_xy"], inst["depot"]
    if name == "zero":
        xy[:, 1] = xy[:, 0]                                  # two tasks on one point
        xy[:, 2] = depot                                     # a task on the depot
    elif name == "ulp":
        xy[:, 1, 0] = xy[:, 0, 0] + 2.0 ** -53               # x one step apart, y equal
        xy[:, 1, 1] = xy[:, 0, 1]
        xy[:, 3, 0] = depot[:, 0]                            # the depot's neighbour in y
        xy[:, 3, 1] = np.where(depot[:, 1] < 0.5, depot[:, 1] + 2.0 ** -53, depot[:, 1] - 2.0 ** -53)
        d = xy[:, 1, 0] - xy[:, 0, 0]
        assert np.all((d == 2.0 ** -53) | (d == 2.0 ** -52)) and np.all(xy[:, 3, 1] != depot[:, 1])   # (the sum rounds to a neighbour)
    elif name == "tiny":
        # around 2^-390 a double resolves 2^-400: the difference is exact, its square 2^-800 is a normal number below 2^-767
        xy[5, 0] = (2.0 ** -390, 0.25)
        xy[5, 1] = (2.0 ** -390 + 2.0 ** -400, 0.25)
        assert xy[5, 1, 0] - xy[5, 0, 0] == 2.0 ** -400 and 0.0 < (2.0 ** -400) ** 2 < 2.0 ** -767
    return inst


def case(name):
    """(instances, choice seeds, first-episode traces, second-episode results): computed once, read-only afterwards"""
    if name not in _cases:
        from dcmrta_amd.choice import env_seeds
        seeds = env_seeds(31, 0, B)
        if name == "generated":
            from dcmrta_amd.instances import generate_batch
            inst = generate_batch(B, A, T, base_seed=0)      # what generate_instances(arange(B)) makes on the device
        else:
            inst = _make(name)
        _cases[name] = (inst, seeds) + O.two_episodes(inst, seeds, A, T)
    return _cases[name]


def _env(gpu_device, name):
    from dcmrta_amd.batched_env import BatchedTaskEnv
    env = BatchedTaskEnv(B, A, T, device=gpu_device)
    if name == "generated":
        from fixtures_ref import assert_same_instances, held_instances
        env.generate_instances(np.arange(B, dtype=np.uint64))
        assert_same_instances(held_instances(env), case(name)[0], "the batch made on the device is the one the oracle plays")
        return env
    return env.load_instances(**case(name)[0])


CASES = {"zero": FAST, "ulp": FAST, "tiny": GENERAL, "generated": FAST}


def test_the_oracle_sees_the_cases():
    """From the oracle alone: in `zero` agents travel a distance of exactly 0 (an arrival at the time of the decision), in `tiny` env 5
    reaches both close points"""
    _, _, first, _ = case("zero")
    assert any(np.any(r["agents_obs"][1:, :, 0] == 0.0) for r in first)
    _, _, first, _ = case("tiny")
    assert {1, 2} <= set(int(a) for a in first[5]["action"])


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CASES))
def test_two_episodes_in_one_launch(gpu_device, name):
    inst, seeds, first, second = case(name)
    env = _env(gpu_device, name)
    assert (env.kernel_name("rollout"), env.kernel_name("step")) == CASES[name], name
    ring = env.enable_return_log(2)
    env.reset(seeds, observe=False)
    steps = env.rollout("random", episodes=2).cpu().numpy()
    got, sm = ring.cpu().numpy(), env.summary().cpu().numpy()
    for b in range(B):
        assert steps[b] == first[b]["n_steps"] + second[b]["n_steps"], (name, b)
        assert got[b, 0] == first[b]["reward"] and got[b, 1] == second[b]["reward"], (name, b)
        O.assert_summary(sm[b], second[b], f"{name} env {b}")
    env.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CASES))
def test_every_decision_of_budget_one_launches(gpu_device, name):
    """the persistent kernel one decision per launch: the observation buffers hold what the decision taken saw"""
    inst, seeds, first, _ = case(name)
    env = _env(gpu_device, name)
    env.reset(seeds, observe=False)
    for d in range(BUDGET_ONE_DECISIONS):
        steps = env.rollout("random", episodes=1, max_decisions=1).cpu().numpy()
        o = env.obs()
        ag, tk, mk = (x.cpu().numpy() for x in (o.agents, o.tasks, o.mask))
        now = env.status()["now"].cpu().numpy()
        for b in range(B):
            r = first[b]
            if d >= r["n_steps"]:
                continue
            tag = f"{name} env {b} decision {d}"
            assert steps[b] == 1, tag
            assert np.array_equal(ag[b], r["agents_obs"][d]) and np.array_equal(tk[b], r["tasks_obs"][d]), (tag, "observation")
            assert np.array_equal(mk[b].astype(np.uint8), r["mask"][d]), (tag, "mask")
            if d + 1 < r["n_steps"]:
                assert now[b] == r["now"][d + 1], (tag, "the clock in front of the next decision")
    env.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CASES))
def test_a_few_lockstep_decisions(gpu_device, name):
    import torch
    inst, seeds, first, _ = case(name)
    env = _env(gpu_device, name)
    obs = env.reset(seeds)
    for d in range(LOCKSTEP_DECISIONS):
        ag, tk, mk, ld = (x.cpu().numpy() for x in (obs.agents, obs.tasks, obs.mask, obs.leader))
        now = env.status()["now"].cpu().numpy()
        actions = np.zeros(B, np.int32)
        for b in range(B):
            r = first[b]
            assert d < r["n_steps"], (name, b, "an episode shorter than the decisions compared")
            tag = f"{name} env {b} decision {d}"
            assert int(ld[b]) == r["leader"][d] and now[b] == r["now"][d], tag
            assert np.array_equal(ag[b], r["agents_obs"][d]) and np.array_equal(tk[b], r["tasks_obs"][d]), (tag, "observation")
            assert np.array_equal(mk[b].astype(np.uint8), r["mask"][d]), (tag, "mask")
            actions[b] = r["action"][d]
        obs = env.step(torch.from_numpy(actions).to(gpu_device))
    env.close()


@pytest.mark.gpu
def test_which_kernels_a_handle_runs(gpu_device):
    """uniform [0, 1) coordinates: in range.  One env out of range takes the whole handle to the general kernels, the next load back.
    A ragged batch is checked at its envs' own sizes: a close pair in rows an env does not have changes nothing."""
    from dcmrta_amd.batched_env import BatchedTaskEnv
    from dcmrta_amd.choice import env_seeds
    env = BatchedTaskEnv(B, A, T, device=gpu_device)
    rng = np.random.default_rng(3)
    uniform = dict(depot=rng.random((B, 2)), task_xy=rng.random((B, T, 2)), req=case("zero")[0]["req"], dur=case("zero")[0]["dur"])
    assert env.load_instances(**uniform).kernel_name() == "k_rollout_fast" and env.kernel_name("step") == "k_step_fast"
    assert env.load_instances(**case("tiny")[0]).kernel_name() == "k_rollout_random" and env.kernel_name("step") == "k_step"
    snapshot = None
    env.reset(0, observe=False)
    snapshot = env.clone_state()
    assert env.load_instances(**uniform).kernel_name() == "k_rollout_fast"
    env.restore_state(snapshot)                               # the records of the out-of-range batch are back
    assert env.kernel_name() == "k_rollout_random"
    assert env.generate_instances(np.arange(B, dtype=np.uint64)).kernel_name() == "k_rollout_fast"
    # ragged: env 5 has two tasks, the close pair sits in its rows 2 and 3
    inst = {k: v.copy() for k, v in case("tiny")[0].items()}
    inst["task_xy"][5, 2:4] = inst["task_xy"][5, 0:2]
    inst["task_xy"][5, 0:2] = rng.random((2, 2))
    na, nt = np.full(B, A, np.int32), np.full(B, T, np.int32)
    nt[5] = 2
    env.load_instances(**inst, n_agents=na, n_tasks=nt)
    assert env.kernel_name() == "k_rollout_fast"
    nt[5] = 4
    env.load_instances(**inst, n_agents=na, n_tasks=nt)
    assert env.kernel_name() == "k_rollout_random"
    # ... and keeps working: env 5 of the ragged out-of-range batch against the oracle
    seeds = env_seeds(31, 0, B)
    env.reset(seeds, observe=False)
    steps = env.rollout("random", episodes=1).cpu().numpy()
    sm = env.summary().cpu().numpy()
    for b in (0, 5, B - 1):
        r = O.episodes(A, T, O.one(inst, b, int(nt[b])), seeds[b], "random", 1)[0]
        assert steps[b] == r["n_steps"], b
        O.assert_summary(sm[b], r, f"ragged env {b}")
    env.close()
