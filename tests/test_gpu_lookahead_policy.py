"""-m gpu: one-step lookahead as a device policy (dcm_rollout_lookahead; BatchedTaskEnv.rollout(policy, lookahead=True); the kernels
k_la_rollout_random / k_larn_rollout_random): one persistent launch plays the rollout algorithm.

Yardsticks, both matched bit for bit: the step-wise oracle walker under the lookahead rule (lookahead_policy_ref.lookahead_walk), and
the host-driven Lookahead.plan(), which test_gpu_lookahead.py pins to the oracle.  Second episodes have the seed-shifted fresh handle
as their reference (a running decision counter is a seed shift, test_lookahead_policy_ref_host.py)."""
import numpy as np
import pytest

import lookahead_policy_ref as LP
import oracle_ref as O

pytestmark = pytest.mark.gpu

ERR_INVALID, ERR_STATE = -1, -4
CAP = 64


def make(gpu_device, B, A, T, inst, log=True, **kw):
    from dcmrta_amd.batched_env import BatchedTaskEnv
    env = BatchedTaskEnv(B, A, T, device=gpu_device, **kw).load_instances(**inst)
    if log:
        env.enable_rollout_log(CAP)
    return env


def left_behind(env, steps=None):
    """everything a launch leaves, as bytes: records + summary rows + side tables, status, episode counts, the rollout log"""
    st = env.status()
    parts = dict(state=env.clone_state(), summary=env.summary(), flags=st["flags"], decisions=st["decisions"], now=st["now"],
                 episodes=env.episodes())
    if steps is not None:
        parts["steps"] = steps
    if getattr(env, "_rollout_route", None) is not None:
        parts.update(zip(("log_task", "log_arrival", "log_len"), env.rollout_routes()))
    if getattr(env, "_retlog", None) is not None:
        parts["ring"] = env._retlog
    return {k: np.ascontiguousarray(v.cpu().numpy()).copy() for k, v in parts.items()}


def assert_same(got, ref, tag, skip=()):
    assert sorted(got) == sorted(ref), tag
    for k in ref:
        if k not in skip:
            assert got[k].dtype == ref[k].dtype and got[k].shape == ref[k].shape and got[k].tobytes() == ref[k].tobytes(), f"{tag}: {k}"


def assert_same_episode(got, want, tag):
    """the last episode of two handles: summary rows, flags, clocks and the rollout log -- its lengths and the entries in front of them
    (an env zeroes its lengths at a restart and leaves the previous episode's entries behind them)"""
    for k in ("summary", "flags", "now", "log_len"):
        assert got[k].tobytes() == want[k].tobytes(), (tag, k)
    assert int(want["log_len"].max()) <= CAP
    live = np.arange(CAP)[None, None, :] < want["log_len"][:, :, None]
    for k in ("log_task", "log_arrival"):
        assert got[k][live].tobytes() == want[k][live].tobytes(), (tag, k)


def assert_is_the_walk(env, steps, b, w, tag):
    """env b after one whole lookahead episode against its walk: summary row, decisions, flags, steps and the rollout log"""
    sm, st = env.summary().cpu().numpy(), {k: v.cpu().numpy() for k, v in env.status().items()}
    O.assert_summary(sm[b], w["result"], f"{tag} env {b}")
    assert int(st["decisions"][b]) == w["n_steps"] == int(steps[b]), (tag, b, int(st["decisions"][b]), w["n_steps"], int(steps[b]))
    assert int(st["flags"][b]) == w["flags"], (tag, b, int(st["flags"][b]), w["flags"])
    O.assert_log(O.log(env), b, LP.Episode(w), tag)


# ---------------------------------------------------------------------------------------------------- 1. against the oracle walker
@pytest.mark.parametrize("policy", ["nearest", "first"])
@pytest.mark.parametrize("name", list(LP.TINY))
def test_against_the_oracle_walker(gpu_device, oracle_lib, name, policy):
    A, T, B, _ = LP.TINY[name]
    inst, seeds = LP.instances(name)
    env = make(gpu_device, B, A, T, inst)
    env.reset(seeds, observe=False)
    steps = env.rollout(policy, episodes=1, write_obs=False, lookahead=True).cpu().numpy()
    for b, w in enumerate(LP.walks(name, policy)):
        assert_is_the_walk(env, steps, b, w, f"{name} {policy}")
    assert (env.episodes().cpu().numpy() == 1).all()
    env.close()


# ---------------------------------------------------------------------------------------------------- 2. against Lookahead.plan()
PLAN_CASES = {"20A50T": (20, 50, 2, {}, "nearest"), "12A70T-multi-chunk": (12, 70, 2, {}, "nearest"),
              "10A20T-wide": (10, 20, 2, dict(member_cap=16), "nearest"), "10A20T-random": (10, 20, 2, {}, "random")}


@pytest.mark.parametrize("case", list(PLAN_CASES))
def test_against_the_host_driven_plan(gpu_device, case):
    from dcmrta_amd.choice import env_seeds
    from dcmrta_amd.instances import generate_batch
    from dcmrta_amd.lookahead import Lookahead
    A, T, B, kw, policy = PLAN_CASES[case]
    inst, seeds = generate_batch(B, A, T, base_seed=LP.INST_SEED + 7 * A + T), env_seeds(LP.CHOICE_SEED + 2, 0, B)
    host = make(gpu_device, B, A, T, inst, log=False, **kw).enable_route_log(CAP)
    host.reset(seeds, observe=False)
    la = Lookahead(host, policy)
    la.plan()
    dev = make(gpu_device, B, A, T, inst, **kw)
    dev.reset(seeds, observe=False)
    steps = dev.rollout(policy, episodes=1, write_obs=False, lookahead=True).cpu().numpy()
    want, got = left_behind(host), left_behind(dev)
    assert (want["flags"] & 1).all() and np.array_equal(steps, want["decisions"])
    for k in want:                                                              # records, summary rows, side tables, status, episode counts
        assert got[k].tobytes() == want[k].tobytes(), (case, k)
    for k, h, d in zip(("task", "arrival", "len"), host.routes(), dev.rollout_routes()):   # rollout log against route log
        assert h.cpu().numpy().tobytes() == d.cpu().numpy().tobytes(), (case, k)
    assert int(got["log_len"].max()) <= CAP
    la.close(); host.close(); dev.close()


# ---------------------------------------------------------------------------------------------------- 3. a ragged loaded batch
def test_a_ragged_loaded_batch_plays_each_env_at_its_own_sizes(gpu_device, oracle_lib):
    _, A, T, sizes = LP.RAGGED
    inst, seeds = LP.ragged_instances()
    env = make(gpu_device, len(sizes), A, T, inst)
    env.reset(seeds, observe=False)
    steps = env.rollout("nearest", episodes=1, lookahead=True).cpu().numpy()
    for b, w in enumerate(LP.ragged_walks()):
        assert_is_the_walk(env, steps, b, w, "ragged")
    env.close()


# ---------------------------------------------------------------------------------------------------- 4. nothing leaks
def test_the_inner_episodes_leave_nothing_behind(gpu_device, oracle_lib):
    import torch
    from dcmrta_amd.batched_env import BatchedTaskEnv
    name, policy = "10A20T", "nearest"
    A, T, B, _ = LP.TINY[name]
    inst, seeds = LP.instances(name)
    walks = LP.walks(name, policy)
    env = make(gpu_device, B, A, T, inst)
    ring = env.enable_return_log(3)
    env.reset(seeds, observe=False)
    steps = env.rollout(policy, episodes=1, write_obs=True, lookahead=True).cpu().numpy()
    ring = ring.cpu().numpy()
    ab = env.abandoned_counts().cpu().numpy()
    obs = env.obs()
    agents, tasks, mask = obs.agents.cpu().numpy(), obs.tasks.cpu().numpy(), obs.mask.cpu().numpy()
    assert (env.episodes().cpu().numpy() == 1).all()
    for b, w in enumerate(walks):
        assert_is_the_walk(env, steps, b, w, "leaks")
        # one entry per OUTER episode: the episode's reward in column 0, the others untouched
        assert ring[b, 0] == w["result"]["reward"] and np.isnan(ring[b, 1:]).all(), (b, ring[b])
        want = np.zeros((A, T), np.int16)
        for t in range(T):
            for a in w["o"].abandoned(t):
                want[a, t] += 1
        assert np.array_equal(ab[b], want), (b, "abandonment counts")
        # the observation buffers hold what the last OUTER decision saw: a second handle replays the plan's decisions up to it
        twin = BatchedTaskEnv(1, A, T, device=gpu_device).load_instances(**{k: v[b:b + 1] for k, v in inst.items()})
        twin.reset(seeds[b:b + 1], observe=False)
        for d in range(w["n_steps"] - 1):
            twin.step(torch.tensor([int(w["action"][d])], dtype=torch.int32, device=gpu_device), observe=False)
        o = twin.observe()
        assert int(o.leader[0]) == int(w["leader"][-1])
        assert np.array_equal(o.agents.cpu().numpy()[0].view(np.uint32), agents[b].view(np.uint32)), (b, "agent rows")
        assert np.array_equal(o.tasks.cpu().numpy()[0].view(np.uint32), tasks[b].view(np.uint32)), (b, "task rows")
        assert np.array_equal(o.mask.cpu().numpy()[0], mask[b]) and np.array_equal(mask[b].astype(np.uint8), w["mask"][-1]), (b, "mask")
        twin.close()
    env.close()


# ---------------------------------------------------------------------------------------------------- 5. budgets
@pytest.mark.parametrize("budget", [7, (0, 5)], ids=["scalar", "per-env-with-0"])
def test_a_budget_stop_and_the_rest_leave_what_one_launch_leaves(gpu_device, budget):
    name, policy = "10A20T", "nearest"
    A, T, B, _ = LP.TINY[name]
    inst, seeds = LP.instances(name)
    whole = make(gpu_device, B, A, T, inst)
    whole.reset(seeds, observe=False)
    ref = left_behind(whole, whole.rollout(policy, episodes=1, lookahead=True))
    parts = make(gpu_device, B, A, T, inst)
    parts.reset(seeds, observe=False)
    fresh = left_behind(parts)
    first = parts.rollout(policy, episodes=1, lookahead=True, max_decisions=budget if isinstance(budget, int) else np.array(budget, np.int64))
    mid = left_behind(parts)
    want_first = np.full(B, budget) if isinstance(budget, int) else np.array(budget)
    assert np.array_equal(first.cpu().numpy(), want_first) and np.array_equal(mid["decisions"], want_first) and not (mid["flags"] & 1).any()
    rec = parts.record_bytes()
    for b in np.flatnonzero(want_first == 0):                                   # no budget: the env's bytes are unchanged
        assert mid["state"][b * rec:(b + 1) * rec].tobytes() == fresh["state"][b * rec:(b + 1) * rec].tobytes(), b
        assert mid["summary"][b].tobytes() == fresh["summary"][b].tobytes() and (mid["log_len"][b] == 0).all(), b
    rest = parts.rollout(policy, episodes=1, lookahead=True)
    assert_same(left_behind(parts, first + rest), ref, f"budget {budget}")
    # ... and the observation buffers, which hold the last decision taken either way
    for k in ("agents", "tasks", "mask"):
        assert getattr(whole.obs(), k).cpu().numpy().tobytes() == getattr(parts.obs(), k).cpu().numpy().tobytes(), k
    whole.close(); parts.close()


# ---------------------------------------------------------------------------------------------------- 6. two episodes
def test_two_episodes_in_one_call_are_two_calls_and_the_second_is_the_shifted_seeds_first(gpu_device):
    name, policy = "10A20T", "nearest"
    A, T, B, _ = LP.TINY[name]
    inst, seeds = LP.instances(name)
    one = make(gpu_device, B, A, T, inst)
    one.enable_return_log(2)
    one.reset(seeds, observe=False)
    steps = one.rollout(policy, episodes=2, write_obs=False, lookahead=True)
    two = make(gpu_device, B, A, T, inst)
    two.enable_return_log(2)
    two.reset(seeds, observe=False)
    n1 = two.rollout(policy, episodes=1, write_obs=False, lookahead=True)
    n2 = two.rollout(policy, episodes=1, write_obs=False, lookahead=True)
    got = left_behind(one, steps)
    assert_same(got, left_behind(two, n1 + n2), "episodes=2 against two calls")
    assert (got["episodes"] == 2).all() and not np.isnan(got["ring"]).any()
    # the second episode is the first episode of a fresh handle under the shifted seeds
    n1 = n1.cpu().numpy()
    fresh = make(gpu_device, B, A, T, inst)
    fresh.reset(np.array([LP.shifted_seed(seeds[b], n1[b]) for b in range(B)], np.uint64), observe=False)
    n = fresh.rollout(policy, episodes=1, write_obs=False, lookahead=True)
    want = left_behind(fresh)
    assert np.array_equal(n.cpu().numpy(), n2.cpu().numpy())
    assert_same_episode(got, want, "second episode")
    assert np.array_equal(got["ring"][:, 1], want["summary"][:, 0])
    one.close(); two.close(); fresh.close()


# ---------------------------------------------------------------------------------------------------- 7. renewal
def test_renewal_draws_the_next_instance_at_the_outer_restart(gpu_device):
    from dcmrta_amd.batched_env import BatchedTaskEnv
    from dcmrta_amd.choice import env_seeds
    A, T, B, policy, stride = 10, 20, 3, "nearest", 100
    inst_seeds, seeds = np.arange(900, 900 + B, dtype=np.uint64), env_seeds(LP.CHOICE_SEED + 3, 0, B)

    def handle(s, renew):
        env = BatchedTaskEnv(B, A, T, device=gpu_device)
        env.generate_instances(s)
        if renew:
            env.set_instance_renewal(stride)
        env.enable_rollout_log(CAP)
        return env
    renewing = handle(inst_seeds, True)
    renewing.reset(seeds, observe=False)
    steps = renewing.rollout(policy, episodes=2, write_obs=False, lookahead=True).cpu().numpy()
    assert (renewing.instance_index().cpu().numpy() == 1).all() and (renewing.episodes().cpu().numpy() == 2).all()
    first = handle(inst_seeds, False)                                           # the first episode alone: its decisions
    first.reset(seeds, observe=False)
    n1 = first.rollout(policy, episodes=1, write_obs=False, lookahead=True).cpu().numpy()
    second = handle(inst_seeds + np.uint64(stride), False)                      # a fresh non-renewing handle on the next instances
    second.reset(np.array([LP.shifted_seed(seeds[b], n1[b]) for b in range(B)], np.uint64), observe=False)
    n2 = second.rollout(policy, episodes=1, write_obs=False, lookahead=True).cpu().numpy()
    assert np.array_equal(steps, n1 + n2)
    got, want = left_behind(renewing), left_behind(second)
    assert_same_episode(got, want, "renewed episode")
    renewing.close(); first.close(); second.close()


# ---------------------------------------------------------------------------------------------------- 8. refusals
def _raw(env, policy, episodes=1, budget=-1):
    import torch
    from dcmrta_amd.batched_env import _ptr
    steps = torch.full((env.B,), -7, dtype=torch.int64, device=env.device)
    with torch.cuda.device(env.device):
        rc = env._lib.dcm_rollout_lookahead(env._h, policy, episodes, budget, None, None, None, None, _ptr(steps), env._stream())
    return rc, env._lib.dcm_last_error(), steps.cpu().numpy()


def test_refusals_leave_the_state_alone(gpu_device):
    from dcmrta_amd._lib import DcmError
    from dcmrta_amd.batched_env import BatchedTaskEnv
    name = "5A8T"
    A, T, B, _ = LP.TINY[name]
    inst, seeds = LP.instances(name)

    def refused(env, status, word, **kw):
        before = env.clone_state().cpu().numpy().copy()
        rc, err, steps = _raw(env, **kw)
        assert rc == status and err.startswith(b"dcm_rollout_lookahead:") and word in err and (steps == -7).all(), (kw, rc, err)
        assert np.array_equal(env.clone_state().cpu().numpy(), before), kw
    env = make(gpu_device, B, A, T, inst)
    refused(env, ERR_STATE, b"dcm_reset", policy=2)                             # no dcm_reset yet
    env.reset(seeds, observe=False)
    for policy in (-1, 3, 7):
        refused(env, ERR_INVALID, b"base policy", policy=policy)
    for episodes in (0, -2):
        refused(env, ERR_INVALID, b"episodes", policy=2, episodes=episodes)
    env.enable_best_log()
    refused(env, ERR_STATE, b"best log", policy=2)
    env.enable_best_log(False)
    with pytest.raises(DcmError, match="cannot be combined with explore"):
        env.rollout("nearest", lookahead=True, explore=0.5)
    assert _raw(env, 1)[0] == 0                                                 # ... and then it runs
    env.close()
    # max_waiting_time <= 0: with a budget too
    env = make(gpu_device, B, A, T, inst, max_waiting_time=0.0)
    env.reset(seeds, observe=False)
    refused(env, ERR_INVALID, b"max_waiting_time <= 0", policy=2)
    refused(env, ERR_INVALID, b"max_waiting_time <= 0", policy=2, budget=5)
    env.close()
    # a launch that would be size-renewing
    env = BatchedTaskEnv(4, 20, 50, device=gpu_device, renew_sizes=True)
    env.generate_instances(np.arange(300, 304, dtype=np.uint64), agents_range=(10, 20), tasks_range=(20, 50))
    env.set_instance_renewal(4)
    env.reset(5, observe=False)
    refused(env, ERR_STATE, b"renews its sizes", policy=2, episodes=2)
    env.close()
