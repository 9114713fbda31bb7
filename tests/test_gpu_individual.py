"""-m gpu: the persistent rollout under individual selection (dcm_rollout_individual; BatchedTaskEnv.rollout(policy, individual=True);
the kernels k_is_rollout_random / k_isrn_rollout_random).  The yardstick is the reference's Worker.run_test_IS loop on the oracle's
step-wise surface (individual_ref.walk), matched bit for bit; test_individual_ref_host.py shows on the oracle alone that no case here
can be passed by a kernel that groups the deciders by location."""
import numpy as np
import pytest

import helpers as H
import individual_ref as IS
import oracle_ref as O

pytestmark = pytest.mark.gpu

ERR_INVALID, ERR_STATE = -1, -4
CAP = 64


def make(gpu_device, name, log=True, **more):
    from dcmrta_amd.batched_env import BatchedTaskEnv
    c = IS.ALL[name]
    inst, seeds = IS.instances(name)
    env = BatchedTaskEnv(c["B"], c["A"], c["T"], device=gpu_device, **{**IS.handle_kw(name), **more}).load_instances(**inst)
    if log:
        env.enable_rollout_log(CAP)
    return env, seeds


def launch(env, policy, q32=0, **kw):
    return env.rollout(policy, individual=True, **({"explore_q32": q32} if q32 else {}), **kw).cpu().numpy()


def left_behind(env, steps=None):
    """everything a launch leaves, as bytes: records + summary rows + side tables, status, episode counts, the rollout log"""
    st = env.status()
    parts = dict(state=env.clone_state(), summary=env.summary(), flags=st["flags"], decisions=st["decisions"], now=st["now"],
                 episodes=env.episodes())
    if steps is not None:
        parts["steps"] = steps
    if getattr(env, "_rollout_route", None) is not None:
        parts.update(zip(("log_task", "log_arrival", "log_len"), env.rollout_routes()))
    return {k: np.ascontiguousarray(v if isinstance(v, np.ndarray) else v.cpu().numpy()).copy() for k, v in parts.items()}


def assert_same(got, ref, tag):
    assert sorted(got) == sorted(ref), tag
    for k in ref:
        assert got[k].dtype == ref[k].dtype and got[k].shape == ref[k].shape and got[k].tobytes() == ref[k].tobytes(), f"{tag}: {k}"


def assert_is_the_walk(env, b, w, tag, decisions=None, fin=None, log=True):
    """env b after the whole episode `w`: summary row, every getter, flags, the decision counter, and the rollout log"""
    f = IS.final(w)
    fin = fin if fin is not None else H.gpu_final(env)
    O.assert_summary(env.summary().cpu().numpy()[b], f, f"{tag} env{b}")
    a, t = w["a"], w["o"].T
    got = {k: (v[:t] if k in ("finished", "feasible", "time_start", "time_finish", "task_wait", "n_members", "n_abandoned") else
               v[:a] if k in ("travel_dist", "returned", "agent_wait") else v) for k, v in fin[b].items()}
    H.assert_final_matches(got, f, f"{tag} env{b}")
    assert fin[b]["flags"] & 7 == f["flags"], (tag, b, fin[b]["flags"], f["flags"])
    if decisions is not None:
        assert int(env.status()["decisions"][b]) == decisions, (tag, b)
    if log:
        O.assert_log(O.log(env), b, IS.Episode(w), tag)


def assert_obs(env, b, w, tag):
    """the observation buffers hold what the last deciding agent saw; rows beyond the env's own sizes are padding (-1, mask 1)"""
    o = env.obs()
    agents, tasks, mask = o.agents.cpu().numpy()[b], o.tasks.cpu().numpy()[b], o.mask.cpu().numpy()[b].astype(np.uint8)
    m, tk, ag = w["obs"]
    a, t = ag.shape[0], tk.shape[0] - 1
    assert np.array_equal(mask[:t + 1], m), (tag, b, "mask")
    assert np.array_equal(tasks[:t + 1].view(np.uint32), tk.view(np.uint32)), (tag, b, "task rows")
    assert np.array_equal(agents[:a].view(np.uint32), ag.view(np.uint32)), (tag, b, "agent rows")
    assert (agents[a:] == -1).all() and (tasks[t + 1:] == -1).all() and (mask[t + 1:] == 1).all(), (tag, b, "padding rows")


def first_valid(obs):
    import torch
    return torch.argmax((~obs.mask.bool()).to(torch.int32), dim=1).to(torch.int32)   # the lowest unmasked action: `first`


def lockstep(env, obs, limit=None):
    """step() with `first`'s action until every env is inactive, or `limit` times; the flagged handle takes the lowest pending id"""
    n = 0
    while bool(obs.active.any()) and (limit is None or n < limit):
        obs = env.step(first_valid(obs))
        n += 1
        assert n < 5000
    return obs


# ---------------------------------------------------------------------------------------------------- 1. the policies on every case
@pytest.mark.parametrize("policy,q32", IS.POLICIES, ids=["random", "first", "nearest", "nearest-eps0.25"])
@pytest.mark.parametrize("name", list(IS.CASES))
def test_policies_against_the_oracle_walk(gpu_device, oracle_lib, name, policy, q32):
    env, seeds = make(gpu_device, name)
    env.reset(seeds, observe=False)
    steps = launch(env, policy, q32)
    fin = H.gpu_final(env)
    for b, eps in enumerate(IS.walks(name, policy, q32)):
        w = eps[0]
        assert int(steps[b]) == w["n_steps"], (name, policy, b, int(steps[b]), w["n_steps"])
        assert_is_the_walk(env, b, w, f"{name} {policy}", decisions=w["n_steps"], fin=fin)
        assert_obs(env, b, w, f"{name} {policy}")
    assert (env.episodes().cpu().numpy() == 1).all()
    env.close()


# ---------------------------------------------------------------------------------------------------- 2. the ends of explore_q32
@pytest.mark.parametrize("name", ["6A12T", "50A200T"])
def test_the_endpoints_of_explore_q32(gpu_device, name):
    def played(policy, **kw):
        env, seeds = make(gpu_device, name)
        env.reset(seeds, observe=False)
        out = left_behind(env, env.rollout(policy, individual=True, **kw))
        env.close()
        return out
    for policy in ("first", "nearest"):
        assert_same(played(policy, explore_q32=0), played(policy), f"{name} {policy} explore_q32 = 0")
        assert_same(played(policy, explore_q32=1 << 32), played("random"), f"{name} {policy} explore_q32 = 2^32")
        assert_same(played(policy, explore=1.0), played("random"), f"{name} {policy} explore = 1.0")


# ---------------------------------------------------------------------------------------------------- 3. hand-over
@pytest.mark.parametrize("name", ["6A12T", "50A200T"])
def test_a_stopped_launch_is_carried_on_by_step(gpu_device, oracle_lib, name):
    c = IS.ALL[name]
    walks = [eps[0] for eps in IS.walks(name, "first")]
    ks = np.array([IS.mid_event_stop(w, c["A"]) for w in walks], np.int64)    # behind the first event, in the middle of a later one
    env, seeds = make(gpu_device, name, log=False)
    env.reset(seeds, observe=False)
    steps = launch(env, "first", max_decisions=ks)
    st = env.status()
    assert np.array_equal(steps, ks) and np.array_equal(st["decisions"].cpu().numpy(), ks) and not (st["flags"].cpu().numpy() & 1).any()
    pg = env.agents_state()["pending_group"].cpu().numpy()
    for b, w in enumerate(walks):                                              # the rest of the event is still pending, lowest id next
        ev = w["event"]
        rest = w["decider"][ks[b]:][ev[ks[b]:] == ev[ks[b]]]
        assert np.array_equal(np.flatnonzero(pg[b] > 0), rest), (name, b)
    obs = env.observe()
    assert np.array_equal(obs.leader.cpu().numpy(), [w["decider"][k] for w, k in zip(walks, ks)])
    lockstep(env, obs)
    for b, w in enumerate(walks):
        assert_is_the_walk(env, b, w, f"{name} launch then step", decisions=w["n_steps"], log=False)
    env.close()


@pytest.mark.parametrize("name", ["6A12T", "50A200T"])
def test_a_launch_carries_on_after_lockstep_steps(gpu_device, oracle_lib, name):
    c = IS.ALL[name]
    walks = [eps[0] for eps in IS.walks(name, "first")]
    k = c["A"] + 3
    assert all(w["n_steps"] > k + 1 for w in walks)
    env, seeds = make(gpu_device, name, log=False)
    lockstep(env, env.reset(seeds), limit=k)
    assert (env.status()["decisions"].cpu().numpy() == k).all()
    steps = launch(env, "first")
    for b, w in enumerate(walks):
        assert int(steps[b]) == w["n_steps"] - k
        assert_is_the_walk(env, b, w, f"{name} step then launch", decisions=w["n_steps"], log=False)
        assert_obs(env, b, w, f"{name} step then launch")
    env.close()


@pytest.mark.parametrize("name", ["6A12T", "50A200T"])
def test_per_env_budgets(gpu_device, oracle_lib, name):
    """max_decisions_in with one entry 0 (the env takes no decision) and one negative (no limit); the rest by a second launch"""
    c = IS.ALL[name]
    walks = [eps[0] for eps in IS.walks(name, "nearest")]
    budget = np.array([0, -1, 5, 9][:c["B"]], np.int64)
    env, seeds = make(gpu_device, name)
    env.reset(seeds, observe=False)
    fresh = left_behind(env)
    first = launch(env, "nearest", max_decisions=budget)
    mid = left_behind(env)
    want = np.array([w["n_steps"] if x < 0 else x for w, x in zip(walks, budget)])
    assert np.array_equal(first, want) and np.array_equal(mid["decisions"], want)
    rec = env.record_bytes()
    assert mid["state"][:rec].tobytes() == fresh["state"][:rec].tobytes() and (mid["log_len"][0] == 0).all()   # budget 0: untouched
    assert_is_the_walk(env, 1, walks[1], f"{name} no limit", decisions=walks[1]["n_steps"])
    rest = launch(env, "nearest", max_decisions=np.where(budget < 0, 0, -1))   # (a finished env would restart: budget 0 keeps its results)
    assert rest[1] == 0
    for b, w in enumerate(walks):
        assert int(first[b] + rest[b]) == w["n_steps"]
        assert_is_the_walk(env, b, w, f"{name} budgets", decisions=w["n_steps"])
    env.close()


# ---------------------------------------------------------------------------------------------------- 4. two episodes in one launch
def assert_two_episodes(env, ring, steps, chains, tag):
    ring, fin = ring.cpu().numpy(), H.gpu_final(env)
    for b, (e0, e1) in enumerate(chains):
        assert int(steps[b]) == e0["n_steps"] + e1["n_steps"], (tag, b)
        assert ring[b, 0] == IS.final(e0)["reward"] and ring[b, 1] == IS.final(e1)["reward"], (tag, b, ring[b])
        assert_is_the_walk(env, b, e1, tag, decisions=e0["n_steps"] + e1["n_steps"], fin=fin)
        assert_obs(env, b, e1, tag)
    assert (env.episodes().cpu().numpy() == 2).all()


@pytest.mark.parametrize("policy,q32", [("random", 0), ("nearest", IS.Q25)], ids=["random", "nearest-eps0.25"])
def test_two_episodes_of_a_ragged_batch(gpu_device, oracle_lib, policy, q32):
    from dcmrta_amd.batched_env import BatchedTaskEnv
    inst, seeds = IS.ragged_instances()
    env = BatchedTaskEnv(len(seeds), IS.RAGGED["A"], IS.RAGGED["T"], device=gpu_device, individual_selection=True).load_instances(**inst)
    env.enable_rollout_log(CAP)
    ring = env.enable_return_log(2)
    env.reset(seeds, observe=False)
    steps = launch(env, policy, q32, episodes=2)
    assert_two_episodes(env, ring, steps, IS.ragged_walks(policy, q32), f"ragged {policy}")
    env.close()


@pytest.mark.parametrize("policy,q32", [("random", 0), ("nearest", IS.Q25)], ids=["random", "nearest-eps0.25"])
def test_two_episodes_of_a_renewing_launch(gpu_device, oracle_lib, policy, q32):
    from dcmrta_amd.batched_env import BatchedTaskEnv
    c = IS.RENEWING
    inst_seeds, seeds, chains = IS.renewing_walks(policy, q32)
    env = BatchedTaskEnv(c["B"], c["A"], c["T"], device=gpu_device, individual_selection=True)
    env.generate_instances(inst_seeds)
    env.set_instance_renewal(c["stride"])
    env.enable_rollout_log(CAP)
    ring = env.enable_return_log(2)
    env.reset(seeds, observe=False)
    steps = launch(env, policy, q32, episodes=2)
    assert (env.instance_index().cpu().numpy() == 1).all()
    assert_two_episodes(env, ring, steps, chains, f"renewing {policy}")
    env.close()


# ---------------------------------------------------------------------------------------------------- 5. a short waiting time
@pytest.mark.parametrize("name", list(IS.SHORT_WAIT))
def test_abandonments_under_a_short_waiting_time(gpu_device, oracle_lib, name):
    env, seeds = make(gpu_device, name)
    env.reset(seeds, observe=False)
    steps = launch(env, "random")
    ab, fin = env.abandoned_counts().cpu().numpy(), H.gpu_final(env)
    for b, eps in enumerate(IS.walks(name, "random")):
        w = eps[0]
        assert int(steps[b]) == w["n_steps"] and IS.final(w)["abandonments"] > 0
        assert_is_the_walk(env, b, w, name, decisions=w["n_steps"], fin=fin)
        assert np.array_equal(ab[b], IS.abandoned_counts(w)), (name, b, "abandonment counts")
    env.close()


# ---------------------------------------------------------------------------------------------------- 6. refusals
def _raw(env, policy=2, q32=0, episodes=1, budget=-1):
    import torch
    from dcmrta_amd.batched_env import _ptr
    steps = torch.full((env.B,), -7, dtype=torch.int64, device=env.device)
    with torch.cuda.device(env.device):
        rc = env._lib.dcm_rollout_individual(env._h, policy, q32, episodes, budget, None, None, None, None, _ptr(steps), env._stream())
    return rc, env._lib.dcm_last_error(), steps.cpu().numpy()


def test_refusals_leave_the_state_alone(gpu_device):
    from dcmrta_amd._lib import DcmError
    from dcmrta_amd.batched_env import BatchedTaskEnv
    name = "6A12T"

    def refused(env, status, word, **kw):
        before = env.clone_state().cpu().numpy().copy()
        rc, err, steps = _raw(env, **kw)
        assert rc == status and err.startswith(b"dcm_rollout_individual:") and word in err and (steps == -7).all(), (kw, rc, err)
        assert np.array_equal(env.clone_state().cpu().numpy(), before), kw
    env, seeds = make(gpu_device, name)
    refused(env, ERR_STATE, b"dcm_reset")                                       # no dcm_reset yet
    env.reset(seeds, observe=False)
    for policy in (-1, 3, 7):
        refused(env, ERR_INVALID, b"unknown policy", policy=policy)
    refused(env, ERR_INVALID, b"explore_q32", q32=(1 << 32) + 1)
    refused(env, ERR_INVALID, b"DCM_POLICY_RANDOM", policy=0, q32=1)
    for episodes in (0, -2):
        refused(env, ERR_INVALID, b"episodes", episodes=episodes)
    env.enable_best_log()
    refused(env, ERR_STATE, b"best log")
    env.enable_best_log(False)
    with pytest.raises(DcmError, match="no lookahead form"):
        env.rollout("nearest", individual=True, lookahead=True)
    assert _raw(env)[0] == 0 and _raw(env, q32=1 << 32)[0] == 0 and _raw(env, policy=0)[0] == 0      # ... and then it runs
    env.close()
    # a handle without DCM_PARAM_NO_GROUPING
    env, seeds = make(gpu_device, name, individual_selection=False)
    env.reset(seeds, observe=False)
    refused(env, ERR_STATE, b"DCM_PARAM_NO_GROUPING")
    with pytest.raises(DcmError, match="individual_selection=True"):
        env.rollout("nearest", individual=True)
    env.close()
    # max_waiting_time <= 0: a greedy policy needs a budget, the random one does not
    env, seeds = make(gpu_device, name, max_waiting_time=0.0)
    env.reset(seeds, observe=False)
    refused(env, ERR_INVALID, b"max_waiting_time <= 0", policy=1)
    refused(env, ERR_INVALID, b"max_waiting_time <= 0", policy=2, q32=5)
    assert _raw(env, policy=1, budget=5)[0] == 0 and _raw(env, policy=0, budget=5)[0] == 0
    env.close()
    # a launch that would be size-renewing
    env = BatchedTaskEnv(4, 20, 50, device=gpu_device, renew_sizes=True, individual_selection=True)
    env.generate_instances(np.arange(300, 304, dtype=np.uint64), agents_range=(10, 20), tasks_range=(20, 50))
    env.set_instance_renewal(4)
    env.reset(5, observe=False)
    refused(env, ERR_STATE, b"renews its sizes", episodes=2)
    env.close()


# ---------------------------------------------------------------------------------------------------- 7. nothing leaks
@pytest.mark.parametrize("name", ["20A50T", "50A200T"])
def test_the_grouped_launches_of_a_flagged_handle_are_what_they_were(gpu_device, name):
    """grouped launch -> restore_state -> individual launch -> restore_state -> grouped launch: the last leaves the first's bytes, and
    the individual launch between them leaves others"""
    from dcmrta_amd.batched_env import BatchedTaskEnv
    c = IS.ALL[name]
    env, seeds = make(gpu_device, name)
    env.reset(seeds, observe=False)
    start = env.clone_state()

    def played(**kw):
        env.restore_state(start)
        env.enable_rollout_log(CAP)                                             # fresh buffers: lengths 0, as behind reset()
        return left_behind(env, env.rollout("nearest", **kw))
    before, between, after = played(), played(individual=True), played()
    assert_same(after, before, f"{name} grouped launch again")
    assert before["state"].tobytes() != between["state"].tobytes() and (between["flags"] & 1).all()
    plain = BatchedTaskEnv(c["B"], c["A"], c["T"], device=gpu_device, max_waiting_time=c["mwt"], max_time=c["max_time"])
    for entry in ("rollout", "step"):
        assert env.kernel_name(entry) == plain.kernel_name(entry)
    assert name != "20A50T" or (env.kernel_name("rollout"), env.kernel_name("step")) == ("k_rollout_fast", "k_step_fast")
    env.close(); plain.close()
