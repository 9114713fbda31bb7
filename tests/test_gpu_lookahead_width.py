"""-m gpu: the width-limited device lookahead (dcm_rollout_lookahead_width; BatchedTaskEnv.rollout(policy, lookahead=True, width=W,
return_inner=True); the kernels k_la_rollout_random / k_larn_rollout_random with their `width` and `inner_out` arguments).

The yardstick is the step-wise oracle walker under the rule of include/dcmrta_env.h (lookahead_width_ref.py), matched bit for bit:
steps, the rollout log, the summary row, flags, the decision counter, and inner_out against the walker's own count.  Width 1 must be the
`nearest` launch and width 0 / width >= T the dcm_rollout_lookahead launch, byte for byte.  tests/test_lookahead_width_ref_host.py
proves from the oracle alone what each case meets."""
import numpy as np
import pytest

import lookahead_policy_ref as LP
import lookahead_width_ref as LW
import oracle_ref as O

pytestmark = pytest.mark.gpu

ERR_INVALID, ERR_STATE = -1, -4
CAP = 64
POLICIES = ["random", "first", "nearest"]
TASK_KEYS = ("n_members", "n_abandoned", "feasible", "finished", "time_start", "time_finish")


def make(gpu_device, B, A, T, inst, **kw):
    from dcmrta_amd.batched_env import BatchedTaskEnv
    return BatchedTaskEnv(B, A, T, device=gpu_device, **kw).load_instances(**inst).enable_rollout_log(CAP)


def left_behind(env, steps=None, obs=True):
    """everything a launch leaves, as bytes: records + summary rows + side tables (the dcm_clone_state blob), the summary, status,
    episode counts, the observation buffers (obs: the launch wrote them) and the rollout log"""
    st = env.status()
    parts = dict(state=env.clone_state(), summary=env.summary(), flags=st["flags"], decisions=st["decisions"], now=st["now"],
                 episodes=env.episodes())
    if obs:
        o = env.obs()
        parts.update(agents=o.agents, tasks=o.tasks, mask=o.mask)
    if steps is not None:
        parts["steps"] = steps
    parts.update(zip(("log_task", "log_arrival", "log_len"), env.rollout_routes()))
    return {k: np.ascontiguousarray(v.cpu().numpy()).copy() for k, v in parts.items()}


def assert_same(got, ref, tag):
    assert sorted(got) == sorted(ref), tag
    for k in ref:
        assert got[k].dtype == ref[k].dtype and got[k].shape == ref[k].shape and got[k].tobytes() == ref[k].tobytes(), f"{tag}: {k}"


def assert_is_the_walk(env, steps, inner, b, w, tag):
    """env b after one whole width-limited episode against its walk: summary row, decisions, flags, steps, the log and inner_out"""
    sm, st = env.summary().cpu().numpy(), {k: v.cpu().numpy() for k, v in env.status().items()}
    print(f"{tag} env {b}: steps {int(steps[b])} / {w['n_steps']}, inner {int(inner[b])} / {w['inner']}, reward {sm[b, 0]!r} / {w['result']['reward']!r}")
    assert int(st["decisions"][b]) == w["n_steps"] == int(steps[b]), (tag, b, int(st["decisions"][b]), w["n_steps"], int(steps[b]))
    O.assert_summary(sm[b], w["result"], f"{tag} env {b}")
    assert int(st["flags"][b]) == w["flags"], (tag, b, int(st["flags"][b]), w["flags"])
    O.assert_log(O.log(env), b, LP.Episode(w), tag)
    assert int(inner[b]) == w["inner"], (tag, b, "inner_out", int(inner[b]), w["inner"])


def raw(env, policy, width=0, episodes=1, budget=-1, old=False, want_inner=True):
    """the C entry itself -- dcm_rollout_lookahead (old) or dcm_rollout_lookahead_width -- with sentinels in steps_out and inner_out"""
    import torch
    from dcmrta_amd.batched_env import _ptr
    steps = torch.full((env.B,), -7, dtype=torch.int64, device=env.device)
    inner = torch.full((env.B,), -9, dtype=torch.int64, device=env.device)
    with torch.cuda.device(env.device):
        if old:
            rc = env._lib.dcm_rollout_lookahead(env._h, policy, episodes, budget, None, None, None, None, _ptr(steps), env._stream())
        else:
            rc = env._lib.dcm_rollout_lookahead_width(env._h, policy, width, episodes, budget, None, None, None, None, _ptr(steps),
                                                      _ptr(inner) if want_inner else None, env._stream())
    return rc, env._lib.dcm_last_error(), steps.cpu().numpy(), inner.cpu().numpy()


# ---------------------------------------------------------------------------------------------------- 1. against the oracle walker
@pytest.mark.parametrize("width", [2, 3])
@pytest.mark.parametrize("policy", POLICIES)
@pytest.mark.parametrize("name", list(LP.TINY))
def test_against_the_oracle_walker(gpu_device, oracle_lib, name, policy, width):
    A, T, B, _ = LP.TINY[name]
    inst, seeds = LP.instances(name)
    env = make(gpu_device, B, A, T, inst)
    env.reset(seeds, observe=False)
    steps, inner = (x.cpu().numpy() for x in env.rollout(policy, episodes=1, write_obs=False, lookahead=True, width=width, return_inner=True))
    for b, w in enumerate(LW.walks(name, policy, width)):
        assert_is_the_walk(env, steps, inner, b, w, f"{name} {policy} width {width}")
    assert (env.episodes().cpu().numpy() == 1).all()
    env.close()


# ---------------------------------------------------------------------------------------------------- 2. width 1 is `nearest`
@pytest.mark.parametrize("policy", POLICIES)
def test_width_1_is_the_nearest_launch(gpu_device, policy):
    name = "10A20T"
    A, T, B, _ = LP.TINY[name]
    inst, seeds = LP.instances(name)
    env, twin = make(gpu_device, B, A, T, inst), make(gpu_device, B, A, T, inst)
    env.reset(seeds, observe=False)
    twin.reset(seeds, observe=False)
    steps, inner = env.rollout(policy, episodes=2, lookahead=True, width=1, return_inner=True)
    want = left_behind(twin, twin.rollout("nearest", episodes=2))
    assert_same(left_behind(env, steps), want, f"width 1 over {policy}")
    assert (want["episodes"] == 2).all() and (want["flags"] & 1).all()
    assert (inner.cpu().numpy() == 0).all(), inner
    env.close(); twin.close()


# ---------------------------------------------------------------------------------------------------- 3. width 0 and width >= T
@pytest.mark.parametrize("name,policy", [("10A20T", "nearest"), ("5A8T", "random")])
def test_width_0_and_width_beyond_the_tasks_are_the_all_actions_launch(gpu_device, oracle_lib, name, policy):
    from dcmrta_amd.batched_env import BatchedTaskEnv
    A, T, B, _ = LP.TINY[name]
    inst, seeds = LP.instances(name)
    p = BatchedTaskEnv.POLICIES[policy]

    def launch(**kw):
        env = make(gpu_device, B, A, T, inst)
        env.reset(seeds, observe=False)
        rc, err, steps, inner = raw(env, p, **kw)
        assert rc == 0, err
        left = left_behind(env, obs=False)
        left["steps"] = steps
        env.close()
        return left, inner
    old, untouched = launch(old=True)
    assert (untouched == -9).all()
    w0, inner0 = launch(width=0)
    w50, inner50 = launch(width=50)
    none, untouched = launch(width=0, want_inner=False)
    assert (untouched == -9).all()
    for tag, got in (("width 0", w0), ("width 50", w50), ("width 0, no inner_out", none)):
        assert_same(got, old, f"{name} {policy}: {tag} against dcm_rollout_lookahead")
    # ... and through rollout(): width=0 with return_inner=True is the old launch through the new entry
    env = make(gpu_device, B, A, T, inst)
    env.reset(seeds, observe=False)
    steps, inner_py = env.rollout(policy, episodes=1, write_obs=False, lookahead=True, return_inner=True)
    assert np.array_equal(steps.cpu().numpy(), old["steps"])
    env.close()
    want = np.array([w["inner"] for w in LW.walks(name, policy, 0)], np.int64)
    print(name, policy, "inner", inner0, inner50, inner_py.cpu().numpy(), "reference", want)
    assert np.array_equal(inner0, want) and np.array_equal(inner50, want) and np.array_equal(inner_py.cpu().numpy(), want)


# ---------------------------------------------------------------------------------------------------- 4. + 5. windows
def getters(env):
    ag, st = env.agents_state(), env.status()
    return dict(mem=env.task_members().cpu().numpy(), abc=env.abandoned_counts().cpu().numpy(),
                ts={k: v.cpu().numpy() for k, v in env.tasks_state().items()},
                ag={k: ag[k].cpu().numpy() for k in ("sum_waiting_time", "travel_dist", "returned")},
                st={k: v.cpu().numpy() for k, v in st.items()})


def assert_stopped(tag, got, b, a, t, s, member_cap=5):
    """env b of a handle against the oracle walker where the window ended (LP.stopped_state)"""
    st, mem, abc = got["st"], got["mem"][b], got["abc"][b]
    assert int(st["decisions"][b]) == s["decisions"] and not (st["flags"][b] & LP.DONE), (tag, "decisions / flags", st["decisions"][b], st["flags"][b])
    assert st["now"][b] == s["now"], (tag, "now", st["now"][b], s["now"])
    want = np.full((t, member_cap), -1, np.int16)
    for j, m in enumerate(s["members"]):
        want[j, :len(m)] = m
    assert np.array_equal(mem[:t], want), (tag, "members", np.flatnonzero((mem[:t] != want).any(1)))
    assert np.array_equal(abc[:a, :t], s["abc"]), (tag, "abandonment counts", np.argwhere(abc[:a, :t] != s["abc"])[:8])
    for k in TASK_KEYS:
        v = got["ts"][k][b, :t].astype(s["tasks"][k].dtype)
        assert np.array_equal(v, s["tasks"][k]), (tag, k, np.flatnonzero(v != s["tasks"][k]))
    for k, v in (("agent_wait", got["ag"]["sum_waiting_time"][b, :a]), ("travel_dist", got["ag"]["travel_dist"][b, :a]),
                 ("returned", got["ag"]["returned"][b, :a]), ("task_wait", got["ts"]["sum_waiting_time"][b, :t])):
        assert np.array_equal(v.astype(s[k].dtype), s[k]), (tag, k, np.flatnonzero(v.astype(s[k].dtype) != s[k]))


@pytest.mark.parametrize("name", list(LW.WINDOWS))
def test_a_window_of_width_limited_decisions(gpu_device, oracle_lib, name):
    """ties-*: pairs of tasks at one point, the cut of the list between two twins and both twins inside it.  The others: one window per
    form of the candidate walk (LW.SIM_KINDS)."""
    c = LW.WINDOWS[name]
    inst, seeds = LW.window_instances(name)
    ws = LW.windows(name)
    A, T, B, K, policy, width = c["A"], c["T"], c["B"], c["K"], c["policy"], c["width"]
    d0 = np.array([x["d0"] for x in ws], np.int64)
    env = make(gpu_device, B, A, T, inst, max_waiting_time=c["mwt"])
    env.reset(seeds, observe=False)
    if d0.any():
        assert np.array_equal(env.rollout(policy, episodes=1, write_obs=False, max_decisions=d0).cpu().numpy(), d0)
    steps, inner = (x.cpu().numpy() for x in env.rollout(policy, episodes=1, write_obs=False, lookahead=True, width=width, max_decisions=K,
                                                         return_inner=True))
    want_inner = np.array([x["window"]["inner"] for x in ws], np.int64)
    print(f"{name}: {LW.SIM_KINDS[name]} width {width} steps {steps} inner {inner} / {want_inner}")
    assert np.array_equal(steps, np.full(B, K)), (name, steps)
    got, log = getters(env), O.log(env)
    for b, x in enumerate(ws):
        assert_stopped(f"{name} env {b}", got, b, A, T, x["stop"])
        O.assert_log(log, b, LP.Stopped(x["stop"], A), f"{name} window")
    assert np.array_equal(inner, want_inner), (name, inner, want_inner)
    # the base policy plays on to the end of the episode: what a wrong candidate or a wrong restore only shows later
    more = env.rollout(policy, episodes=1, write_obs=False).cpu().numpy()
    sm, st, log = env.summary().cpu().numpy(), {k: v.cpu().numpy() for k, v in env.status().items()}, O.log(env)
    for b, x in enumerate(ws):
        tail, tag = x["tail"], f"{name} tail env {b}"
        assert int(more[b]) == tail["n_steps"] - x["d0"] - K and int(st["decisions"][b]) == tail["n_steps"], (tag, more[b], st["decisions"][b])
        O.assert_summary(sm[b], tail["result"], tag)
        assert int(st["flags"][b]) == tail["flags"], (tag, st["flags"][b], tail["flags"])
        O.assert_log(log, b, LP.Episode(tail), tag)
    env.close()


def test_a_ragged_loaded_batch_plays_each_env_at_its_own_sizes(gpu_device, oracle_lib):
    _, A, T, sizes = LP.RAGGED
    inst, seeds = LP.ragged_instances()
    env = make(gpu_device, len(sizes), A, T, inst)
    env.reset(seeds, observe=False)
    steps, inner = (x.cpu().numpy() for x in env.rollout("nearest", episodes=1, lookahead=True, width=2, return_inner=True))
    for b, w in enumerate(LW.ragged_walks("nearest", 2)):
        assert_is_the_walk(env, steps, inner, b, w, "ragged width 2")
    env.close()


# ---------------------------------------------------------------------------------------------------- 6. composition and refusals
def test_two_episodes_sum_their_inner_decisions(gpu_device, oracle_lib):
    name, policy, width = "10A20T", "nearest", 2
    A, T, B, _ = LP.TINY[name]
    inst, seeds = LP.instances(name)
    one, two = make(gpu_device, B, A, T, inst), make(gpu_device, B, A, T, inst)
    one.reset(seeds, observe=False)
    two.reset(seeds, observe=False)
    steps, inner = one.rollout(policy, episodes=2, lookahead=True, width=width, return_inner=True)
    n1, i1 = two.rollout(policy, episodes=1, lookahead=True, width=width, return_inner=True)
    n2, i2 = two.rollout(policy, episodes=1, lookahead=True, width=width, return_inner=True)
    assert_same(left_behind(one, steps), left_behind(two, n1 + n2), "episodes=2 against two calls")
    i1, i2 = i1.cpu().numpy(), i2.cpu().numpy()
    assert np.array_equal(i1, [w["inner"] for w in LW.walks(name, policy, width)]) and (i2 > 0).all(), (i1, i2)
    assert np.array_equal(inner.cpu().numpy(), i1 + i2), (inner, i1, i2)
    assert (one.episodes().cpu().numpy() == 2).all()
    one.close(); two.close()


def test_a_budget_stop_and_the_rest_are_one_launch(gpu_device, oracle_lib):
    name, policy, width = "10A20T", "first", 3
    A, T, B, _ = LP.TINY[name]
    inst, seeds = LP.instances(name)
    budget = np.array([0, 9], np.int64)                          # per env: nothing at all, and a stop inside the episode
    whole, parts = make(gpu_device, B, A, T, inst), make(gpu_device, B, A, T, inst)
    whole.reset(seeds, observe=False)
    parts.reset(seeds, observe=False)
    steps, inner = whole.rollout(policy, episodes=1, lookahead=True, width=width, return_inner=True)
    n1, i1 = parts.rollout(policy, episodes=1, lookahead=True, width=width, max_decisions=budget, return_inner=True)
    assert np.array_equal(n1.cpu().numpy(), budget) and not (parts.status()["flags"].cpu().numpy() & 1).any()
    n2, i2 = parts.rollout(policy, episodes=1, lookahead=True, width=width, return_inner=True)
    assert_same(left_behind(parts, n1 + n2), left_behind(whole, steps), "budget stop + rest")
    i1, i2, inner = i1.cpu().numpy(), i2.cpu().numpy(), inner.cpu().numpy()
    assert i1[0] == 0 and 0 < i1[1] < inner[1], (i1, inner)      # an env that valued nothing writes 0
    assert np.array_equal(i1 + i2, inner) and np.array_equal(inner, [w["inner"] for w in LW.walks(name, policy, width)]), (i1, i2, inner)
    whole.close(); parts.close()


def test_refusals_leave_the_state_and_the_outputs_alone(gpu_device):
    from dcmrta_amd._lib import DcmError
    from dcmrta_amd.batched_env import BatchedTaskEnv
    A, T, B, _ = LP.TINY["5A8T"]
    inst, seeds = LP.instances("5A8T")

    def refused(env, status, word, **kw):
        before = env.clone_state().cpu().numpy().copy()
        rc_old = raw(env, old=True, **{k: v for k, v in kw.items() if k != "width"})[0] if kw.get("width", 0) >= 0 else status
        rc, err, steps, inner = raw(env, **kw)
        assert rc == status == rc_old, (kw, rc, rc_old, err)
        assert err.startswith(b"dcm_rollout_lookahead_width:") and word in err, (kw, err)
        assert (steps == -7).all() and (inner == -9).all(), (kw, steps, inner)
        assert np.array_equal(env.clone_state().cpu().numpy(), before), kw
    env = make(gpu_device, B, A, T, inst)
    refused(env, ERR_STATE, b"dcm_reset", policy=2, width=2)                    # no dcm_reset yet
    env.reset(seeds, observe=False)
    for policy in (-1, 3, 7):
        refused(env, ERR_INVALID, b"base policy", policy=policy, width=2)
    for width in (-1, -50):
        refused(env, ERR_INVALID, b"width must be >= 0", policy=2, width=width)
    for episodes in (0, -2):
        refused(env, ERR_INVALID, b"episodes", policy=2, width=2, episodes=episodes)
    env.enable_best_log()
    refused(env, ERR_STATE, b"best log", policy=2, width=2)
    env.enable_best_log(False)
    with pytest.raises(DcmError, match="width must be an integer >= 0"):
        env.rollout("nearest", lookahead=True, width=-1)
    assert raw(env, 1, width=2)[0] == 0                                         # ... and then it runs
    env.close()
    env = make(gpu_device, B, A, T, inst, max_waiting_time=0.0)                 # max_waiting_time <= 0: with a budget too
    env.reset(seeds, observe=False)
    refused(env, ERR_INVALID, b"max_waiting_time <= 0", policy=2, width=2)
    refused(env, ERR_INVALID, b"max_waiting_time <= 0", policy=2, width=2, budget=5)
    env.close()
    env = BatchedTaskEnv(4, 20, 50, device=gpu_device, renew_sizes=True)        # a launch that would be size-renewing
    env.generate_instances(np.arange(300, 304, dtype=np.uint64), agents_range=(10, 20), tasks_range=(20, 50))
    env.set_instance_renewal(4)
    env.reset(5, observe=False)
    refused(env, ERR_STATE, b"renews its sizes", policy=2, width=2, episodes=2)
    env.close()
