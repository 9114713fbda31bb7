"""-m gpu: the epsilon-greedy device policies of the persistent rollout (dcm_rollout_explore; BatchedTaskEnv.rollout(..., explore= /
explore_q32=)) on the register-resident form (k_ex_rollout_fast) and the general form (k_ex_rollout_random), plain and renewing, with
the rollout log set and without it.

Yardsticks: explore_q32 = 0 is the greedy launch and explore_q32 = 2^32 the random one, byte for byte, and both are the oracle's; every
value in between is a chain of one-decision greedy / random launches chosen on the host by choice.explores -- existing, oracle-pinned
entry points only; and four known answers computed on the CPU from the definition.  Every comparison is exact."""
import numpy as np
import pytest

import oracle_ref as O
from forms import Forms, assert_same, snap

pytestmark = pytest.mark.gpu

ERR_INVALID, ERR_STATE = -1, -4
BASES = ("first", "nearest")
Q_ALL = 1 << 32
CAP = 64

# id: (A, T, B, BatchedTaskEnv keywords, ragged ranges, scalar budget of every launch)
FORMS = {
    "F1": (20, 50, 6, {}, None, -1),                                            # fast, exact
    "F2": (20, 50, 6, {}, ((10, 20), (20, 50)), -1),                            # fast, runtime sizes (a ragged batch)
    "F3": (30, 60, 4, {}, None, -1),                                            # fast, Lay{64,64}
    "F4": (10, 64, 4, {}, None, -1),                                            # general: no free depot lane
    "F5": (66, 70, 4, {}, None, -1),                                            # general, the mid-size layout
    "F6": (10, 20, 4, dict(max_waiting_time=0.0), None, 60),                    # general, the literal rule; every launch under a budget
}
# ... and one whose launches need the raised dynamic-LDS limit (record_bytes > 64 KiB): the two ends only
BIG_FORMS = {"F7-above-64KiB": (4, 700, 2, {}, None, -1)}
ALL_FORMS = {**FORMS, **BIG_FORMS}
F = Forms(FORMS, BIG_FORMS, 6000, 6100, 41)                                     # base seeds: uniform instances, ragged ones, choice


def _form_env(gpu_device, form, logged=True, ring=2):
    env, seeds = F.env(gpu_device, form)
    if logged:
        env.enable_rollout_log(CAP)
    env._ring = env.enable_return_log(ring)
    env.reset(seeds, observe=False)
    return env, seeds


# ---------------------------------------------------------------------------------------------------- 1. + 2. the two ends
@pytest.mark.parametrize("logged", [True, False], ids=["log", "nolog"])
@pytest.mark.parametrize("base", BASES)
@pytest.mark.parametrize("form", sorted(ALL_FORMS))
def test_the_ends_are_the_greedy_and_the_random_policy(gpu_device, form, base, logged):
    """explore_q32 = 0 against rollout(base), explore_q32 = 2^32 against rollout("random"), each on a twin handle, two episodes: byte for
    byte; and the twin's launch is the oracle's (steps, the last episode's reward, the logged lists)."""
    budget = ALL_FORMS[form][5]
    for q32, pinned in ((0, base), (Q_ALL, "random")):
        tag = f"{form} {base} q={q32} {'log' if logged else 'nolog'}"
        twin, _ = _form_env(gpu_device, form, logged)
        ref = snap(twin, twin.rollout(pinned, episodes=2, max_decisions=budget).cpu().numpy())
        env, _ = _form_env(gpu_device, form, logged)
        got = snap(env, env.rollout(base, episodes=2, max_decisions=budget, explore_q32=q32).cpu().numpy())
        assert_same(got, ref, tag)
        sims, ref_steps = F.sims(form, pinned, 2)
        assert np.array_equal(got["steps"], ref_steps), tag
        for b, s in enumerate(sims):
            if s.done:
                assert got["summary"][b, 0] == s.o.final()["reward"] and got["flags"][b] & 1, (tag, b)
            else:
                assert budget >= 0 and not got["flags"][b] & 1, (tag, b)
        if logged:
            log = O.log(env)
            for b, s in enumerate(sims):
                O.assert_log(log, b, s, tag)


# ---------------------------------------------------------------------------------------------------- 3. in between: the chain
def _chain(env, seeds, base, q32, episodes, total):
    """The epsilon-greedy policy composed of pinned launches: per round, every env that still has episodes (and budget) to play takes ONE
    decision -- in rollout(base) if choice.explores says no, in rollout("random") if it says yes; everybody else gets budget 0.  A budget
    stop leaves an env at its decision point and a later launch carries on identically.  Returns (steps, explored[B], greedy[B])."""
    from dcmrta_amd.choice import explores
    B = env.B
    eps_done, taken = np.zeros(B, np.int64), np.zeros(B, np.int64)
    n_ex, n_gr = np.zeros(B, np.int64), np.zeros(B, np.int64)
    for _ in range(20000):
        live = (eps_done < episodes) & ((taken < total) if total >= 0 else True)
        if not live.any():
            break
        d = env.status()["decisions"].cpu().numpy()
        ex = np.array([bool(live[b]) and explores(int(seeds[b]), int(d[b]), q32) for b in range(B)])
        gr = live & ~ex
        steps = np.zeros(B, np.int64)
        if gr.any():
            steps += env.rollout(base, episodes=1, max_decisions=gr.astype(np.int64)).cpu().numpy()
        if ex.any():
            steps += env.rollout("random", episodes=1, max_decisions=ex.astype(np.int64)).cpu().numpy()
        assert np.array_equal(steps, live.astype(np.int64))
        taken += steps
        n_ex += ex
        n_gr += gr
        eps_done += live & ((env.status()["flags"].cpu().numpy() & 1) != 0)
    else:
        raise AssertionError("the chain did not end")
    return taken, n_ex, n_gr


CHAIN_CASES = [(f, b, 1 << 30) for f in sorted(FORMS) for b in BASES] + [(f, b, 1 << 31) for f in ("F1", "F4") for b in BASES]


@pytest.mark.parametrize("form,base,q32", CHAIN_CASES, ids=[f"{f}-{b}-2^{q.bit_length() - 1}" for f, b, q in CHAIN_CASES])
def test_a_launch_is_the_chain_of_pinned_one_decision_launches(gpu_device, form, base, q32):
    budget = FORMS[form][5]
    twin, seeds = _form_env(gpu_device, form)
    taken, n_ex, n_gr = _chain(twin, seeds, base, q32, 2, budget)
    assert ((n_ex > 0) & (n_gr > 0)).any(), (n_ex, n_gr)                        # some env both explored and did not: not vacuous
    ref = snap(twin, taken)
    env, _ = _form_env(gpu_device, form)
    got = snap(env, env.rollout(base, episodes=2, max_decisions=budget, explore_q32=q32).cpu().numpy())
    assert_same(got, ref, f"{form} {base} q={q32}")


# ---------------------------------------------------------------------------------------------------- 4. budget stop and continuation
@pytest.mark.parametrize("base", BASES)
@pytest.mark.parametrize("form", ["F1", "F4"])
def test_a_budget_stop_in_mid_episode_and_a_second_launch_equal_the_uninterrupted_one(gpu_device, form, base):
    q32 = 1 << 30
    B = FORMS[form][2]
    whole, _ = _form_env(gpu_device, form)
    ref = snap(whole, whole.rollout(base, episodes=2, explore_q32=q32).cpu().numpy())
    budgets = np.array([0, 1, 7, 23, 2, 30][:B], np.int64)                      # all inside the first episode (checked below)
    env, _ = _form_env(gpu_device, form)
    first = env.rollout(base, episodes=2, max_decisions=budgets, explore_q32=q32).cpu().numpy()
    assert np.array_equal(first, budgets) and not (env.status()["flags"].cpu().numpy() & 1).any()
    second = env.rollout(base, episodes=2, explore_q32=q32).cpu().numpy()
    assert (second > 0).all()
    assert_same(snap(env, first + second), ref, f"{form} {base}")


# ---------------------------------------------------------------------------------------------------- 5. instance renewal
@pytest.mark.parametrize("A,T,B,base_seed", [pytest.param(20, 50, 6, 9500, id="F1"), pytest.param(10, 64, 4, 9600, id="F4")])
def test_three_episodes_under_instance_renewal_play_instances_0_1_2(gpu_device, A, T, B, base_seed):
    from dcmrta_amd.batched_env import BatchedTaskEnv
    from dcmrta_amd.choice import env_seeds
    from dcmrta_amd.instances import generate_instance, renewal_seeds
    seeds, q32 = env_seeds(83, 0, B), 1 << 30

    def make():
        env = BatchedTaskEnv(B, A, T, device=gpu_device)
        env.generate_instances(np.arange(base_seed, base_seed + B, dtype=np.uint64))
        env.set_instance_renewal(B)
        env.enable_rollout_log(CAP)
        env._ring = env.enable_return_log(3)
        env.reset(seeds, observe=False)
        return env

    twin = make()
    taken, n_ex, n_gr = _chain(twin, seeds, "nearest", q32, 3, -1)
    assert ((n_ex > 0) & (n_gr > 0)).any()
    ref = snap(twin, taken)
    env = make()
    got = snap(env, env.rollout("nearest", episodes=3, explore_q32=q32).cpu().numpy())
    assert_same(got, ref, f"renewal {A}A{T}T")
    assert (env.instance_index().cpu().numpy() == 2).all() and (twin.instance_index().cpu().numpy() == 2).all()
    held = {k: v.cpu().numpy() for k, v in env.instances().items() if v is not None}
    for b in range(B):
        third = generate_instance(A, T, int(renewal_seeds(base_seed + b, 2, B)))
        assert all(np.array_equal(held[k][b], third[k]) for k in ("depot", "task_xy", "req", "dur")), b
    assert not np.isnan(got["ring"]).any()


# ---------------------------------------------------------------------------------------------------- 6. known answers
# 20A/50T, instance generate_instance(20, 50, 7000 + i), env seed env_seed(11, i), 256 consecutive episodes in one env, nearest at
# explore_q32 = 214748364 (epsilon 0.05): computed on the CPU by the project's oracle with the definition's pick in place of policy_pick.
# (nearest's return of every episode, the best return under epsilon 0.05, the episode it came in, decisions of the 256 episodes)
KNOWN = [(-66.46152330138433, -64.2592719427987, 21, 30536),
         (-73.17642526148323, -59.269079517211125, 43, 27368),
         (-68.08463749080511, -53.5311803994863, 230, 27990),
         (-67.97824060623559, -55.751632502919165, 73, 29958)]


def test_known_answers_of_256_episodes_at_epsilon_0_05(gpu_device):
    from dcmrta_amd.batched_env import BatchedTaskEnv
    from dcmrta_amd.choice import env_seed, explore_q32
    from dcmrta_amd.instances import generate_instance
    B = len(KNOWN)
    insts = [generate_instance(20, 50, 7000 + i) for i in range(B)]
    seeds = np.array([env_seed(11, i) for i in range(B)], np.uint64)
    assert explore_q32(0.05) == 214748364

    def make(cap):
        env = BatchedTaskEnv(B, 20, 50, device=gpu_device)
        env.load_instances(*[np.stack([i[k] for i in insts]) for k in ("depot", "task_xy", "req", "dur")])
        ring = env.enable_return_log(cap)
        env.reset(seeds, observe=False)
        return env, ring

    bits = lambda x: np.array(x, np.float64).view(np.uint64)
    env, ring = make(256)
    steps = env.rollout("nearest", episodes=256, write_obs=False, explore=0.05).cpu().numpy()
    rl = ring.cpu().numpy()
    print("best returns", [repr(float(np.nanmax(r))) for r in rl], "at", [int(np.nanargmax(r)) for r in rl], "steps", steps.tolist())
    for i, (_, best, at, n) in enumerate(KNOWN):
        assert not np.isnan(rl[i]).any(), i
        assert bits(np.nanmax(rl[i])) == bits(best) and int(np.nanargmax(rl[i])) == at and int(steps[i]) == n, (i, np.nanmax(rl[i]))
    for kw in (dict(), dict(explore_q32=0)):
        env, ring = make(2)
        env.rollout("nearest", episodes=2, **kw)
        rl = ring.cpu().numpy()
        for i, (greedy, _, _, _) in enumerate(KNOWN):
            assert np.array_equal(bits(rl[i]), bits([greedy, greedy])), (i, kw, rl[i])


# ---------------------------------------------------------------------------------------------------- 7. refusals
def _raw(env, policy, q32, budget=-1, episodes=1):
    import ctypes as C
    import torch
    from dcmrta_amd.batched_env import _ptr
    steps = torch.full((env.B,), -7, dtype=torch.int64, device=env.device)
    with torch.cuda.device(env.device):
        rc = env._lib.dcm_rollout_explore(env._h, policy, C.c_uint64(q32), episodes, budget, None, None, None, None, _ptr(steps), env._stream())
    return rc, env._lib.dcm_last_error(), steps.cpu().numpy()


def test_refusals_leave_the_state_alone(gpu_device):
    from dcmrta_amd.batched_env import BatchedTaskEnv
    from dcmrta_amd._lib import DcmError
    env, _ = _form_env(gpu_device, "F1")
    before = env.clone_state().cpu().numpy().copy()
    for policy, q32, status, msg in ((0, 5, ERR_INVALID, b"base policy"), (3, 5, ERR_INVALID, b"base policy"), (-1, 0, ERR_INVALID, b"base policy"),
                                     (2, Q_ALL + 1, ERR_INVALID, b"explore_q32"), (1, (1 << 64) - 1, ERR_INVALID, b"explore_q32")):
        rc, err, steps = _raw(env, policy, q32)
        assert rc == status and msg in err and err.startswith(b"dcm_rollout_explore:") and (steps == -7).all(), (policy, q32, rc, err)
    assert np.array_equal(env.clone_state().cpu().numpy(), before)
    with pytest.raises(DcmError, match="greedy base policy"):
        env.rollout("random", explore=0.5)
    assert _raw(env, 2, Q_ALL)[0] == 0                                          # ... and the largest value runs
    # a size-renewing launch
    B = 8
    env = BatchedTaskEnv(B, 20, 50, device=gpu_device, renew_sizes=True)
    env.generate_instances(np.arange(300, 300 + B, dtype=np.uint64), agents_range=(10, 20), tasks_range=(20, 50))
    env.set_instance_renewal(B)
    env.reset(5, observe=False)
    before = env.clone_state().cpu().numpy().copy()
    with pytest.raises(DcmError, match=r"error %d: dcm_rollout_explore: no epsilon-greedy policy while a ragged batch renews its sizes" % ERR_STATE):
        env.rollout("nearest", episodes=2, explore=0.1)
    assert np.array_equal(env.clone_state().cpu().numpy(), before)
    env.set_instance_renewal(0)                                                 # ragged without renewal works
    assert int(env.rollout("nearest", episodes=1, explore=0.1).sum()) > 0
    # max_waiting_time <= 0 without a budget
    env, _ = _form_env(gpu_device, "F6")
    before = env.clone_state().cpu().numpy().copy()
    with pytest.raises(DcmError, match=r"error %d: dcm_rollout_explore: .*give a decision budget" % ERR_INVALID):
        env.rollout("first", episodes=2, explore=0.1)
    assert np.array_equal(env.clone_state().cpu().numpy(), before)
    # ... and a negative per-env entry counts as 0 there
    neg = np.array([-1, 0, -5, -1], np.int64)
    assert np.array_equal(env.rollout("first", episodes=2, max_decisions=neg, explore=0.1).cpu().numpy(), np.zeros(4, np.int64))
    assert np.array_equal(env.clone_state().cpu().numpy(), before)


# ---------------------------------------------------------------------------------------------------- 8. a sampled plan
def test_the_best_sampled_episode_is_a_plan_the_route_replay_accepts(gpu_device):
    from dcmrta_amd.batched_env import BatchedTaskEnv
    from dcmrta_amd.choice import env_seeds
    from dcmrta_amd.instances import generate_instance
    A, T, B = 20, 50, 64
    inst = generate_instance(A, T, 7001)
    rep = lambda n: [np.stack([inst[k]] * n) for k in ("depot", "task_xy", "req", "dur")]
    env = BatchedTaskEnv(B, A, T, device=gpu_device).load_instances(*rep(B))
    env.enable_rollout_log(CAP)
    env.reset(env_seeds(19, 0, B), observe=False)
    env.rollout("nearest", episodes=1, explore=0.05)
    sm = env.summary().cpu().numpy()
    assert len(set(sm[:, 0].tolist())) > B // 4                                 # the seeds give different episodes
    best = max(range(B), key=lambda b: (sm[b, 1], sm[b, 0]))
    plan = env.rollout_plan(best)
    assert len(plan) == A and sum(len(r) for r in plan) > A
    one = BatchedTaskEnv(1, A, T, device=gpu_device).load_instances(*rep(1))
    out = one.load_routes([plan]).execute_routes(reactive=False, fields=())
    flags = int(out["flags"].cpu().numpy()[0])
    assert not flags & 0x38, flags                                              # no bad action, overflow or bad leader
