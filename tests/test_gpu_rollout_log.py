"""-m gpu: the rollout log of the persistent launches (dcm_set_rollout_log; BatchedTaskEnv.enable_rollout_log) -- every agent's route
and arrival times of the last episode an env played under rollout("random" / "first" / "nearest"), through the register-resident
logging form (k_lg_rollout_fast) and the general one (k_lg_rollout_random), plain and renewing.

Yardsticks: the reference's own route / arrival / members / trajectory arrays (tests/golden/traj_*.npz), the reference's route_len of
the 50A/200T traces, and beyond them the oracle's lists (OracleEnv.route).  Every comparison is exact: task ids, lengths, arrival
times as f64 bit patterns."""
import functools
import os

import numpy as np
import pytest

import helpers as H
import oracle_ref as O
from fixtures_ref import traj_fixture
from forms import Forms

pytestmark = pytest.mark.gpu

ERR_STATE = -4
POLICIES = ("random", "first", "nearest")


# ---------------------------------------------------------------------------------------------------- 1. the reference's own lists
TRAJ = [("traj_5A8T_random_s3.npz", "random"), ("traj_6A9T_random_s5.npz", "random"), ("traj_10A20T_nearest_s4.npz", "nearest")]


@functools.lru_cache(maxsize=None)
def _traj(name):
    return traj_fixture(H.GOLDEN, name)


def test_the_oracle_reproduces_the_trajectory_fixtures_under_its_own_policy():
    """On the CPU: the fixtures' recorded actions are what the oracle's RANDOM / NEAREST policy takes, its lists are the reference's,
    and the longest route has 10 entries (so a log of 16 holds every one)."""
    import oracle
    longest = 0
    for name, policy in TRAJ:
        z, routes, _, _ = _traj(name)
        A, T = z["route"].shape[0], z["task_xy"].shape[0]
        o = oracle.OracleEnv(A, T).load(z["depot"], z["task_xy"], z["req"], z["dur"])
        r = o.rollout(int(z["seed_e"]), 0, O.opol(policy), cap_steps=4096, record=True)
        assert np.array_equal(r["action"], z["action"]), name
        for a, (rt, ra) in enumerate(routes):
            ot, oa = o.route(a)
            assert list(ot) == rt and np.array_equal(oa.view(np.uint64), np.array(ra, np.float64).view(np.uint64)), (name, a)
            longest = max(longest, len(rt))
    assert longest == 10


@pytest.mark.parametrize("name,policy", TRAJ)
def test_reference_routes_arrivals_members_and_trajectories(gpu_device, name, policy):
    """One persistent launch plays the reference's episode and leaves the reference's agent['route'] / ['arrival_time'] lists,
    task['members'], and -- through generate_traj -- its trajectories, array for array."""
    from dcmrta_amd.batched_env import BatchedTaskEnv
    from dcmrta_amd.trajectory import generate_traj
    z, routes, _, ref = _traj(name)
    A, T = z["route"].shape[0], z["task_xy"].shape[0]
    env = BatchedTaskEnv(1, A, T, device=gpu_device).enable_rollout_log(16)
    env.load_instances(z["depot"][None], z["task_xy"][None], z["req"][None], z["dur"][None])
    env.reset(np.array([int(z["seed_e"])], np.uint64), observe=False)
    assert int(env.rollout(policy, episodes=1)[0]) == len(z["action"])
    task, arr, ln = O.log(env)
    for a, (rt, ra) in enumerate(routes):
        assert ln[0, a] == len(rt) and list(task[0, a, :len(rt)]) == rt, (name, a)
        assert np.array_equal(arr[0, a, :len(rt)].view(np.uint64), np.array(ra, np.float64).view(np.uint64)), (name, a)
    assert np.array_equal(env.task_members()[0].cpu().numpy(), z["members"])
    got = generate_traj(env, 0, log="rollout")
    assert len(got) == len(ref)
    for a, (g, r) in enumerate(zip(got, ref)):
        assert g.shape == r.shape and np.array_equal(g, r), (name, a)


# ---------------------------------------------------------------------------------------------------- 2. the oracle through every form
# id: (A, T, B, BatchedTaskEnv keywords, ragged ranges, scalar budget of the launch)
FORMS = {
    "20A50T-fast": (20, 50, 16, {}, None, -1),
    "ragged-fast": (20, 50, 16, {}, ((10, 20), (20, 50)), -1),                  # runtime sizes, loaded (dcm_load_instances_ragged)
    "64A63T-fast": (64, 63, 4, {}, None, -1),                                   # Lay{64,64}
    "64A64T-general": (64, 64, 4, {}, None, -1),                                # no free depot lane
    "50A200T-general": (50, 200, 2, {}, None, -1),                              # multi-chunk
    "70A130T-general": (70, 130, 2, {}, None, -1),                              # runtime layout
    "10A20T-wide": (10, 20, 4, dict(member_cap=16), None, -1),
    "10A20T-mwt0": (10, 20, 4, dict(max_waiting_time=0.0), None, 60),           # the launch stops at 60 decisions: the prefix
}
# ... and one whose launches need the raised dynamic-LDS limit (record_bytes > 64 KiB): test 7 only
BIG_FORMS = {"4A700T-general-above-64KiB": (4, 700, 2, {}, None, -1)}


CAP = 64
F = Forms(FORMS, BIG_FORMS, 4000, 4100, 37)                                  # base seeds: uniform instances, ragged ones, choice


@pytest.mark.parametrize("policy", POLICIES)
@pytest.mark.parametrize("form", sorted(FORMS))
def test_two_episodes_leave_the_second_episodes_lists(gpu_device, form, policy):
    """Two episodes in one launch, so that the restart's zeroing runs: the log holds the second episode's lists (on the
    max_waiting_time = 0 handle, whose launch carries a budget of 60 decisions: the lists of the decisions taken)."""
    budget = FORMS[form][5]
    sims, ref_steps = F.sims(form, policy, 2)
    env, seeds = F.env(gpu_device, form)
    # (the longest list here has 56 entries -- a greedy policy on the max_waiting_time = 0 handle -- so a log of 64 holds every one)
    assert max(len(s.o.route(a)[0]) for s in sims for a in range(s.a)) <= CAP
    env.enable_rollout_log(CAP)
    env.reset(seeds, observe=False)
    steps = env.rollout(policy, episodes=2, max_decisions=budget).cpu().numpy()
    assert np.array_equal(steps, ref_steps), (form, policy)
    if budget < 0:
        assert all(s.j == 1 and s.done for s in sims)                           # every env restarted once and finished
    log = O.log(env)
    for b, s in enumerate(sims):
        O.assert_log(log, b, s, f"{form} {policy}")


@pytest.mark.parametrize("name,policy", [("trace_50A200T_nearest_s0.npz", "nearest"), ("trace_50A200T_random_s0.npz", "random")])
def test_route_lengths_of_the_reference_50A200T_traces(gpu_device, name, policy):
    from dcmrta_amd.batched_env import BatchedTaskEnv
    tr = H.load_trace(os.path.join(H.GOLDEN, name))
    assert int(tr["route_len"].max()) <= 15                                     # (15 under nearest, 12 under random) cap = 16 holds every entry
    env = BatchedTaskEnv(1, 50, 200, device=gpu_device).enable_rollout_log(16)
    env.load_instances(*[tr[k][None] for k in ("depot", "task_xy", "req", "dur")])
    env.reset(np.array([int(tr["seed_e"])], np.uint64), observe=False)
    assert int(env.rollout(policy, episodes=1)[0]) == int(tr["n_steps"])
    log = O.log(env)
    assert np.array_equal(log[2][0], tr["route_len"])
    s = O.Sim(50, 200, lambda j: O.one({k: tr[k][None] for k in ("depot", "task_xy", "req", "dur")}, 0), int(tr["seed_e"]), policy)
    s.launch(1, -1)
    O.assert_log(log, 0, s, name)


# ---------------------------------------------------------------------------------------------------- 3. budget stops
@pytest.mark.parametrize("policy", POLICIES)
@pytest.mark.parametrize("form", ["20A50T-fast", "50A200T-general"])
def test_budget_stops_hold_the_prefix_and_a_later_launch_carries_on(gpu_device, form, policy):
    """Per-env budgets (none, a few, past the episode's end, exactly the episode's last decision, unlimited) in a two-episode launch:
    the log holds the oracle's lists after exactly the decisions taken -- the finished first episode's where the budget ended on its
    last decision.  A second, unlimited launch then appends from the stored lengths (the envs stopped in mid-episode) or restarts (the
    finished ones) and leaves full lists."""
    A, T, B = FORMS[form][:3]
    inst, seeds = F.instances(form)
    n0 = F.sims(form, policy, 1)[1]                                         # length of every env's first episode
    e = 7 % B                                                                   # its budget ends exactly at the episode's last decision
    budgets = np.array([0, 1, 2, 7, 40, 85, -1, 0, 3, 120, -1, 0, 19, 64, 200, 1] if B == 16 else [40, 0], np.int64)
    budgets[e] = n0[e]
    sims = [O.Sim(A, T, lambda j, one=O.one(inst, b): one, seeds[b], policy) for b in range(B)]
    env, _ = F.env(gpu_device, form)
    env.enable_rollout_log(CAP)
    env.reset(seeds, observe=False)
    steps = env.rollout(policy, episodes=2, max_decisions=budgets).cpu().numpy()
    assert np.array_equal(steps, np.array([s.launch(2, int(k)) for s, k in zip(sims, budgets)]))
    assert sims[e].done and sims[e].j == 0 and steps[e] == n0[e]                # stopped at the boundary: the first episode's log stays
    assert any(not s.done and 0 < s.k for s in sims)                            # ... and somebody stopped in mid-episode
    log = O.log(env)
    for b, s in enumerate(sims):
        O.assert_log(log, b, s, f"{form} {policy} after the budgets")
    steps = env.rollout(policy, episodes=1).cpu().numpy()
    assert np.array_equal(steps, np.array([s.launch(1, -1) for s in sims]))
    assert all(s.done for s in sims)
    log = O.log(env)
    for b, s in enumerate(sims):
        O.assert_log(log, b, s, f"{form} {policy} after the second launch")


# ---------------------------------------------------------------------------------------------------- 4. overflow
@pytest.mark.parametrize("policy", POLICIES)
def test_a_log_of_four_counts_the_true_lengths_and_keeps_its_neighbours(gpu_device, policy):
    """cap = 4 at 20A/50T, where routes reach 9 to 13 entries: route_len counts them all, the first four of every list are right, and
    no row spills into the next agent's or the next env's (every row of the batch is compared)."""
    sims, ref_steps = F.sims("20A50T-fast", policy, 1)
    env, seeds = F.env(gpu_device, "20A50T-fast")
    env.enable_rollout_log(4)
    env.reset(seeds, observe=False)
    assert np.array_equal(env.rollout(policy, episodes=1).cpu().numpy(), ref_steps)
    log = O.log(env)
    assert log[0].shape == (16, 20, 4) and log[2].max() >= 9 and (log[2] > 4).sum() > 16 * 20 // 2
    for b, s in enumerate(sims):
        O.assert_log(log, b, s, f"cap 4 {policy}")
    with pytest.raises(ValueError, match=r"enable_rollout_log\(cap\)"):
        env.rollout_plan()


# ---------------------------------------------------------------------------------------------------- 5. renewal
@pytest.mark.parametrize("policy", ["nearest", "random"])
@pytest.mark.parametrize("A,T,B,base", [pytest.param(20, 50, 8, 9300, id="20A50T-fast"), pytest.param(50, 200, 2, 9400, id="50A200T-general")])
def test_the_log_under_instance_renewal_is_the_third_instances(gpu_device, A, T, B, base, policy):
    from dcmrta_amd.batched_env import BatchedTaskEnv
    from dcmrta_amd.choice import env_seeds
    from dcmrta_amd.instances import generate_instance, renewal_seeds
    seeds = env_seeds(71, 0, B)
    env = BatchedTaskEnv(B, A, T, device=gpu_device)
    env.generate_instances(np.arange(base, base + B, dtype=np.uint64))
    env.set_instance_renewal(B)
    env.enable_rollout_log(CAP)
    env.reset(seeds, observe=False)
    steps = env.rollout(policy, episodes=3).cpu().numpy()
    log, idx = O.log(env), env.instance_index().cpu().numpy()
    held = {k: v.cpu().numpy() for k, v in env.instances().items() if v is not None}
    for b in range(B):
        s = O.Sim(A, T, lambda j, b=b: generate_instance(A, T, int(renewal_seeds(base + b, j, B))), seeds[b], policy)
        assert steps[b] == s.launch(3, -1) and s.j == 2 and idx[b] == 2, b
        third = s.inst_of(2)
        assert all(np.array_equal(held[k][b], third[k]) for k in ("depot", "task_xy", "req", "dur")), b
        O.assert_log(log, b, s, f"renewal {A}A{T}T {policy}")


# ---------------------------------------------------------------------------------------------------- 6. refusal
def test_a_size_renewing_launch_is_refused_while_the_log_is_set(gpu_device):
    from dcmrta_amd.batched_env import BatchedTaskEnv
    from dcmrta_amd._lib import DcmError
    B = 8
    env = BatchedTaskEnv(B, 20, 50, device=gpu_device, renew_sizes=True)
    env.generate_instances(np.arange(300, 300 + B, dtype=np.uint64), agents_range=(10, 20), tasks_range=(20, 50))
    env.set_instance_renewal(B)
    env.enable_rollout_log(16)
    env.reset(5, observe=False)
    before = env.clone_state().cpu().numpy().copy()
    for policy in POLICIES:
        with pytest.raises(DcmError, match=r"error %d: dcm_rollout_(random|policy): no rollout log while a ragged batch renews its sizes.*"
                                           r"dcm_set_rollout_log" % ERR_STATE):
            env.rollout(policy, episodes=2)
        assert np.array_equal(env.clone_state().cpu().numpy(), before), policy
    assert (O.log(env)[2] == 0).all()
    env.enable_rollout_log(0)                                                   # without the log the size-renewing random launch runs
    assert int(env.rollout("random", episodes=2).sum()) > 0
    with pytest.raises(DcmError, match="rollout log is off"):
        env.rollout_routes()


# ---------------------------------------------------------------------------------------------------- 7. the log changes nothing else
@pytest.mark.parametrize("policy", POLICIES)
@pytest.mark.parametrize("form", sorted(FORMS) + sorted(BIG_FORMS))
def test_a_launch_with_the_log_returns_what_it_returns_without(gpu_device, form, policy):
    """The same two-episode launch with and without the log: steps, records (clone_state), summary rows, the return log and the
    observation buffers byte for byte.  A lockstep log enabled beside the rollout log stays empty."""
    budget = {**FORMS, **BIG_FORMS}[form][5]
    out = []
    for logged in (False, True):
        env, seeds = F.env(gpu_device, form)
        ring = env.enable_return_log(2)
        if logged:
            env.enable_rollout_log(CAP)
            env.enable_route_log(8)
        env.reset(seeds, observe=False)
        steps = env.rollout(policy, episodes=2, max_decisions=budget)
        o = env.obs()
        out.append([x.cpu().numpy().copy() for x in (steps, env.clone_state(), env.summary(), ring, o.agents, o.tasks, o.mask)])
        if logged:
            task, arr, ln = (x.cpu().numpy() for x in env.routes())
            assert (ln == 0).all() and (task == -2).all() and (arr == 0.0).all()     # the persistent launch never writes the lockstep log
            assert int(O.log(env)[2].sum()) > 0
    assert int(out[0][0].sum()) > 0
    for i, (a, b) in enumerate(zip(*out)):
        assert a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8)), (form, policy, i)


def test_the_lockstep_api_never_writes_the_rollout_log(gpu_device):
    env, seeds = F.env(gpu_device, "10A20T-wide")
    env.enable_rollout_log(16)
    env.enable_route_log(16)
    H.run_lockstep(env, seeds, lambda b, i, m, l: H.host_random_action(m, int(seeds[b]), i))
    task, arr, ln = O.log(env)
    assert (ln == 0).all() and (task == -2).all() and (arr == 0.0).all()
    assert int(env.routes()[2].sum()) > 0                                       # ... while its own log filled


# ---------------------------------------------------------------------------------------------------- 8. a plan goes round
def test_a_nearest_plan_replays_like_the_oracle_and_round_trips_through_yaml(gpu_device, tmp_path):
    import oracle
    import yaml
    from dcmrta_amd.batched_env import BatchedTaskEnv
    from dcmrta_amd.choice import env_seeds
    from dcmrta_amd.instances import generate_batch
    from dcmrta_amd.trajectory import routes_to_yaml
    A, T, B = 10, 20, 4
    inst, seeds = generate_batch(B, A, T, base_seed=615), env_seeds(9, 0, B)
    env = BatchedTaskEnv(B, A, T, device=gpu_device).load_instances(**inst).enable_rollout_log(32)
    env.reset(seeds, observe=False)
    env.rollout("nearest", episodes=1)
    plan = env.rollout_plan()
    ln = O.log(env)[2]
    assert [[len(r) for r in p] for p in plan] == ln.tolist() and ln.sum() > B * A
    assert env.rollout_plan(2) == plan[2]
    for b in range(B):                                                          # Worker.generate_route's file (worker.py:244-251)
        path = tmp_path / f"routes_{b}.yaml"
        assert routes_to_yaml(env, str(path), b, log="rollout") == dict(enumerate(plan[b]))
        assert yaml.safe_load(path.read_text()) == dict(enumerate(plan[b]))
    cap = int(ln.max())
    routes = np.zeros((B, A, cap), np.int32)
    for b in range(B):
        for a in range(A):
            routes[b, a, :ln[b, a]] = plan[b][a]
    ref = oracle.batch_replay(inst["depot"], inst["task_xy"], inst["req"], inst["dur"], routes, ln.astype(np.int32))
    out = env.load_routes(plan).execute_routes(reactive=False, fields=())
    flags = out["flags"].cpu().numpy()
    assert np.array_equal(out["steps"].cpu().numpy(), ref["steps"])
    assert np.array_equal((flags & 4) != 0, ref["status"] == 1) and np.array_equal((flags & 64) != 0, ref["status"] == 2)
    assert not (flags & 0x38).any()
    assert np.array_equal(out["summary"][:, 0].cpu().numpy(), ref["reward"])
