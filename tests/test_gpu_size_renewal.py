"""-m gpu: size renewal (DCM_PARAM_RENEW_SIZES, BatchedTaskEnv(renew_sizes=True)) -- on a ragged batch made by generate_instances
an env that restarts an episode inside a kernel draws its next instance WITH its next sizes, the way every reference Worker builds
a fresh TaskEnv(agents_range, tasks_range, ..., seed=...) with the tuple ranges of parameters.py:15-16 (worker.py:32,
env/task_env.py:58-65).

The yardstick is the oracle with a new host instance per episode (renewal_ref.oracle_chain), as in test_gpu_instance_renewal:
episode k of env b plays generate_instance_ranges(agents_range, tasks_range, renewal_seeds(base + b, k, stride)) on an
OracleEnv(A_k, T_k), with the decision counter running across the episodes.  Every comparison is array_equal."""
import numpy as np
import pytest
import torch

import helpers as H
import renewal_ref as R
from renewal_ref import EPISODES, M64

pytestmark = pytest.mark.gpu

GAMMA = 0x9E3779B97F4A7C15
ERR_STATE = -4
WRAP_STRIDE = (1 << 63) + 12345          # two of them pass 2^64


def _size_table(ar, tr, B, base, stride, mcs=5, n=EPISODES):
    """[episode, env, (A, T)] on the host -- and the condition every case must meet: in every dimension that has a range some env grows
    and some env shrinks between consecutive episodes, so that a later change of seeds cannot quietly test nothing."""
    from dcmrta_amd.instances import renewal_seeds
    sz = np.zeros((n, B, 2), np.int64)
    for k in range(n):
        for b in range(B):
            A, inst = R.host_instance(ar, tr, int(renewal_seeds((base + b) % M64, k, stride)), mcs)
            sz[k, b] = (A, inst["req"].shape[0])
    for dim, r in ((0, ar), (1, tr)):
        d = np.diff(sz[:, :, dim], axis=0)
        if isinstance(r, tuple) and r[0] < r[1]:
            assert (d > 0).any() and (d < 0).any(), ("sizes must both grow and shrink", dim, sz[:, :, dim].tolist())
        else:
            assert not d.any()
    return sz


# agents range, tasks range, batch, member_cap / max_coalition_size, stride (None = B), base seed: one case per kernel class of
# dcm_rollout_random that can serve a ragged batch
ROLLOUT_CASES = [
    pytest.param((3, 20), (5, 50), 32, 5, 5, None, 18100, id="20x50-layout"),
    pytest.param((10, 20), (20, 50), 32, 5, 5, None, 18150, id="reference-ranges"),
    pytest.param((10, 64), (20, 63), 16, 5, 5, None, 18300, id="64x64-layout"),
    pytest.param((30, 70), (40, 160), 8, 5, 5, None, 18500, id="fast-g"),
    pytest.param((60, 100), (200, 300), 4, 5, 5, None, 18600, id="general"),
    pytest.param((3, 20), (5, 50), 16, 16, 9, None, 18700, id="wide-9"),
    pytest.param(20, (5, 50), 16, 5, 5, None, 18800, id="tasks-range-only"),
    pytest.param((3, 20), 50, 16, 5, 5, None, 18900, id="agents-range-only"),
    pytest.param((3, 20), (5, 50), 16, 5, 5, WRAP_STRIDE, (1 << 63) + 77, id="20x50-layout-stride-wraps"),
    pytest.param(4, (690, 700), 2, 5, 5, None, 19000, id="general-above-64KiB"),   # a launch that needs the raised dynamic-LDS limit
]


@pytest.mark.parametrize("ar,tr,B,member_cap,mcs,stride,base", ROLLOUT_CASES)
def test_persistent_rollout_plays_new_sizes_every_episode(gpu_device, ar, tr, B, member_cap, mcs, stride, base):
    from dcmrta_amd.choice import env_seeds
    stride = B if stride is None else stride
    _size_table(ar, tr, B, base, stride, mcs)
    seeds = env_seeds(61, 0, B)
    env, ring = R.make(gpu_device, B, ar, tr, base, stride, mcs, member_cap)
    if R.dim(tr) == 700:
        assert env.record_bytes() > 65536
    env.reset(seeds, observe=False)
    steps = env.rollout_random(episodes=EPISODES).cpu().numpy()
    R.assert_after(env, ring, R.chains(ar, tr, B, base, stride, seeds, mcs), steps)


def test_split_calls_give_the_same_results(gpu_device):
    """Three calls of one episode; a per-env budget that stops mid-episode, then a call that finishes; a budget that runs out exactly
    at an episode boundary leaves index, instance AND sizes unrenewed until the next call.  Same arrays as the single call."""
    from dcmrta_amd.choice import env_seeds
    ar, tr, B, base = (3, 20), (5, 50), 32, 18100
    _size_table(ar, tr, B, base, B)
    seeds = env_seeds(61, 0, B)
    chains = R.chains(ar, tr, B, base, B, seeds)
    n0 = np.array([chains[b][0][0]["n_steps"] for b in range(B)], np.int64)
    n1 = np.array([chains[b][0][1]["n_steps"] for b in range(B)], np.int64)
    # three calls of one episode each
    env, ring = R.make(gpu_device, B, ar, tr, base, B)
    env.reset(seeds, observe=False)
    steps = sum(env.rollout_random(episodes=1).cpu().numpy() for _ in range(EPISODES))
    R.assert_after(env, ring, chains, steps)
    # a budget that ends in the middle of episode 1 (every env its own), then the rest: the pending episode counts as one
    env, ring = R.make(gpu_device, B, ar, tr, base, B)
    env.reset(seeds, observe=False)
    s1 = env.rollout_random(episodes=EPISODES, max_decisions=n0 + n1 // 2).cpu().numpy()
    assert np.array_equal(s1, n0 + n1 // 2)
    assert np.array_equal(env.instance_index().cpu().numpy(), np.ones(B, np.int64))
    held = R.held(env)
    for b in range(B):
        R.assert_instance(held, b, chains[b][1][1])
    s2 = env.rollout_random(episodes=2).cpu().numpy()
    R.assert_after(env, ring, chains, s1 + s2)
    # a budget that runs out exactly at the end of episode 0: the finished episode's instance, sizes and results stay
    env, ring = R.make(gpu_device, B, ar, tr, base, B)
    env.reset(seeds, observe=False)
    s1 = env.rollout_random(episodes=EPISODES, max_decisions=n0).cpu().numpy()
    assert np.array_equal(s1, n0)
    assert np.array_equal(env.instance_index().cpu().numpy(), np.zeros(B, np.int64))
    held, sm = R.held(env), env.summary().cpu().numpy()
    for b in range(B):
        R.assert_instance(held, b, chains[b][1][0])
        assert np.array_equal(sm[b], chains[b][0][0]["row"], equal_nan=True), b
    s2 = env.rollout_random(episodes=2).cpu().numpy()
    R.assert_after(env, ring, chains, s1 + s2)


@pytest.mark.parametrize("ar,tr,B,base", [
    pytest.param((3, 20), (5, 50), 32, 18100, id="20x50-layout"),
    pytest.param((30, 70), (40, 160), 8, 18500, id="fast-g"),
])
def test_stored_observations_after_a_size_change(gpu_device, ar, tr, B, base):
    """What the summary cannot see: the observation buffers j decisions into episode 1 equal, over the WHOLE batch shape, those of an
    unflagged twin that was given instance 1 (a ragged batch: tests/test_gpu_ragged.py checks that path against the oracle) and took
    the same j decisions -- rows beyond the env's new sizes are padding (-1, mask 1), rows that were padding in episode 0 are real."""
    from dcmrta_amd.batched_env import BatchedTaskEnv
    from dcmrta_amd.choice import env_seeds
    from dcmrta_amd.instances import renewal_seeds
    J = 3
    sz = _size_table(ar, tr, B, base, B)
    assert (sz[1] > sz[0]).any() and (sz[1] < sz[0]).any()
    seeds = env_seeds(61, 0, B)
    chains = R.chains(ar, tr, B, base, B, seeds)
    n0 = np.array([chains[b][0][0]["n_steps"] for b in range(B)], np.int64)
    assert all(chains[b][0][1]["n_steps"] >= J for b in range(B))
    x, _ = R.make(gpu_device, B, ar, tr, base, B)
    x.reset(seeds, observe=False)
    sx = x.rollout_random(episodes=EPISODES, max_decisions=n0 + J).cpu().numpy()
    assert np.array_equal(sx, n0 + J)
    y = BatchedTaskEnv(B, R.dim(ar), R.dim(tr), device=gpu_device)
    y.generate_instances(renewal_seeds(R.inst_seeds(base, B), 1, B), agents_range=ar, tasks_range=tr)
    y.reset(np.array([(int(seeds[b]) + GAMMA * int(n0[b])) % M64 for b in range(B)], dtype=np.uint64), observe=False)
    sy = y.rollout_random(episodes=1, max_decisions=J).cpu().numpy()
    assert np.array_equal(sy, np.full(B, J))
    for name in ("_agents", "_tasks", "_mask"):
        gx, gy = getattr(x, name).cpu().numpy(), getattr(y, name).cpu().numpy()
        assert gx.shape == gy.shape and np.array_equal(gx, gy), name
    # the padding really is there, and really moved
    mask = x._mask.cpu().numpy()
    for b in range(B):
        assert (mask[b, sz[1, b, 1] + 1:] == 1).all() and (x._agents[b, sz[1, b, 0]:].cpu().numpy() == -1.0).all(), b


@pytest.mark.parametrize("ar,tr,B,base,read_every", [
    pytest.param((10, 20), (20, 50), 64, 19100, 40, id="reference-ranges"),
    pytest.param((10, 20), (20, 50), 64, 19100, 0, id="reference-ranges-summaries-read-at-the-end"),
    pytest.param((10, 64), (20, 63), 16, 19300, 40, id="64x64-layout"),
    pytest.param((30, 70), (40, 160), 8, 19400, 40, id="general-k_step-128x256"),
    pytest.param(4, (690, 700), 2, 19000, 40, id="general-k_step-above-64KiB"),
])
def test_lockstep_auto_reset_renews_sizes(gpu_device, ar, tr, B, base, read_every):
    from dcmrta_amd.choice import env_seeds
    _size_table(ar, tr, B, base, B)
    seeds = env_seeds(63, 0, B)
    env, ring = R.make(gpu_device, B, ar, tr, base, B, auto_reset=True, auto_reset_episodes=EPISODES)
    if R.dim(tr) == 700:
        assert env.record_bytes() > 65536
    dcount = R.lockstep_to_end(env, seeds, read_every)
    R.assert_after(env, ring, R.chains(ar, tr, B, base, B, seeds), dcount)
    assert np.array_equal(env.status()["decisions"].cpu().numpy(), dcount)


def test_first_observation_after_a_size_renewal_is_the_new_instances(gpu_device):
    """The dcm_step that ends episode 0 returns the first decision of episode 1: it must equal reset() of an unflagged twin that was
    GIVEN instance 1 (same ranges, seeds + stride) with the choice seed seed + GAMMA * d, over the whole batch-shaped tensors --
    padding rows of the new sizes included -- and the leader."""
    from dcmrta_amd.batched_env import BatchedTaskEnv
    from dcmrta_amd.choice import env_seeds
    ar, tr, B, base = (3, 20), (5, 50), 64, 19600
    sz = _size_table(ar, tr, B, base, B, n=2)
    seeds = env_seeds(65, 0, B)
    env, _ = R.make(gpu_device, B, ar, tr, base, B, auto_reset=True, auto_reset_episodes=2)
    obs = env.reset(seeds)
    dcount, seen, got = np.zeros(B, np.int64), np.zeros(B, bool), {}
    for s in range(4000):
        mk = obs.mask.cpu().numpy().astype(np.uint8)
        active = obs.active.cpu().numpy()
        act = np.array([H.host_random_action(mk[b], int(seeds[b]), int(dcount[b])) if active[b] else 0 for b in range(B)], np.int32)
        obs = env.step(act)
        dcount += active
        eps = env.episodes().cpu().numpy()
        for b in np.flatnonzero((eps >= 1) & ~seen):
            got[b] = (int(dcount[b]), obs.agents[b].cpu().numpy(), obs.tasks[b].cpu().numpy(), obs.mask[b].cpu().numpy(),
                      int(obs.leader[b]))
            seen[b] = True
        if seen.all():
            break
    assert seen.all()
    twin = BatchedTaskEnv(B, R.dim(ar), R.dim(tr), device=gpu_device).generate_instances(R.inst_seeds(base + B, B), agents_range=ar, tasks_range=tr)
    assert np.array_equal(twin.n_agents, sz[1, :, 0]) and np.array_equal(twin.n_tasks, sz[1, :, 1])
    tobs = twin.reset(np.array([(int(seeds[b]) + GAMMA * got[b][0]) % M64 for b in range(B)], dtype=np.uint64))
    ta, tt, tm, tl = tobs.agents.cpu().numpy(), tobs.tasks.cpu().numpy(), tobs.mask.cpu().numpy(), tobs.leader.cpu().numpy()
    for b in range(B):
        _, ag, tk, mk, ld = got[b]
        assert np.array_equal(ag, ta[b]) and np.array_equal(tk, tt[b]) and np.array_equal(mk, tm[b]) and ld == tl[b], b


def test_captured_step_loop_renews_sizes_like_the_eager_loop(gpu_device):
    from dcmrta_amd.choice import env_seeds
    from dcmrta_amd.graph_rollout import GraphedRollout
    ar, tr, B, base = (10, 20), (20, 50), 64, 19700
    _size_table(ar, tr, B, base, B)
    seeds = env_seeds(67, 0, B)
    policy = lambda obs: torch.argmax((~obs.mask).to(torch.int32), dim=1).to(torch.int32)
    eager, ering = R.make(gpu_device, B, ar, tr, base, B, auto_reset=True, auto_reset_episodes=EPISODES)
    R.lockstep_to_end(eager, seeds, policy=policy)
    env, ring = R.make(gpu_device, B, ar, tr, base, B, auto_reset=True, auto_reset_episodes=EPISODES)
    GraphedRollout(env, policy, check_every=8).run(seeds, max_steps=4000)
    assert np.array_equal(env.episodes().cpu().numpy(), np.full(B, EPISODES))
    assert np.array_equal(ring.cpu().numpy(), ering.cpu().numpy())
    assert np.array_equal(env.summary().cpu().numpy(), eager.summary().cpu().numpy(), equal_nan=True)
    assert np.array_equal(env.instance_index().cpu().numpy(), np.full(B, EPISODES - 1))
    a, b = R.held(env), R.held(eager)
    assert all(np.array_equal(a[k], b[k]) for k in a)
    # ... and the held instances are instance 2 with its sizes
    from dcmrta_amd.instances import renewal_seeds
    for e in range(B):
        R.assert_instance(a, e, R.host_instance(ar, tr, int(renewal_seeds((base + e) % M64, 2, B)), 5))
    assert not np.array_equal(ering.cpu().numpy()[:, 0], ering.cpu().numpy()[:, 1])


def test_clone_and_restore_carry_the_sizes(gpu_device):
    from dcmrta_amd.batched_env import BatchedTaskEnv
    from dcmrta_amd.choice import env_seeds
    ar, tr, B, base = (3, 20), (5, 50), 16, 18100
    seeds = env_seeds(61, 0, B)
    _size_table(ar, tr, B, base, 32)
    chains = R.chains(ar, tr, B, base, 32, seeds)                   # (the first 16 envs of the B = 32 case: stride 32)
    env, ring = R.make(gpu_device, B, ar, tr, base, 32)
    env.reset(seeds, observe=False)
    s0 = env.rollout_random(episodes=1, max_decisions=5).cpu().numpy()           # in episode 0
    assert all(chains[b][0][0]["n_steps"] > 5 for b in range(B))
    snap = env.clone_state()
    # the snapshot of a flagged handle with a ragged batch holds the per-env sizes: 8 B bytes more than an unflagged handle's
    plain = BatchedTaskEnv(B, R.dim(ar), R.dim(tr), device=gpu_device).generate_instances(R.inst_seeds(base, B), agents_range=ar, tasks_range=tr)
    plain.reset(seeds, observe=False)
    assert snap.numel() == plain.clone_state().numel() + 8 * B
    s1 = env.rollout_random(episodes=EPISODES).cpu().numpy()                     # into episode 2
    R.assert_after(env, ring, chains, s0 + s1)
    first = (env.summary().clone(), ring.clone(), R.held(env))
    env.restore_state(snap)
    assert np.array_equal(env.instance_index().cpu().numpy(), np.zeros(B, np.int64))
    held = R.held(env)
    for b in range(B):
        R.assert_instance(held, b, chains[b][1][0])
    ring.fill_(float("nan"))
    s2 = env.rollout_random(episodes=EPISODES).cpu().numpy()
    assert np.array_equal(s2, s1)
    assert torch.equal(env.summary().view(torch.int64), first[0].view(torch.int64)) and torch.equal(ring.view(torch.int64), first[1].view(torch.int64))
    again = R.held(env)
    assert all(np.array_equal(again[k], first[2][k]) for k in again)
    R.assert_after(env, ring, chains, s0 + s2)


def test_state_rules(gpu_device):
    from dcmrta_amd._lib import DcmError
    from dcmrta_amd.batched_env import BatchedTaskEnv
    from dcmrta_amd.choice import env_seeds
    from dcmrta_amd.instances import generate_batch_ranges, generate_batch
    ar, tr, B = (3, 12), (5, 23), 8
    A, T = R.dim(ar), R.dim(tr)
    seeds = env_seeds(66, 0, B)
    env = BatchedTaskEnv(B, A, T, device=gpu_device, renew_sizes=True)
    setter = lambda stride: env._lib.dcm_set_instance_renewal(env._h, stride)
    # an unflagged handle refuses the ragged generated batch; the flagged one accepts it, with either or both ranges
    plain = BatchedTaskEnv(B, A, T, device=gpu_device).generate_instances(100, agents_range=ar, tasks_range=tr)
    assert plain._lib.dcm_set_instance_renewal(plain._h, B) == ERR_STATE
    env.generate_instances(100, agents_range=ar, tasks_range=tr)
    assert setter(B) == 0
    env.generate_instances(100, tasks_range=tr)
    assert setter(B) == 0
    env.generate_instances(100, agents_range=ar)
    assert setter(B) == 0
    # a loaded ragged batch is refused with the flag too, and a loaded uniform one
    env.load_instances(**generate_batch_ranges(range(100, 100 + B), ar, tr))
    assert setter(B) == ERR_STATE and b"dcm_set_instance_renewal" in env._lib.dcm_last_error()
    assert setter(0) == 0
    with pytest.raises(DcmError):
        env.set_instance_renewal(B)
    env.load_instances(**generate_batch(B, A, T, base_seed=1))
    assert setter(B) == ERR_STATE

    def two_episodes_change_nothing():
        before = R.held(env)
        env.reset(seeds, observe=False)
        env.rollout_random(episodes=2)
        assert np.array_equal(env.episodes().cpu().numpy(), np.full(B, 2))
        assert np.array_equal(env.instance_index().cpu().numpy(), np.zeros(B, np.int64))
        after = R.held(env)
        assert all(np.array_equal(before[k], after[k]) for k in before)

    # on, then a new generate_instances / load_instances turn it off
    env.generate_instances(200, agents_range=ar, tasks_range=tr)
    assert setter(B) == 0
    env.generate_instances(300, agents_range=ar, tasks_range=tr)
    two_episodes_change_nothing()
    assert setter(B) == 0
    env.load_instances(**generate_batch_ranges(range(300, 300 + B), ar, tr))
    two_episodes_change_nothing()
    # a non-zero stride really is on: index 1, instance 1 with its sizes; dcm_reset does not renew
    env.generate_instances(400, agents_range=ar, tasks_range=tr)
    sz = _size_table(ar, tr, B, 400, B, n=2)
    assert setter(B) == 0
    env.reset(seeds, observe=False)
    env.rollout_random(episodes=2)
    assert np.array_equal(env.instance_index().cpu().numpy(), np.ones(B, np.int64))
    env.reset(seeds, observe=False)
    assert np.array_equal(env.instance_index().cpu().numpy(), np.ones(B, np.int64))
    held = R.held(env)
    for b in range(B):
        R.assert_instance(held, b, R.host_instance(ar, tr, 400 + b + B, 5))
    assert np.array_equal(held["n_agents"], sz[1, :, 0]) and np.array_equal(held["n_tasks"], sz[1, :, 1])
    # stride 0 after size renewals: the next two episodes stay on the held instance and sizes, index 1
    assert setter(0) == 0
    env.rollout_random(episodes=2)
    assert np.array_equal(env.instance_index().cpu().numpy(), np.ones(B, np.int64))
    after = R.held(env)
    assert all(np.array_equal(held[k], after[k]) for k in held)
    # route replay still refuses a ragged batch
    env.load_routes([[[1, 0]] * A] * B)
    with pytest.raises(DcmError):
        env.execute_routes()


def test_flagged_handle_with_a_uniform_batch_equals_an_unflagged_one(gpu_device):
    """12A/23T, uniform generated batch, renewal on: the flag changes nothing -- ring, summary, steps, held instances bit for bit."""
    from dcmrta_amd.batched_env import BatchedTaskEnv
    from dcmrta_amd.choice import env_seeds
    A, T, B, base = 12, 23, 16, 19900
    seeds = env_seeds(68, 0, B)
    out = []
    for flag in (False, True):
        env = BatchedTaskEnv(B, A, T, device=gpu_device, renew_sizes=flag)
        env.generate_instances(R.inst_seeds(base, B))
        env.set_instance_renewal(B)
        ring = env.enable_return_log(EPISODES)
        env.reset(seeds, observe=False)
        steps = env.rollout_random(episodes=EPISODES)
        assert env.instances()["n_agents"] is None
        out.append((ring.clone(), env.summary().clone(), steps.clone(), env.instance_index().clone(), R.held(env)))
    (r0, s0, n0, i0, h0), (r1, s1, n1, i1, h1) = out
    assert torch.equal(r0.view(torch.int64), r1.view(torch.int64)) and torch.equal(s0.view(torch.int64), s1.view(torch.int64))
    assert torch.equal(n0, n1) and torch.equal(i0, i1) and (i1 == EPISODES - 1).all()
    assert all(np.array_equal(h0[k], h1[k]) for k in h0)


@pytest.mark.parametrize("ar,tr,B,base,member_cap,mcs", [
    pytest.param((3, 20), (5, 50), 32, 19100, 5, 5, id="k_step-20x50-layout"),
    pytest.param((10, 64), (20, 63), 16, 19300, 5, 5, id="k_step-64x64-layout"),
    pytest.param((3, 20), (5, 50), 16, 18700, 16, 9, id="k_step-wide-9"),
])
def test_lockstep_with_a_route_log_takes_the_general_step(gpu_device, ar, tr, B, base, member_cap, mcs):
    """With the route log on (and on a wide handle) dcm_step runs the general kernel on the one-chunk layouts too: its
    size-renewing form.  Results as the chain's; and the route log holds the LAST episode's routes only -- every agent of the held
    sizes has moved, every row beyond them reads length 0, also where the env had more agents one episode earlier."""
    from dcmrta_amd.choice import env_seeds
    sz = _size_table(ar, tr, B, base, B, mcs)
    assert (sz[2, :, 0] < sz[1, :, 0]).any()                                    # rows that held a route in episode 1 and are padding now
    seeds = env_seeds(63, 0, B)
    env, ring = R.make(gpu_device, B, ar, tr, base, B, mcs, member_cap, auto_reset=True, auto_reset_episodes=EPISODES)
    env.enable_route_log(64)
    dcount = R.lockstep_to_end(env, seeds, 40)
    R.assert_after(env, ring, R.chains(ar, tr, B, base, B, seeds, mcs), dcount)
    length = env.routes()[2].cpu().numpy()
    for b in range(B):
        a = int(sz[2, b, 0])
        assert (length[b, :a] >= 1).all() and not length[b, a:].any(), (b, a, length[b].tolist())


TASK_KEYS = ("finished", "feasible", "time_start", "time_finish", "task_wait", "n_members", "n_abandoned")
AGENT_KEYS = ("travel_dist", "returned", "agent_wait")


def test_overflowed_abandonment_counts_do_not_survive_a_size_change(gpu_device):
    """max_waiting_time 3 against MAX_TIME 250: agents are abandoned more than 16 times per episode, so their counts spill into the
    dense table, which is indexed a * T + t with the env's own T and is cleared -- with the finished episode's sizes, before they
    change -- at the restart.  One call per episode; after each, every per-task and per-agent terminal quantity of the episode (the
    waiting sums are summed from that table) equals the oracle's on that episode's instance and sizes."""
    import oracle
    from dcmrta_amd import _lib
    from dcmrta_amd.choice import env_seeds
    from dcmrta_amd.instances import renewal_seeds
    oracle.build()
    ar, tr, B, base, mwt, mt = (10, 20), (30, 63), 32, 19800, 3.0, 250.0
    sz = _size_table(ar, tr, B, base, B)
    seeds = env_seeds(69, 0, B)
    env, _ = R.make(gpu_device, B, ar, tr, base, B, max_waiting_time=mwt, max_time=mt)
    env.reset(seeds, observe=False)
    d0, spilled = np.zeros(B, np.int64), np.zeros((EPISODES, B), bool)
    for k in range(EPISODES):
        steps = env.rollout_random(episodes=1).cpu().numpy()
        fin, counts = H.gpu_final(env), env.abandoned_counts().cpu().numpy().astype(np.int64)
        for b in range(B):
            A, inst = R.host_instance(ar, tr, int(renewal_seeds((base + b) % M64, k, B)), 5)
            T = inst["req"].shape[0]
            assert (A, T) == tuple(sz[k, b])
            ref = oracle.OracleEnv(A, T, max_waiting_time=mwt, max_time=mt).load(inst["depot"], inst["task_xy"], inst["req"], inst["dur"]) \
                .rollout(int(seeds[b]), int(d0[b]), oracle.POLICY_RANDOM, cap_steps=100000, record=False)
            assert steps[b] == ref["n_steps"], (k, b)
            assert not fin[b]["flags"] & _lib.FLAG_WAIT_ORDER
            got = dict(fin[b])
            got.update({key: fin[b][key][:T] for key in TASK_KEYS})
            got.update({key: fin[b][key][:A] for key in AGENT_KEYS})
            H.assert_final_matches(got, ref, f"episode {k} env {b} ({A}A/{T}T)")
            assert np.array_equal(counts[b, :A, :T].sum(axis=0), ref["n_abandoned"]) and not counts[b, A:].any() and not counts[b, :, T:].any(), (k, b)
            spilled[k, b] = (counts[b].sum(axis=1) > 16).any()
            d0[b] += ref["n_steps"]
    # the scenario really exercises the table across a size change: some env spilled in two consecutive episodes of different sizes
    both = spilled[:-1] & spilled[1:] & (sz[:-1] != sz[1:]).any(axis=2)
    assert both.any(), spilled.sum(axis=1)
