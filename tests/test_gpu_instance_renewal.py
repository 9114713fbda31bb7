"""-m gpu: instance renewal (dcm_set_instance_renewal) -- an env that restarts an episode inside a kernel first draws its next
instance, seed inst_seeds[e] + (n + 1) * stride, the way every reference Worker builds a new TaskEnv(..., seed=...) (worker.py:32).

The yardstick is the oracle (renewal_ref.oracle_chain, on oracle_ref.episodes), with a new host instance per episode:
episode k of an env loads generate_instance(A, T, seed + k * stride) and runs rollout(choice_seed, d0, POLICY_RANDOM) with the running
decision counter d0, which keeps running across instances.  Every comparison is array_equal."""
import numpy as np
import pytest
import torch

import helpers as H
import oracle_ref as O
import renewal_ref as R
from renewal_ref import EPISODES, M64

pytestmark = pytest.mark.gpu

GAMMA = 0x9E3779B97F4A7C15
ERR_STATE = -4
WRAP_STRIDE = (1 << 63) + 12345          # two of them pass 2^64


# shape, batch, member_cap / max_coalition_size, stride (None = B), base seed: one case per kernel class of dcm_rollout_random
ROLLOUT_CASES = [
    pytest.param(20, 50, 32, 5, 5, None, 8100, id="20A50T-exact"),
    pytest.param(12, 23, 32, 5, 5, WRAP_STRIDE, (1 << 63) + 77, id="12A23T-runtime-sizes-wrap"),
    pytest.param(64, 63, 16, 5, 5, None, 8300, id="64A63T"),
    pytest.param(50, 200, 8, 5, 5, None, 8400, id="50A200T-fast-mc"),
    pytest.param(70, 130, 8, 5, 5, None, 8500, id="70A130T-fast-g"),
    pytest.param(100, 300, 4, 5, 5, None, 8600, id="100A300T-general"),
    pytest.param(20, 50, 16, 16, 9, None, 8700, id="20A50T-wide-9"),
    pytest.param(4, 700, 2, 5, 5, None, 8800, id="4A700T-general-above-64KiB"),   # a launch that needs the raised dynamic-LDS limit
]


@pytest.mark.parametrize("A,T,B,member_cap,mcs,stride,base", ROLLOUT_CASES)
def test_persistent_rollout_plays_a_new_instance_every_episode(gpu_device, A, T, B, member_cap, mcs, stride, base):
    from dcmrta_amd.choice import env_seeds
    stride = B if stride is None else stride
    seeds = env_seeds(51, 0, B)
    env, ring = R.make(gpu_device, B, A, T, base, stride, mcs, member_cap)
    if T == 700:
        assert env.record_bytes() > 65536
    env.reset(seeds, observe=False)
    steps = env.rollout_random(episodes=EPISODES).cpu().numpy()
    R.assert_after(env, ring, R.chains(A, T, B, base, stride, seeds, mcs), steps)


def test_machine_filling_launch_renews_too(gpu_device):
    """B = 4096 in one launch: the wave-priority instantiation of the one-chunk kernel.  A fixed sample of 64 envs is compared."""
    from dcmrta_amd.choice import env_seeds
    A, T, B, base = 20, 50, 4096, 9000
    seeds = env_seeds(52, 0, B)
    env, ring = R.make(gpu_device, B, A, T, base, B)
    env.reset(seeds, observe=False)
    steps = env.rollout_random(episodes=EPISODES).cpu().numpy()
    rows = [int(b) for b in np.arange(64) * 64 + (np.arange(64) * 37) % 64]
    R.assert_after(env, ring, R.chains(A, T, B, base, B, seeds, rows=rows), steps, rows)
    assert np.array_equal(env.instance_index().cpu().numpy(), np.full(B, EPISODES - 1))


def test_split_calls_give_the_same_results(gpu_device):
    """Three calls of one episode; a per-env budget that stops mid-episode, then a call that finishes; a budget that runs out exactly
    at an episode boundary leaves index and instance unrenewed until the next call.  Same arrays as the single call (same chains)."""
    from dcmrta_amd.choice import env_seeds
    A, T, B, base = 20, 50, 32, 8100
    seeds = env_seeds(51, 0, B)
    chains = R.chains(A, T, B, base, B, seeds)
    n0 = np.array([chains[b][0][0]["n_steps"] for b in range(B)], np.int64)
    n1 = np.array([chains[b][0][1]["n_steps"] for b in range(B)], np.int64)
    # three calls of one episode each
    env, ring = R.make(gpu_device, B, A, T, base, B)
    env.reset(seeds, observe=False)
    steps = sum(env.rollout_random(episodes=1).cpu().numpy() for _ in range(EPISODES))
    R.assert_after(env, ring, chains, steps)
    # a budget that ends in the middle of episode 1 (every env its own), then the rest: the pending episode counts as one
    env, ring = R.make(gpu_device, B, A, T, base, B)
    env.reset(seeds, observe=False)
    s1 = env.rollout_random(episodes=EPISODES, max_decisions=n0 + n1 // 2).cpu().numpy()
    assert np.array_equal(s1, n0 + n1 // 2)
    assert np.array_equal(env.instance_index().cpu().numpy(), np.ones(B, np.int64))
    s2 = env.rollout_random(episodes=2).cpu().numpy()
    R.assert_after(env, ring, chains, s1 + s2)
    # a budget that runs out exactly at the end of episode 0: the finished episode's instance and results stay
    env, ring = R.make(gpu_device, B, A, T, base, B)
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


@pytest.mark.parametrize("A,T,B,base,read_every", [
    pytest.param(20, 50, 96, 9100, 40, id="20A50T-deferred-terminal"),
    pytest.param(20, 50, 96, 9100, 0, id="20A50T-summaries-read-at-the-end"),
    pytest.param(64, 63, 16, 9300, 40, id="64A63T"),
    pytest.param(50, 200, 8, 9400, 40, id="50A200T-general-k_step"),
    pytest.param(4, 700, 2, 8800, 40, id="4A700T-general-k_step-above-64KiB"),
])
def test_lockstep_auto_reset_renews(gpu_device, A, T, B, base, read_every):
    from dcmrta_amd.choice import env_seeds
    seeds = env_seeds(53, 0, B)
    env, ring = R.make(gpu_device, B, A, T, base, B, auto_reset=True, auto_reset_episodes=EPISODES)
    if T == 700:
        assert env.record_bytes() > 65536
    dcount = R.lockstep_to_end(env, seeds, read_every)
    R.assert_after(env, ring, R.chains(A, T, B, base, B, seeds), dcount)
    assert np.array_equal(env.status()["decisions"].cpu().numpy(), dcount)


def test_lockstep_auto_reset_renews_with_individual_selection(gpu_device, oracle_lib):
    """DCM_PARAM_NO_GROUPING (the general k_step): Worker.run_test_IS restated on the oracle's step-wise surface as
    test_gpu_api.test_individual_selection_mode does, with the first valid action, on a new host instance per episode."""
    from dcmrta_amd.choice import env_seeds
    from dcmrta_amd.instances import renewal_seeds
    A, T, B, base = 20, 50, 96, 9500
    seeds = env_seeds(54, 0, B)
    env, ring = R.make(gpu_device, B, A, T, base, B, auto_reset=True, auto_reset_episodes=EPISODES, individual_selection=True)
    dcount = R.lockstep_to_end(env, seeds, 40, policy=lambda obs: torch.argmax((~obs.mask).to(torch.int32), dim=1).to(torch.int32))
    sm, rl, idx, held = env.summary().cpu().numpy(), ring.cpu().numpy(), env.instance_index().cpu().numpy(), R.held(env)
    for b in range(B):
        total, rows = 0, []
        for k in range(EPISODES):
            sized = R.host_instance(A, T, int(renewal_seeds((base + b) % M64, k, B)), 5)
            inst = sized[1]
            o = oracle_lib.OracleEnv(A, T).load(inst["depot"], inst["task_xy"], inst["req"], inst["dur"])
            finished, guard = False, 0
            while not finished and o.now < 100:                                  # worker.py:163
                ids, t = o.next_decision()                                       # :165
                o.now = t                                                        # :167
                o.task_update(); o.agent_update()                                # :168-169
                for a in ids:                                                    # :170
                    o.agent_step(int(a), int(np.flatnonzero(o.mask() == 0)[0]))  # :175-186
                    o.task_update(); o.agent_update()                            # :187-188
                    total += 1
                finished = o.check_finished()                                    # :189
                guard += 1
                assert guard < 5000
            oracle_lib.lib().orc_finish_episode(o._h)
            ref = o.final()
            rows.append(O.summary_row(ref))
        assert np.array_equal(rl[b], np.array([r[0] for r in rows])), b
        assert np.array_equal(sm[b], rows[-1], equal_nan=True), b
        assert idx[b] == EPISODES - 1 and dcount[b] == total, b
        R.assert_instance(held, b, sized)


def test_first_observation_after_a_renewal_is_the_new_instances(gpu_device):
    """The dcm_step that ends episode 0 returns the first decision of episode 1: it must equal observe() of a handle that was GIVEN
    instance 1 and reset with the choice seed seed + GAMMA * d (d = the env's decisions so far), which has the same keys (choice.py)."""
    from dcmrta_amd.batched_env import BatchedTaskEnv
    from dcmrta_amd.choice import env_seeds
    A, T, B, base = 20, 50, 64, 9600
    seeds = env_seeds(55, 0, B)
    env, _ = R.make(gpu_device, B, A, T, base, B, auto_reset=True, auto_reset_episodes=2)
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
    twin = BatchedTaskEnv(B, A, T, device=gpu_device).generate_instances(R.inst_seeds(base + B, B))
    tobs = twin.reset(np.array([(int(seeds[b]) + GAMMA * got[b][0]) % M64 for b in range(B)], dtype=np.uint64))
    ta, tt, tm, tl = tobs.agents.cpu().numpy(), tobs.tasks.cpu().numpy(), tobs.mask.cpu().numpy(), tobs.leader.cpu().numpy()
    for b in range(B):
        _, ag, tk, mk, ld = got[b]
        assert np.array_equal(ag, ta[b]) and np.array_equal(tk, tt[b]) and np.array_equal(mk, tm[b]) and ld == tl[b], b


def test_renewal_turned_off_after_renewals_restarts_from_the_held_instance(gpu_device):
    """Lockstep with auto-reset and deferred summaries (read at the end only), renewal on until every env holds an instance of index
    >= 1; then stride 0, and the stepping goes on through the remaining episode ends.  From there on an env restarts from the
    instance it holds -- all of it: the restart image that dcm_reset took describes instance 0 and must not come back.  Returns,
    final summary row, index, held instance and decision count equal the oracle's on instances 0..n, n, .. (n = index at the switch)."""
    from dcmrta_amd.choice import env_seeds
    A, T, B, base = 20, 50, 32, 9800
    seeds = env_seeds(58, 0, B)
    env, ring = R.make(gpu_device, B, A, T, base, B, auto_reset=True, auto_reset_episodes=EPISODES)
    obs = env.reset(seeds)
    dcount, at_switch = np.zeros(B, np.int64), None
    for s in range(4001):
        active = obs.active.cpu().numpy()
        if not active.any():
            break
        assert s < 4000, "envs still active after 4000 steps"
        mk = obs.mask.cpu().numpy().astype(np.uint8)
        act = np.array([H.host_random_action(mk[b], int(seeds[b]), int(dcount[b])) if active[b] else 0 for b in range(B)], np.int32)
        obs = env.step(act)
        dcount += active
        if at_switch is None:
            idx = env.instance_index().cpu().numpy()
            if (idx >= 1).all():
                at_switch = idx
                env.set_instance_renewal(0)
    assert at_switch is not None and (at_switch < EPISODES - 1).any()        # episodes do end after the switch
    sm, rl, idx, held = env.summary().cpu().numpy(), ring.cpu().numpy(), env.instance_index().cpu().numpy(), R.held(env)
    assert np.array_equal(env.episodes().cpu().numpy(), np.full(B, EPISODES))
    assert np.array_equal(idx, at_switch)
    for b in range(B):
        n = int(at_switch[b])
        eps, insts = R.oracle_chain(A, T, (base + b) % M64, B, int(seeds[b]), indices=tuple(min(k, n) for k in range(EPISODES)))
        assert np.array_equal(rl[b], np.array([e["row"][0] for e in eps])), b
        assert np.array_equal(sm[b], eps[-1]["row"], equal_nan=True), b
        R.assert_instance(held, b, insts[-1])
        assert dcount[b] == sum(e["n_steps"] for e in eps), b


def test_clone_and_restore_carry_index_and_instance(gpu_device):
    from dcmrta_amd.choice import env_seeds
    A, T, B, base = 20, 50, 16, 8100
    seeds = env_seeds(51, 0, B)
    chains = R.chains(A, T, B, base, 32, seeds)                     # (the first 16 envs of the B = 32 case: stride 32)
    env, ring = R.make(gpu_device, B, A, T, base, 32)
    env.reset(seeds, observe=False)
    s0 = env.rollout_random(episodes=1, max_decisions=20).cpu().numpy()          # in episode 0
    snap = env.clone_state()
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
    from dcmrta_amd.instances import generate_batch
    A, T, B = 12, 23, 8
    seeds = env_seeds(56, 0, B)
    env = BatchedTaskEnv(B, A, T, device=gpu_device)
    setter = lambda stride: env._lib.dcm_set_instance_renewal(env._h, stride)

    def two_episodes_change_nothing():
        before = R.held(env)
        env.reset(seeds, observe=False)
        env.rollout_random(episodes=2)
        assert np.array_equal(env.episodes().cpu().numpy(), np.full(B, 2))
        assert np.array_equal(env.instance_index().cpu().numpy(), np.zeros(B, np.int64))
        after = R.held(env)
        assert all(np.array_equal(before[k], after[k]) for k in before)

    # refused after load_instances, and on a batch generated with a real range; stride 0 is always accepted
    env.load_instances(**generate_batch(B, A, T, base_seed=1))
    assert setter(B) == ERR_STATE and b"dcm_set_instance_renewal" in env._lib.dcm_last_error()
    assert setter(0) == 0
    with pytest.raises(DcmError):
        env.set_instance_renewal(B)
    two_episodes_change_nothing()
    env.generate_instances(100, agents_range=(6, A), tasks_range=(10, T))
    assert setter(B) == ERR_STATE
    env.generate_instances(100, tasks_range=(10, T))
    assert setter(B) == ERR_STATE
    # never set: three episodes on the same instance
    env.generate_instances(100)
    before = R.held(env)
    env.reset(seeds, observe=False)
    env.rollout_random(episodes=3)
    assert np.array_equal(env.instance_index().cpu().numpy(), np.zeros(B, np.int64))
    assert all(np.array_equal(before[k], v) for k, v in R.held(env).items())
    # on, then a new generate_instances / load_instances turn it off
    assert setter(B) == 0
    env.generate_instances(200)
    two_episodes_change_nothing()
    assert setter(B) == 0
    env.load_instances(**generate_batch(B, A, T, base_seed=2))
    two_episodes_change_nothing()
    # stride 0 after a non-zero stride turns it off; a non-zero stride really is on
    env.generate_instances(300)
    assert setter(B) == 0 and setter(0) == 0
    two_episodes_change_nothing()
    assert setter(B) == 0
    env.reset(seeds, observe=False)
    env.rollout_random(episodes=2)
    assert np.array_equal(env.instance_index().cpu().numpy(), np.ones(B, np.int64))
    # dcm_reset does not renew and leaves the index alone
    env.reset(seeds, observe=False)
    assert np.array_equal(env.instance_index().cpu().numpy(), np.ones(B, np.int64))
    held = R.held(env)
    for b in range(B):
        R.assert_instance(held, b, R.host_instance(A, T, 300 + b + B, 5))
    # stride 0 after renewals have happened: the next two episodes stay on the held instance, index 1
    assert setter(0) == 0
    env.rollout_random(episodes=2)
    assert np.array_equal(env.instance_index().cpu().numpy(), np.ones(B, np.int64))
    after = R.held(env)
    assert all(np.array_equal(held[k], after[k]) for k in held)
    # load_instances and generate_instances zero an index that was not 0
    env.load_instances(**generate_batch(B, A, T, base_seed=3))
    assert np.array_equal(env.instance_index().cpu().numpy(), np.zeros(B, np.int64))
    env.generate_instances(400)
    assert setter(B) == 0
    env.reset(seeds, observe=False)
    env.rollout_random(episodes=2)
    assert np.array_equal(env.instance_index().cpu().numpy(), np.ones(B, np.int64))
    env.generate_instances(500)
    assert np.array_equal(env.instance_index().cpu().numpy(), np.zeros(B, np.int64))


def test_captured_step_loop_renews_like_the_eager_loop(gpu_device):
    from dcmrta_amd.choice import env_seeds
    from dcmrta_amd.graph_rollout import GraphedRollout
    A, T, B, base = 20, 50, 64, 9700
    seeds = env_seeds(57, 0, B)
    policy = lambda obs: torch.argmax((~obs.mask).to(torch.int32), dim=1).to(torch.int32)
    eager, ering = R.make(gpu_device, B, A, T, base, B, auto_reset=True, auto_reset_episodes=EPISODES)
    R.lockstep_to_end(eager, seeds, policy=policy)
    env, ring = R.make(gpu_device, B, A, T, base, B, auto_reset=True, auto_reset_episodes=EPISODES)
    GraphedRollout(env, policy, check_every=8).run(seeds, max_steps=4000)
    assert np.array_equal(env.episodes().cpu().numpy(), np.full(B, EPISODES))
    assert np.array_equal(ring.cpu().numpy(), ering.cpu().numpy())
    assert np.array_equal(env.summary().cpu().numpy(), eager.summary().cpu().numpy(), equal_nan=True)
    assert np.array_equal(env.instance_index().cpu().numpy(), np.full(B, EPISODES - 1))
    a, b = R.held(env), R.held(eager)
    assert all(np.array_equal(a[k], b[k]) for k in a)
    # ... and the eager loop's returns differ from episode to episode, i.e. the instances really changed
    assert not np.array_equal(ering.cpu().numpy()[:, 0], ering.cpu().numpy()[:, 1])
