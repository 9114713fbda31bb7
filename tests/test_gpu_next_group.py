"""The NEXT-GROUP step of the persistent rollout kernels (worker.py:52: an event whose deciding agents stand at several
locations is served group by group) and the wave reductions behind their event times, on instances that exercise them.

Under the random policy ordinary instances almost never produce an event with several groups, so the parity runs on generated
instances hardly reach the line that advances cur_group.  Mirror-symmetric instances do: the depot in the centre, tasks in
quadruples (0.5 +- a, 0.5 +- b), every requirement 1 and one common duration, so agents that left together for the members of a
quadruple arrive, finish and decide again at the same instant at different places.  Offsets are multiples of 2^-10: 0.5 +- a is
exact in fp64 and the mirrored distances are bit-equal.

One shape per kernel and reduction width, each compared with the oracle bit for bit: decisions per env, every episode's return,
summary(), and the per-decision outputs at a stop right behind a next-group step.  That every env's inputs contain such steps is
asserted from the oracle's trace (a test of its own, without a GPU): consecutive decisions with equal `now` and a different leader
position (row 0 of tasks_obs holds depot - leader position)."""
import functools

import numpy as np
import pytest

import helpers as H
import oracle_ref as O

DUR = 2.0
#        A,  T,  env's sizes (None: the handle's own), B     kernel, reduction
SHAPES = [(20, 50, None, 16),       # Fast<20,50>, wave_nanmin_n<20>
          (20, 50, (17, 20), 16),   # runtime sizes in the <20,50> layout; agents in lanes 16+ need the row_bcast:15 stage
          (64, 63, None, 16),       # Fast<64,64>: full-wave reduction, rows 2-3
          (50, 200, None, 6),       # k_rollout_fast_mc
          (70, 130, None, 6)]       # k_rollout_fast_g


def mirror_batch(B, A, T, seed):
    """B mirror-symmetric instances of T tasks (see the module docstring); a last incomplete quadruple keeps its first members."""
    rng = np.random.default_rng(seed)
    nq = (T + 3) // 4
    task_xy = np.empty((B, T, 2), np.float64)
    for b in range(B):
        # distinct (a, b) per quadruple, multiples of 2^-10 in (0, 0.5)
        ab = rng.choice(500 * 500, size=nq, replace=False)
        a, c = (ab // 500 + 1) / 1024.0, (ab % 500 + 1) / 1024.0
        quad = np.stack([np.stack([0.5 + sx * a, 0.5 + sy * c], -1) for sx, sy in ((1, 1), (-1, -1), (-1, 1), (1, -1))], 1)
        task_xy[b] = quad.reshape(-1, 2)[:T]
    return dict(depot=np.full((B, 2), 0.5), task_xy=task_xy, req=np.ones((B, T), np.int32), dur=np.full((B, T), DUR))


def next_group_steps(ref):
    """indices k such that decision k+1 is the first of the next group of the same event"""
    now, pos = ref["now"], ref["tasks_obs"][:, 0, 3:5]
    return np.flatnonzero((now[1:] == now[:-1]) & (pos[1:] != pos[:-1]).any(axis=1))


@functools.lru_cache(maxsize=None)
def references(oracle_lib, A, T, sizes, B):
    """(instances, seeds, first-episode traces, second-episode results) of a shape: computed once, read-only afterwards"""
    from dcmrta_amd.choice import env_seeds
    inst, seeds = mirror_batch(B, A, T, seed=1000 * A + T + (7 if sizes else 0)), env_seeds(52, 0, B)
    return (inst, seeds) + O.two_episodes(inst, seeds, *(sizes or (A, T)))


@pytest.mark.parametrize("A,T,sizes,B", SHAPES)
def test_inputs_contain_next_group_steps(oracle_lib, A, T, sizes, B):
    """The condition of the comparison below, from the oracle's trace on the CPU: every env takes next-group steps."""
    _, _, ep1, _ = references(oracle_lib, A, T, sizes, B)
    counts = [len(next_group_steps(r)) for r in ep1]
    print(f"{A}A/{T}T sizes {sizes}: next-group steps {sum(counts)} of {sum(r['n_steps'] for r in ep1)} decisions, per env {counts}")
    assert min(counts) >= 1, counts


@pytest.mark.gpu
@pytest.mark.parametrize("A,T,sizes,B", SHAPES)
def test_mirror_instances_against_the_oracle(gpu_device, oracle_lib, A, T, sizes, B):
    inst, seeds, ep1, ep2 = references(oracle_lib, A, T, sizes, B)
    a, t = sizes or (A, T)
    tag = f"{A}A/{T}T sizes {sizes}"
    assert min(len(next_group_steps(r)) for r in ep1) >= 1
    n1 = np.array([r["n_steps"] for r in ep1], np.int64)
    n2 = np.array([r["n_steps"] for r in ep2], np.int64)
    # two episodes in one launch: decisions, both returns, summary() of the second
    env = H.sized_env(gpu_device, A, T, inst, sizes)
    ring = env.enable_return_log(2)
    env.reset(seeds, observe=False)
    steps = env.rollout_random(episodes=2).cpu().numpy()
    got, sm = ring.cpu().numpy(), env.summary().cpu().numpy()
    assert np.array_equal(steps, n1 + n2), (tag, steps, n1 + n2)
    for b in range(B):
        assert got[b, 0] == ep1[b]["reward"] and got[b, 1] == ep2[b]["reward"], (tag, b, got[b], ep1[b]["reward"], ep2[b]["reward"])
        O.assert_summary(sm[b], ep2[b], f"{tag} env{b} episode 2")
    # stop right behind a next-group step (the one nearest to the middle of the episode): the last decision taken is the first of
    # the new group, and what the kernel stored for it is the oracle's record of it
    env.enable_return_log(0)
    env.reset(seeds, observe=False)
    at = np.empty(B, np.int64)
    for b, r in enumerate(ep1):
        ks = next_group_steps(r)
        at[b] = ks[np.argmin(np.abs(ks - r["n_steps"] // 2))] + 2
    steps = env.rollout_random(episodes=1, max_decisions=at).cpu().numpy()
    assert np.array_equal(steps, at), (tag, steps, at)
    obs = env.obs()
    ag, tk, mk = (x.clone().cpu().numpy() for x in (obs.agents, obs.tasks, obs.mask))
    st = {k: v.cpu().numpy() for k, v in env.status().items()}
    for b, r in enumerate(ep1):
        k, name = int(at[b]) - 1, f"{tag} env{b} decision {int(at[b]) - 1}"
        assert np.array_equal(ag[b, :a], r["agents_obs"][k]), name + ": agents observation"
        assert np.array_equal(tk[b, :t + 1], r["tasks_obs"][k]), name + ": tasks observation"
        assert np.array_equal(mk[b, :t + 1].astype(np.uint8), r["mask"][k]), name + ": mask"
        assert st["decisions"][b] == k + 1, name + ": decision counter"
    # the state it left: the pending decision through dcm_observe
    o2 = env.observe()
    ag2, tk2, mk2, ld2, act2 = (x.cpu().numpy() for x in (o2.agents, o2.tasks, o2.mask, o2.leader, o2.active))
    for b, r in enumerate(ep1):
        k, name = int(at[b]), f"{tag} env{b} pending decision {int(at[b])}"
        if k >= r["n_steps"]:
            assert not act2[b] and (st["flags"][b] & 1), name + ": episode must be over"
            continue
        assert act2[b] and st["now"][b] == r["now"][k] and ld2[b] == r["leader"][k], name + ": time / leader"
        assert np.array_equal(ag2[b, :a], r["agents_obs"][k]) and np.array_equal(tk2[b, :t + 1], r["tasks_obs"][k]), name
        assert np.array_equal(mk2[b, :t + 1].astype(np.uint8), r["mask"][k]), name
    # ... and the rest of the episode
    live = at < n1
    steps = env.rollout_random(episodes=1, max_decisions=np.where(live, -1, 0).astype(np.int64)).cpu().numpy()
    assert np.array_equal(steps, n1 - at), (tag, steps, n1 - at)
    sm = env.summary().cpu().numpy()
    for b in range(B):
        O.assert_summary(sm[b], ep1[b], f"{tag} env{b} episode 1 after the stop")


@pytest.mark.gpu
def test_full_machine_launch_on_mirror_instances(gpu_device, oracle_lib):
    """4096 envs at 20A/50T: the launch that fills the machine runs the wave-priority instantiation of the kernel."""
    from dcmrta_amd.choice import env_seeds
    B, A, T = 4096, 20, 50
    inst = mirror_batch(B, A, T, seed=99)
    seeds = env_seeds(53, 0, B)
    env = H.sized_env(gpu_device, A, T, inst)
    env.reset(seeds, observe=False)
    steps = env.rollout_random(episodes=1).cpu().numpy()
    sm = env.summary().cpu().numpy()
    for b in range(B):
        ref = O.episodes(A, T, O.one(inst, b), seeds[b], "random", 1)[0]
        assert steps[b] == ref["n_steps"], (b, steps[b], ref["n_steps"])
        O.assert_summary(sm[b], ref, f"env{b} of 4096")
