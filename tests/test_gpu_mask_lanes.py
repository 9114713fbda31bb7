"""The lane predicates of the register-resident kernels as wave-uniform masks (common.hpp, lane_of), where a wrong mask shows.

Fast<> carries its predicates -- open tasks, status <= 0, ok, the leavers, becomes-feasible, the members of a step, the `gone`
agents of a dropping task -- as masks and combines them on the scalar unit; lanes that own no task hold a copy of task 0's words, so
every mask that decides anything must pass through tm / am.  Where that can go wrong:
  (20, 50) uniform;
  (20, 50) with per-env sizes (17, 20): lanes 20-49 hold copies of task 0, agents in lanes 16+;
  (64, 63): am all ones, bit 63 shared by agent 63 and the depot lane, tm of 63 bits;
  (5, 8).
(The multi-chunk kernels k_rollout_fast_mc / k_rollout_fast_g keep their text: no shape of theirs here.)

max_waiting_time 10.0 (the reference's) and 2.0: at 2.0 every env abandons many times, so the removal path and the walk over the
dropping tasks' `gone` masks run at most decisions -- asserted from the oracle on the CPU.  Each case is compared with the oracle bit
for bit: decisions per env, both episodes' returns, summary(), the observation and mask tensors of the decision at a stop in the
middle of the first episode -- through rollout_random (k_rollout_fast) and through the lockstep step loop (k_step_fast runs the same
Fast<> text), whose every decision's observation is compared."""
import functools

import numpy as np
import pytest

import helpers as H
import oracle_ref as O

B = 16
#        A,  T,  env's sizes (None: the handle's own)
SHAPES = [(20, 50, None), (20, 50, (17, 20)), (64, 63, None), (5, 8, None)]
MWTS = [10.0, 2.0]
CASES = [(A, T, s, w) for A, T, s in SHAPES for w in MWTS]


@functools.lru_cache(maxsize=None)
def references(oracle_lib, A, T, sizes, mwt):
    """(instances, seeds, first-episode traces, second-episode results): computed once per case, read-only afterwards"""
    from dcmrta_amd.choice import env_seeds
    from dcmrta_amd.instances import generate_batch
    inst, seeds = generate_batch(B, A, T, base_seed=7), env_seeds(3, 0, B)
    return (inst, seeds) + O.two_episodes(inst, seeds, *(sizes or (A, T)), mwt)


def abandonments(ep1):
    """per env: appends to an abandoned_agent list in the first episode"""
    return [int(r["n_abandoned"].sum()) for r in ep1]


@pytest.mark.parametrize("A,T,sizes,mwt", CASES)
def test_inputs_run_the_removal_path(oracle_lib, A, T, sizes, mwt):
    """The condition of the comparisons below, from the oracle on the CPU.  max_waiting_time 2.0: every env abandons at least 10
    times in its first episode (minima 202 / 16 / 42 / 14 in the order of SHAPES).  10.0: small shapes have envs without a removal,
    the batch's total is above zero."""
    _, _, ep1, _ = references(oracle_lib, A, T, sizes, mwt)
    counts = abandonments(ep1)
    print(f"{A}A/{T}T sizes {sizes} max_waiting_time {mwt}: abandonments per env min {min(counts)} total {sum(counts)}, "
          f"mean decisions per episode {np.mean([r['n_steps'] for r in ep1]):.0f}")
    if mwt == 2.0:
        assert min(counts) >= 10, counts
    else:
        assert sum(counts) > 0, counts


@pytest.mark.gpu
@pytest.mark.parametrize("A,T,sizes,mwt", CASES)
def test_rollout_against_the_oracle(gpu_device, oracle_lib, A, T, sizes, mwt):
    inst, seeds, ep1, ep2 = references(oracle_lib, A, T, sizes, mwt)
    a, t = sizes or (A, T)
    tag = f"{A}A/{T}T sizes {sizes} mwt {mwt}"
    n1 = np.array([r["n_steps"] for r in ep1], np.int64)
    n2 = np.array([r["n_steps"] for r in ep2], np.int64)
    # two episodes in one launch: decisions, both returns, summary() of the second
    env = H.sized_env(gpu_device, A, T, inst, sizes, max_waiting_time=mwt)
    ring = env.enable_return_log(2)
    env.reset(seeds, observe=False)
    steps = env.rollout_random(episodes=2).cpu().numpy()
    got, sm = ring.cpu().numpy(), env.summary().cpu().numpy()
    assert np.array_equal(steps, n1 + n2), (tag, steps, n1 + n2)
    for b in range(B):
        assert got[b, 0] == ep1[b]["reward"] and got[b, 1] == ep2[b]["reward"], (tag, b, got[b], ep1[b]["reward"], ep2[b]["reward"])
        O.assert_summary(sm[b], ep2[b], f"{tag} env{b} episode 2")
    # a stop in the middle of the first episode: what the kernel stored for the last decision taken is the oracle's record of it
    env.enable_return_log(0)
    env.reset(seeds, observe=False)
    at = np.maximum(n1 // 2, 1)
    steps = env.rollout_random(episodes=1, max_decisions=at).cpu().numpy()
    assert np.array_equal(steps, at), (tag, steps, at)
    obs = env.obs()
    ag, tk, mk = (x.clone().cpu().numpy() for x in (obs.agents, obs.tasks, obs.mask))
    for b, r in enumerate(ep1):
        k, name = int(at[b]) - 1, f"{tag} env{b} decision {int(at[b]) - 1}"
        assert np.array_equal(ag[b, :a], r["agents_obs"][k]), name + ": agents observation"
        assert np.array_equal(tk[b, :t + 1], r["tasks_obs"][k]), name + ": tasks observation"
        assert np.array_equal(mk[b, :t + 1].astype(np.uint8), r["mask"][k]), name + ": mask"
    # ... and the rest of the episode
    steps = env.rollout_random(episodes=1, max_decisions=np.where(at < n1, -1, 0).astype(np.int64)).cpu().numpy()
    assert np.array_equal(steps, n1 - at), (tag, steps, n1 - at)
    sm = env.summary().cpu().numpy()
    for b in range(B):
        O.assert_summary(sm[b], ep1[b], f"{tag} env{b} episode 1 after the stop")
    env.close()


@pytest.mark.gpu
@pytest.mark.parametrize("A,T,sizes,mwt", CASES)
def test_lockstep_against_the_oracle(gpu_device, oracle_lib, A, T, sizes, mwt):
    """The same first episode decision by decision through step(): the protocol's random action from the mask the kernel returned"""
    inst, seeds, ep1, _ = references(oracle_lib, A, T, sizes, mwt)
    a, t = sizes or (A, T)
    tag = f"lockstep {A}A/{T}T sizes {sizes} mwt {mwt}"
    env = H.sized_env(gpu_device, A, T, inst, sizes, max_waiting_time=mwt)
    got = H.run_lockstep(env, seeds, lambda b, i, m, l: H.host_random_action(m[:t + 1], int(seeds[b]), i))
    sm = env.summary().cpu().numpy()
    for b, r in enumerate(ep1):
        g, name = got[b], f"{tag} env{b}"
        assert g["n_steps"] == r["n_steps"], (name, g["n_steps"], r["n_steps"])
        for k in ("leader", "action", "now"):
            assert np.array_equal(g[k], r[k]), f"{name}: {k}"
        assert np.array_equal(g["mask"][:, :t + 1], r["mask"]), name + ": mask"
        assert np.array_equal(g["agents_obs"][:, :a], r["agents_obs"]), name + ": agents observation"
        assert np.array_equal(g["tasks_obs"][:, :t + 1], r["tasks_obs"]), name + ": tasks observation"
        O.assert_summary(sm[b], r, name)
    env.close()
