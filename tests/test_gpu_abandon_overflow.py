"""The abandonment log past its sixteen entries (Fast<>::task_update: the log's store is the one arm under the dropped lanes' own
predicate, the count table's atomic sits behind one wave-uniform test of the lanes past AB_CAP) against the oracle.

32 envs of 2A/3T, every requirement 3 -- two agents never complete a coalition -- and max_waiting_time 0.02: an agent waits, is dropped
by the waiting rule (env/task_env.py:268-271), decides again, and so on to MAX_TIME: dozens of abandonments per agent and episode,
the seventeenth and later ones of an agent counted in the dense table (at 0.02 every first episode is longer than the 60 decisions
compared one by one: 65 at the least; at 0.5 some end after 40).  The instances are generate_batch's with the requirements
replaced; the oracle is walked with its step-wise API (removal_ref.walk_episode), and the condition that makes the case real -- in
at least a quarter of the envs an agent is past AB_CAP within the decisions compared -- is checked on that walk alone.

On the GPU: the persistent kernel one decision per launch (a budget of 1) for the first 60 decisions, after each of which the member
lists, the abandonment counts per (agent, task) -- log and count table together, dcm_get_abandoned -- the tasks' state, the
observation and the agents' side are compared with the walk (removal_ref.assert_handover); and one launch of two full episodes:
decisions, both returns, summary() and the second episode's abandonment counts."""
import numpy as np
import pytest

import oracle_ref as O
from removal_ref import MAX_TIME, Lists, assert_handover, read_batch, sparse_abandoned, walk_episode

A, T, B, MWT = 2, 3, 32, 0.02
AB_CAP = 16                 # entries of an agent's abandonment log (csrc/common.hpp); further ones go to the count table
DECISIONS = 60

_ref = {}


def ref():
    """(instances, seeds, per-env snapshots of the first episode, per-env [first, second] episode results, per-env abandonment counts
    [A, T] of the second episode): computed once, read-only afterwards"""
    if not _ref:
        import oracle
        from dcmrta_amd.choice import env_seeds
        from dcmrta_amd.instances import generate_batch
        oracle.build()
        inst = generate_batch(B, A, T, base_seed=41)
        inst["req"] = np.full((B, T), 3, np.int32)
        seeds = env_seeds(9, 0, B)
        snaps, eps, ab2 = [], [], []
        for b in range(B):
            one = O.one(inst, b)
            o = oracle.OracleEnv(A, T, max_waiting_time=MWT, max_time=MAX_TIME).load(one["depot"], one["task_xy"], one["req"], one["dur"])
            snaps.append(sparse_abandoned(walk_episode(o, inst["req"][b], int(seeds[b]))[0]))
            eps.append(O.episodes(A, T, one, seeds[b], "random", 2, MWT))
            o2, k2, ended = O.play(A, T, one, seeds[b], eps[b][0]["n_steps"], "random", None, MWT)
            assert ended and k2 == eps[b][1]["n_steps"]
            ab2.append(np.stack([np.bincount(o2.abandoned(t), minlength=A)[:A] for t in range(T)], axis=1))
        _ref.update(inst=inst, seeds=seeds, snaps=snaps, eps=eps, ab2=ab2)
    return _ref


def _most(s):
    """the largest number of abandonments of one agent in a snapshot"""
    idx, val = s["abandoned"]
    return int(np.bincount(idx // T, val, minlength=A).max()) if len(idx) else 0


def test_the_case_is_real():
    """From the oracle alone: the walk is the oracle's own episode, and in at least a quarter of the envs an agent is past AB_CAP
    abandonments in front of decision 60 -- so the decisions compared one by one cross the log's end -- and in every env by the end of
    the second episode"""
    r = ref()
    for b in range(B):
        assert len(r["snaps"][b]) == r["eps"][b][0]["n_steps"] > DECISIONS, b
    early = sum(1 for s in r["snaps"] if _most(s[DECISIONS]) > AB_CAP)
    late = sum(1 for ab in r["ab2"] if ab.sum(axis=1).max() > AB_CAP)
    print("envs past AB_CAP in front of decision", DECISIONS, ":", early, "of", B, "; in the second episode:", late)
    assert 4 * early >= B and 4 * late >= B, (early, late)


def _env(gpu_device):
    from dcmrta_amd.batched_env import BatchedTaskEnv
    env = BatchedTaskEnv(B, A, T, device=gpu_device, max_waiting_time=MWT).load_instances(**ref()["inst"])
    assert env.kernel_name() == "k_rollout_fast"
    return env


@pytest.mark.gpu
def test_after_every_decision_of_budget_one_launches(gpu_device):
    r = ref()
    env = _env(gpu_device)
    env.reset(r["seeds"], observe=False)
    lists = [Lists(T, 5) for _ in range(B)]
    for d in range(1, DECISIONS + 1):
        steps = env.rollout_random(episodes=1, max_decisions=1).cpu().numpy()
        assert np.all(steps == 1), d
        got = read_batch(env)
        for b in range(B):
            assert_handover(f"env {b} behind decision {d - 1}", got, b, d, r["snaps"][b], lists[b], A, T, O.one(r["inst"], b), r["seeds"][b], MWT)
    env.close()


@pytest.mark.gpu
def test_two_episodes_in_one_launch(gpu_device):
    r = ref()
    env = _env(gpu_device)
    ring = env.enable_return_log(2)
    env.reset(r["seeds"], observe=False)
    steps = env.rollout_random(episodes=2).cpu().numpy()
    got, sm, abc = ring.cpu().numpy(), env.summary().cpu().numpy(), env.abandoned_counts().cpu().numpy()
    for b, (first, second) in enumerate(r["eps"]):
        assert steps[b] == first["n_steps"] + second["n_steps"], b
        assert got[b, 0] == first["reward"] and got[b, 1] == second["reward"], b
        O.assert_summary(sm[b], second, f"env {b}")
        assert np.array_equal(abc[b].astype(np.int64), r["ab2"][b]), (b, abc[b], r["ab2"][b])
    env.close()
