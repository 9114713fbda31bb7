"""The reference layer of the lookahead tests (lookahead_ref.py) against the oracle, before any GPU test leans on it: the Python distance
on the known-answer table, and the walker under first / nearest / random against the oracle's own rollouts.  No GPU."""
import os

import numpy as np
import pytest

import lookahead_ref as LA
import oracle_ref as O

SHAPES = ((10, 20), (20, 50))
N_INST = 8


def test_python_distance_is_the_known_answer_table(golden_dir):
    z = np.load(os.path.join(golden_dir, "distance_kat.npz"))
    a, b, want = z["a"], z["b"], z["dist"]
    got = np.array([LA.distance(a[i, 0], a[i, 1], b[i, 0], b[i, 1]) for i in range(len(want))])
    assert got.tobytes() == want.tobytes(), np.flatnonzero(got != want)[:8]


@pytest.fixture(scope="module")
def batches(oracle_lib):
    from dcmrta_amd.choice import env_seeds
    from dcmrta_amd.instances import generate_batch
    return {(A, T): (generate_batch(N_INST, A, T, base_seed=300 + A), env_seeds(9, 0, N_INST)) for A, T in SHAPES}


@pytest.mark.parametrize("policy", ["first", "nearest", "random"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dA%dT" % s)
def test_walker_reproduces_the_oracles_rollouts(batches, shape, policy):
    """the actions, leaders, follower counts and masks of every decision; reward, finished tasks and the six metrics of the episode the
    oracle replays from the walk's choices"""
    A, T = shape
    inst, seeds = batches[shape]
    for b in range(N_INST):
        one = O.one(inst, b)
        ref = O.episodes(A, T, one, seeds[b], policy, 1, record=True)[0]
        w = LA.policy_walk(A, T, one, int(seeds[b]), policy)
        assert w["ended"] and w["n_steps"] == ref["n_steps"], (b, w["n_steps"], ref["n_steps"])
        for k in ("action", "leader", "nfol", "mask"):
            assert np.array_equal(w[k], ref[k]), (b, k, np.flatnonzero(np.asarray(w[k] != ref[k]).reshape(len(w[k]), -1).any(1))[:4])
        assert np.array_equal(w["followers"], ref["followers"]), b
        r = LA.result(A, T, one, w)
        assert r["reward"] == ref["reward"] and np.array_equal(r["finished"], ref["finished"]), b
        assert np.array_equal(r["metrics"], ref["metrics"]) and LA.pair(r) == LA.pair(ref), b


def test_a_seed_switch_at_decision_0_is_the_other_seeds_episode_and_a_late_one_keeps_the_prefix(batches):
    A, T = SHAPES[0]
    inst, seeds = batches[SHAPES[0]]
    one = O.one(inst, 0)
    for policy in ("nearest", "random"):
        other = O.episodes(A, T, one, seeds[1], policy, 1, record=True)[0]
        w = LA.policy_walk(A, T, one, int(seeds[0]), policy, switch=(0, int(seeds[1])))
        assert np.array_equal(w["action"], other["action"]) and np.array_equal(w["leader"], other["leader"])
        own = LA.policy_walk(A, T, one, int(seeds[0]), policy)
        late = LA.policy_walk(A, T, one, int(seeds[0]), policy, switch=(5, int(seeds[1])))
        assert np.array_equal(late["action"][:5], own["action"][:5]) and np.array_equal(late["leader"][:5], own["leader"][:5])
        assert LA.result(A, T, one, late)["n_steps"] == late["n_steps"]


def test_lookahead_values_hold_the_base_policys_own_episode(batches):
    """the column of the action `nearest` itself picks is the plain `nearest` episode; masked entries are NaN / -1"""
    A, T = SHAPES[0]
    inst, seeds = batches[SHAPES[0]]
    one = O.one(inst, 2)
    ref = O.episodes(A, T, one, seeds[2], "nearest", 1, record=True)[0]
    for d in (0, ref["n_steps"] // 2):
        reward, finished, mask = LA.lookahead_values(A, T, one, int(seeds[2]), d)
        assert np.array_equal(mask, ref["mask"][d])
        assert np.array_equal(np.isnan(reward), mask == 1) and np.array_equal(finished == -1, mask == 1)
        a = int(ref["action"][d])
        assert reward[a] == ref["reward"] and finished[a] == int(ref["finished"].sum())
    assert LA.lookahead_values(A, T, one, int(seeds[2]), ref["n_steps"]) is None
