"""-m gpu: per-action lookahead values and the rollout-algorithm planner (dcmrta_amd.lookahead.Lookahead) against the oracle's walks.

values(): for envs stopped at three places of their `nearest` episodes -- the first decision, the middle, two decisions before the end
(finished tasks are masked there), and one env that is DONE -- every unmasked action's (reward, finished tasks) is the walker's, bit
for bit: the oracle's episode with that one action forced and `nearest` playing every other decision (lookahead_ref.lookahead_values).
plan(): every env ends at or above its `nearest` episode, exactly, and the logged routes replay to the reported summary rows."""
import numpy as np
import pytest

import lookahead_ref as LA
import oracle_ref as O

CASES = {"10A20T": dict(A=10, T=20, B=4), "20A50T": dict(A=20, T=50, B=2)}
INST_SEED, CHOICE_SEED = 61, 3

_cache = {}


def batch(name):
    """(instances, seeds, the oracle's `nearest` episode of every env, recorded): computed once, never changed"""
    from dcmrta_amd.choice import env_seeds
    from dcmrta_amd.instances import generate_batch
    if name not in _cache:
        c = CASES[name]
        inst, seeds = generate_batch(c["B"], c["A"], c["T"], base_seed=INST_SEED + c["A"]), env_seeds(CHOICE_SEED, 0, c["B"])
        eps = [O.episodes(c["A"], c["T"], O.one(inst, b), seeds[b], "nearest", 1, record=True)[0] for b in range(c["B"])]
        _cache[name] = (inst, seeds, eps)
    return _cache[name]


def points(name):
    """the decision every env is stopped in front of, per place; -1: the env plays its episode to the end (DONE)"""
    n = np.array([e["n_steps"] for e in batch(name)[2]])
    late = n - 2
    late[-1] = -1
    return dict(first=np.zeros(len(n), np.int64), middle=n // 2, late=late)


@pytest.mark.parametrize("name", list(CASES))
def test_the_places_cover_what_the_values_test_claims(oracle_lib, name):
    """CPU: every stop lies inside the episode, and the late place has masked tasks"""
    _, _, eps = batch(name)
    for place, ds in points(name).items():
        for b, d in enumerate(ds):
            assert d == -1 or 0 <= d < eps[b]["n_steps"], (place, b)
    for b, d in enumerate(points(name)["late"]):
        if d >= 0:
            assert eps[b]["mask"][d][1:].sum() >= 1 and (eps[b]["mask"][d] == 0).sum() >= 1, b


def make(gpu_device, name):
    from dcmrta_amd.batched_env import BatchedTaskEnv
    c = CASES[name]
    inst, seeds, _ = batch(name)
    return BatchedTaskEnv(c["B"], c["A"], c["T"], device=gpu_device).load_instances(**inst), seeds


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CASES))
def test_values_are_the_walkers(gpu_device, oracle_lib, name):
    from dcmrta_amd.lookahead import Lookahead
    c = CASES[name]
    A, T, B = c["A"], c["T"], c["B"]
    inst, seeds, eps = batch(name)
    env, _ = make(gpu_device, name)
    la = Lookahead(env, "nearest")
    assert la.branch.B == B * (T + 1)
    for place, ds in points(name).items():
        env.reset(seeds, observe=False)
        env.rollout("nearest", write_obs=False, max_decisions=ds)            # (-1: no limit, the env ends DONE)
        before = env.clone_state().cpu().numpy()
        reward, finished = (x.cpu().numpy() for x in la.values())
        assert reward.shape == (B, T + 1) and reward.dtype == np.float64 and finished.dtype == np.int32
        assert env.clone_state().cpu().numpy().tobytes() == before.tobytes(), (place, "the main env changed")
        for b, d in enumerate(ds):
            if d == -1:
                assert np.isnan(reward[b]).all() and (finished[b] == -1).all(), (place, b, "a DONE env")
                continue
            want_r, want_f, mask = LA.lookahead_values(A, T, O.one(inst, b), int(seeds[b]), int(d))
            assert np.array_equal(np.isnan(reward[b]), mask == 1) and np.array_equal(finished[b] == -1, mask == 1), (place, b, "masked entries")
            assert np.array_equal(reward[b], want_r, equal_nan=True) and np.array_equal(finished[b], want_f), \
                (place, b, np.flatnonzero(~((reward[b] == want_r) | np.isnan(want_r))), reward[b], want_r)
            a = int(eps[b]["action"][d])                                    # the action `nearest` itself takes there: its own episode
            assert reward[b, a] == eps[b]["reward"] and finished[b, a] == int(eps[b]["finished"].sum()), (place, b, a)
    assert la.launches == 3
    la.close(); env.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CASES))
def test_plan_never_ends_below_nearest_and_its_routes_replay(gpu_device, oracle_lib, name, capsys):
    from dcmrta_amd.lookahead import Lookahead
    c = CASES[name]
    A, T, B = c["A"], c["T"], c["B"]
    inst, seeds, eps = batch(name)
    env, _ = make(gpu_device, name)
    env.enable_route_log(64)
    env.reset(seeds, observe=False)
    la = Lookahead(env, "nearest")
    n = la.plan()
    sm = env.summary().cpu().numpy()
    st = {k: v.cpu().numpy() for k, v in env.status().items()}
    task, _, length = (x.cpu().numpy() for x in env.routes())
    assert (st["flags"] & 1).all() and n == int(st["decisions"].max()) + 1 == la.launches
    better = 0
    for b in range(B):
        got, base = (int(sm[b, 1]), float(sm[b, 0])), LA.pair(eps[b])
        assert got >= base, (b, got, base)                                  # exact: the seeded determinism, not a statistic
        better += got > base
        assert length[b].max() <= 64
        w = LA.routes_walk(A, T, O.one(inst, b), int(seeds[b]), task[b])
        assert w["ended"] and w["n_steps"] == int(st["decisions"][b]), (b, w["n_steps"], int(st["decisions"][b]))
        O.assert_summary(sm[b], LA.result(A, T, O.one(inst, b), w), f"{name} env {b}: the logged plan")
    with capsys.disabled():
        print(f"\n[lookahead plan {name}] {better} of {B} instances end strictly above nearest; {n} lookahead launches")
    la.close(); env.close()
