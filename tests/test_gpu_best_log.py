"""-m gpu: the best log of the persistent launches (dcm_set_best_log; BatchedTaskEnv.enable_best_log) -- every env keeps the best episode
it has finished since reset(), by (finished tasks, reward), with its summary row, its ordinal and its routes -- through the
register-resident form (k_bs_rollout_fast) and the general one (k_bs_rollout_random), under all three entry points.

Yardstick: the chain of pinned launches.  A twin handle with only the rollout log plays the same episodes one per launch through the
existing entry points (a later launch "carries on with identical results"); after each launch the host reads summary, episode count
and log and applies the order of include/dcmrta_env.h itself.  For "random" and plain "nearest" the kept lists are the oracle's as
well.  Every comparison is exact."""
import numpy as np
import pytest

import oracle_ref as O
from forms import Forms, assert_same, snap

pytestmark = pytest.mark.gpu

ERR_INVALID, ERR_STATE = -1, -4
CAP, E = 64, 4
Q30 = 1 << 30
ERR_FLAGS = 0x38 | 0x40                                                         # bad action, overflow, bad leader, bad instance
PLAYS = {"random": ("random", None), "nearest": ("nearest", None), "nearest-q30": ("nearest", Q30)}

# id: (A, T, B, BatchedTaskEnv keywords, ragged ranges, scalar budget of every launch) -- the entries and base seeds of
# test_gpu_explore.py, so the two files share the cached instances and oracle runs (forms.py caches by value)
FORMS = {
    "F1": (20, 50, 6, {}, None, -1),                                            # fast, exact
    "F2": (20, 50, 6, {}, ((10, 20), (20, 50)), -1),                            # fast, runtime sizes (a ragged batch)
    "F3": (30, 60, 4, {}, None, -1),                                            # fast, Lay{64,64}
    "F4": (10, 64, 4, {}, None, -1),                                            # general: no free depot lane
    "F5": (66, 70, 4, {}, None, -1),                                            # general, the mid-size layout
    "F6": (10, 20, 4, dict(max_waiting_time=0.0), None, 60),                    # general, the literal rule; every launch under a budget
}
BIG_FORMS = {"F7-above-64KiB": (4, 700, 2, {}, None, -1)}                       # record_bytes > 64 KiB: the raised dynamic-LDS limit
ALL_FORMS = {**FORMS, **BIG_FORMS}
F = Forms(FORMS, BIG_FORMS, 6000, 6100, 41)


def _play(env, play, episodes, budget=None):
    policy, q32 = PLAYS[play]
    kw = {} if q32 is None else dict(explore_q32=q32)
    if budget is None:
        budget = ALL_FORMS[env._form][5]
    return env.rollout(policy, episodes=episodes, max_decisions=budget, **kw).cpu().numpy()


def _env(gpu_device, form, best, cap=CAP):
    env, seeds = F.env(gpu_device, form)
    env.enable_rollout_log(cap)
    if best:
        env.enable_best_log()
    env._ring = env.enable_return_log(2)
    env._form = form
    env.reset(seeds, observe=False)
    return env


def _best(env):
    task, arrival, length = (x.cpu().numpy().copy() for x in env.best_routes())
    return dict(task=task, arrival=arrival, len=length, summary=env.best_summary().cpu().numpy().copy(),
                episode=env.best_episode().cpu().numpy().copy())


def _chain(gpu_device, form, play, episodes, cap=CAP, total=None):
    """The yardstick: `episodes` episodes per env as launches of ONE episode on a twin without the best log, under the launch's total
    decision budget (`total`: an int for every env; default the form's).  Returns (twin, kept, taken): kept[b] = None or the dict
    (summary, episode, len, task, arrival) of the episode the order keeps, taken[b] the decisions."""
    twin = _env(gpu_device, form, False, cap)
    B = twin.B
    total = ALL_FORMS[form][5] if total is None else total
    kept, seen = [None] * B, np.zeros(B, np.int64)
    played, taken = np.zeros(B, np.int64), np.zeros(B, np.int64)
    mid = np.zeros(B, bool)                                                     # in the middle of an episode that counts already
    for _ in range(20 * episodes + 20):
        live = (played < episodes) | mid
        if total >= 0:
            live &= taken < total
        if not live.any():
            break
        budget = np.where(live, (total - taken) if total >= 0 else (1 << 40), 0).astype(np.int64)
        steps = _play(twin, play, 1, budget)
        assert (steps[~live] == 0).all()
        taken += steps
        st = twin.status()["flags"].cpu().numpy()
        sm, ep = twin.summary().cpu().numpy(), twin.episodes().cpu().numpy()
        task, arrival, length = (x.cpu().numpy() for x in twin.rollout_routes())
        for b in np.flatnonzero(live):
            played[b] += 0 if mid[b] else 1
            mid[b] = not st[b] & 1
            if mid[b] or st[b] & ERR_FLAGS or ep[b] == seen[b]:
                continue
            seen[b] = ep[b]
            k = kept[b]
            if k is None or sm[b, 1] > k["summary"][1] or (sm[b, 1] == k["summary"][1] and sm[b, 0] > k["summary"][0]):
                kept[b] = dict(summary=sm[b].copy(), episode=int(ep[b]) - 1, len=length[b].copy(), task=task[b].copy(), arrival=arrival[b].copy())
    else:
        raise AssertionError("the chain did not end")
    return twin, kept, taken


def _assert_best(got, kept, sizes, tag):
    """The best log against what the chain keeps: the summary row as bytes, the ordinal, the true lengths, the defined prefix of every
    row (nothing is defined behind it: an earlier kept episode may have been longer) -- and, in the rows of agents the env does not
    have, the buffers' initial fill."""
    cap = got["task"].shape[2]
    for b, k in enumerate(kept):
        if k is None:
            assert got["episode"][b] == -1 and np.isnan(got["summary"][b]).all() and (got["len"][b] == 0).all(), (tag, b)
            continue
        assert got["episode"][b] == k["episode"], (tag, b, int(got["episode"][b]), k["episode"])
        assert got["summary"][b].tobytes() == k["summary"].tobytes(), (tag, b)
        for a in range(got["task"].shape[1]):
            if a >= sizes[b]:
                assert got["len"][b, a] == 0 and (got["task"][b, a] == -2).all() and (got["arrival"][b, a] == 0.0).all(), (tag, b, a)
                continue
            n = min(int(k["len"][a]), cap)
            assert got["len"][b, a] == k["len"][a], (tag, b, a)
            assert np.array_equal(got["task"][b, a, :n], k["task"][a, :n]), (tag, b, a)
            assert got["arrival"][b, a, :n].tobytes() == k["arrival"][a, :n].tobytes(), (tag, b, a)


def _sizes(form):
    A, _, B, _, ranges, _ = ALL_FORMS[form]
    inst, _ = F.instances(form)
    return [A] * B if ranges is None else [int(x) for x in inst["n_agents"]]


# ---------------------------------------------------------------------------------------------------- 1. + 2. the chain, not vacuous
# the episode each env keeps under "random" (E = 4, env_seeds(41, 0, B)): computed with the oracle on the CPU
KEPT_RANDOM = {"F1": [3, 3, 3, 2, 2, 2], "F2": [0, 0, 2, 1, 1, 2], "F3": [2, 3, 2, 3], "F4": [1, 0, 1, 3], "F5": [1, 2, 1, 0], "F7-above-64KiB": [3, 1]}
CASES = ([(f, "random", E) for f in sorted(ALL_FORMS) if ALL_FORMS[f][5] < 0] + [(f, "nearest-q30", E) for f in ("F1", "F2", "F3", "F4", "F5")]
         + [(f, "nearest", E) for f in ("F1", "F4")])


@pytest.mark.parametrize("form,play,episodes", CASES, ids=[f"{f}-{p}" for f, p, _ in CASES])
def test_one_launch_keeps_what_the_chain_of_one_episode_launches_keeps(gpu_device, form, play, episodes):
    tag = f"{form} {play}"
    twin, kept, taken = _chain(gpu_device, form, play, episodes)
    env = _env(gpu_device, form, True)
    steps = _play(env, play, episodes)
    got = _best(env)
    print(tag, "kept episodes", got["episode"].tolist(), "chain", [None if k is None else k["episode"] for k in kept])
    assert np.array_equal(steps, taken), tag
    assert all(k is not None for k in kept), tag
    _assert_best(got, kept, _sizes(form), tag)
    eps = got["episode"]
    if play == "nearest":                                                       # every episode alike: the tie keeps the earliest
        assert (eps == 0).all(), (tag, eps)
    else:                                                                       # somebody keeps another episode than the last, somebody another than the first
        assert (eps != episodes - 1).any() and (eps != 0).any(), (tag, eps)
    if play == "random":
        assert eps.tolist() == KEPT_RANDOM[form], (tag, eps)
    if play in ("random", "nearest"):                                           # ... and the kept lists are the oracle's
        orc = F.episodes(form, play, episodes)
        log = (got["task"], got["arrival"], got["len"])
        for b in range(env.B):
            fin = [e.o.final() for e in orc[b]]
            order = [(int(f["finished"].sum()), f["reward"]) for f in fin]
            assert int(eps[b]) == max(range(episodes), key=lambda i: (order[i], -i)), (tag, b, order)   # the earliest of the best
            assert (got["summary"][b, 1], got["summary"][b, 0]) == order[int(eps[b])], (tag, b)
            O.assert_log(log, b, orc[b][int(eps[b])], tag)


# ---------------------------------------------------------------------------------------------------- 3. the invariant
@pytest.mark.parametrize("play", ["random", "nearest-q30"])
@pytest.mark.parametrize("form", ["F1", "F4", "F5", "F7-above-64KiB"])
def test_a_launch_with_the_best_log_returns_what_it_returns_with_the_rollout_log_alone(gpu_device, form, play):
    twin = _env(gpu_device, form, False)
    ref = snap(twin, _play(twin, play, E))
    env = _env(gpu_device, form, True)
    got = snap(env, _play(env, play, E))
    assert_same(got, ref, f"{form} {play}")
    assert (env.best_episode().cpu().numpy() >= 0).all()


# ---------------------------------------------------------------------------------------------------- 4. budgets and launches
@pytest.mark.parametrize("play", ["random", "nearest-q30"])
@pytest.mark.parametrize("form", ["F1", "F4"])
def test_budget_stops_keep_nothing_and_later_launches_carry_on(gpu_device, form, play):
    tag = f"{form} {play}"
    B = ALL_FORMS[form][2]
    whole = _env(gpu_device, form, True)
    ref = snap(whole, _play(whole, play, E))
    ref_best = _best(whole)
    kept = [dict(summary=ref_best["summary"][b], episode=int(ref_best["episode"][b]), len=ref_best["len"][b], task=ref_best["task"][b],
                 arrival=ref_best["arrival"][b]) for b in range(B)]
    # budgets inside episode 0: nothing is kept; the second launch finishes what the uninterrupted one plays
    budgets = np.array([0, 1, 7, 23, 2, 30][:B], np.int64)
    env = _env(gpu_device, form, True)
    first = _play(env, play, E, budgets)
    assert np.array_equal(first, budgets) and not (env.status()["flags"].cpu().numpy() & 1).any()
    _assert_best(_best(env), [None] * B, _sizes(form), tag + " stopped")
    second = _play(env, play, E)
    assert_same(snap(env, first + second), ref, tag + " continued")
    _assert_best(_best(env), kept, _sizes(form), tag + " continued")
    # two launches of two episodes
    env = _env(gpu_device, form, True)
    steps = _play(env, play, 2)
    half = _best(env)
    assert (half["episode"] >= 0).all() and (half["episode"] <= 1).all()
    steps = steps + _play(env, play, 2)
    assert_same(snap(env, steps), ref, tag + " 2 + 2")
    _assert_best(_best(env), kept, _sizes(form), tag + " 2 + 2")
    # reset() forgets
    env.reset(F.instances(form)[1], observe=False)
    cleared = _best(env)
    assert (cleared["episode"] == -1).all() and np.isnan(cleared["summary"]).all() and (cleared["len"] == 0).all()


@pytest.mark.parametrize("total", [60, 600])
@pytest.mark.parametrize("play", ["random", "nearest-q30"])
def test_on_the_literal_rule_a_budgeted_launch_keeps_nothing_or_what_the_chain_keeps(gpu_device, play, total):
    """F6: max_waiting_time = 0, the launch under the form's 60 decisions (and under ten times as many) -- the chain splits the same
    budget over its launches."""
    twin, kept, taken = _chain(gpu_device, "F6", play, E, total=total)
    env = _env(gpu_device, "F6", True)
    steps = _play(env, play, E, total)
    got = _best(env)
    print("F6", play, total, "kept episodes", got["episode"].tolist(), "steps", steps.tolist())
    assert np.array_equal(steps, taken)
    _assert_best(got, kept, _sizes("F6"), f"F6 {play}")
    assert_same(snap(env, steps), snap(twin, taken), f"F6 {play}")


# ---------------------------------------------------------------------------------------------------- 5. a small cap
def test_a_log_of_four_keeps_the_true_lengths_and_the_prefixes(gpu_device):
    twin, kept, taken = _chain(gpu_device, "F1", "random", E, cap=4)
    env = _env(gpu_device, "F1", True, cap=4)
    assert np.array_equal(_play(env, "random", E), taken)
    got = _best(env)
    assert got["task"].shape == (6, 20, 4) and (got["len"] > 4).sum() > 6 * 20 // 2 and got["len"].max() >= 9
    _assert_best(got, kept, _sizes("F1"), "cap 4")                              # every row of the batch: nothing spills into a neighbour
    assert got["episode"].tolist() == KEPT_RANDOM["F1"]
    with pytest.raises(ValueError, match=r"enable_rollout_log\(cap\)"):
        env.best_plan()


# ---------------------------------------------------------------------------------------------------- 6. refusals
def _everything(env):
    parts = dict(state=env.clone_state(), summary=env.summary(), episodes=env.episodes())
    parts.update(zip(("log_task", "log_arrival", "log_len"), env.rollout_routes()))
    out = {k: v.cpu().numpy().copy() for k, v in parts.items()}
    out.update({"best_" + k: v for k, v in _best(env).items()})
    return out


def _assert_unchanged(env, before, tag):
    after = _everything(env)
    for k in before:
        assert after[k].tobytes() == before[k].tobytes(), (tag, k)


def test_refusals_launch_nothing_and_change_nothing(gpu_device):
    import helpers as H
    from dcmrta_amd.batched_env import BatchedTaskEnv, _ptr
    from dcmrta_amd._lib import DcmError
    # a partial set of buffers
    env = _env(gpu_device, "F1", True)
    _play(env, "random", 2)
    before = _everything(env)
    bufs = [_ptr(x) for x in env._best]
    for hole in range(5):
        rc = env._lib.dcm_set_best_log(env._h, *[None if i == hole else p for i, p in enumerate(bufs)])
        assert rc == ERR_INVALID and b"dcm_set_best_log" in env._lib.dcm_last_error(), hole
    # the best log without the rollout log, at launch (the Python layer never gets there: the C call)
    assert env._lib.dcm_set_rollout_log(env._h, None, None, None, 0) == 0
    for play in PLAYS:
        with pytest.raises(DcmError, match=r"error %d: dcm_rollout_(random|policy|explore): the best log is set and the rollout log is not" % ERR_STATE):
            _play(env, play, 1)
        _assert_unchanged(env, before, play)
    assert env._lib.dcm_set_rollout_log(env._h, *[_ptr(x) for x in env._rollout_route], CAP) == 0
    assert int(_play(env, "random", 1).sum()) > 0                               # ... and with it the launch runs again
    # a renewal stride on a generated batch
    B = 4
    env = BatchedTaskEnv(B, 20, 50, device=gpu_device)
    env.generate_instances(np.arange(9700, 9700 + B, dtype=np.uint64))
    env.enable_rollout_log(CAP).enable_best_log()
    env.reset(5, observe=False)
    env._form = "F1"
    _play(env, "random", 1)
    env.set_instance_renewal(B)
    before = _everything(env)
    for play in PLAYS:
        with pytest.raises(DcmError, match=r"error %d: dcm_rollout_(random|policy|explore): no best log while instances are renewed.*"
                                           r"dcm_set_instance_renewal\(env, 0\).*dcm_set_best_log" % ERR_STATE):
            _play(env, play, 2)
        _assert_unchanged(env, before, "renewal " + play)
    env.enable_best_log(False)                                                  # either way out works
    assert int(_play(env, "random", 1).sum()) > 0
    env.enable_best_log()
    env.set_instance_renewal(0)
    assert int(_play(env, "random", 1).sum()) > 0
    with pytest.raises(DcmError, match="best log is off"):
        env.enable_best_log(False).best_routes()
    # episodes that dcm_step ends are no candidates
    env = _env(gpu_device, "F1", True)
    seeds = F.instances("F1")[1]
    H.run_lockstep(env, seeds, lambda b, i, m, l: H.host_random_action(m, int(seeds[b]), i))
    assert (env.episodes().cpu().numpy() >= 1).all()
    got = _best(env)
    assert (got["episode"] == -1).all() and np.isnan(got["summary"]).all() and (got["len"] == 0).all() and (got["task"] == -2).all()


def test_the_rollout_logs_cap_takes_the_best_log_with_it(gpu_device):
    env = _env(gpu_device, "F1", True)
    env.enable_rollout_log(16)
    assert env.best_routes()[0].shape == (6, 20, 16) and env.rollout_routes()[0].shape == (6, 20, 16)
    env.reset(F.instances("F1")[1], observe=False)
    _play(env, "random", 2)
    assert (env.best_episode().cpu().numpy() >= 0).all()
    env.enable_rollout_log(0)
    assert env._best is None
    assert int(_play(env, "random", 1).sum()) > 0                               # the C side dropped it too: no refusal


# ---------------------------------------------------------------------------------------------------- 7. consumers
def test_the_kept_plan_reaches_yaml_and_generate_traj(gpu_device, tmp_path):
    from dcmrta_amd.trajectory import generate_traj, routes_to_yaml
    env = _env(gpu_device, "F1", True)
    _play(env, "random", E)
    eps = env.best_episode().cpu().numpy()
    assert eps.tolist() == KEPT_RANDOM["F1"]
    plan = env.best_plan()
    assert [[len(r) for r in p] for p in plan] == env.best_routes()[2].cpu().numpy().tolist()
    for b in range(env.B):
        assert env.best_plan(b) == plan[b]
        assert routes_to_yaml(env, str(tmp_path / f"best_{b}.yaml"), b, log="best") == dict(enumerate(plan[b]))
    # generate_traj: the twin stopped after the kept episode.  The records hold the last episode, so the envs that keep it
    twin = _env(gpu_device, "F1", False)
    _play(twin, "random", E)
    last = [b for b in range(env.B) if eps[b] == E - 1]
    assert last and len(last) < env.B
    for b in last:
        got, ref = generate_traj(env, b, log="best"), generate_traj(twin, b, log="rollout")
        assert len(got) == len(ref) == 20 and all(g.tobytes() == r.tobytes() for g, r in zip(got, ref)), b
    for b in set(range(env.B)) - set(last):                                     # ... and says so for the others
        with pytest.raises(ValueError, match="replay best_plan"):
            generate_traj(env, b, log="best")
