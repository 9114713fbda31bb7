"""What test_gpu_param_edges.py reaches, proven on the CPU from the oracle alone: the kernel every shape of the table selects, how the
episodes of every (max_waiting_time, max_time) set end, how often agents are abandoned, where `nearest` meets equal distances on the
degenerate instances -- so a change of the base seeds that loses a path fails here, without a GPU.  And the reference layer with
max_time threaded through: given 100.0 explicitly, every reference returns what it returns by default.  No GPU."""
import numpy as np
import pytest

import explore_ref as EX
import lookahead_policy_ref as LP
import lookahead_ref as LA
import lookahead_width_ref as LW
import oracle_ref as O
import param_edges_ref as PE
import removal_ref as RR
import renewal_ref as R
from forms import degenerate

FORMS, F = PE.FORMS, PE.F

# the kernel dcm_rollout_random takes with all or no observation buffers, and the Sim<> instantiation of the general kernels
KERNELS = {
    "small": ("k_rollout_fast", "<20,50,true>"), "few-agents": ("k_rollout_fast", "<20,50,true>"), "exact": ("k_rollout_fast", "<20,50,false>"),
    "ragged": ("k_rollout_fast", "<20,50,true>"), "lay64": ("k_rollout_fast", "<64,64,true>"), "no-depot-lane": ("k_rollout_random", "<64,64,true>"),
    "mid": ("k_rollout_fast_g", "<128,256,true>"), "mc": ("k_rollout_fast_mc", "<50,200,false>"), "chunks": ("k_rollout_fast_g", "<128,256,true>"),
    "wide": ("k_rollout_random", "<0,0,false,MW>"), "many-agents": ("k_rollout_fast_g", "<128,256,true>"),
}


def test_every_shape_selects_the_kernel_it_is_there_for():
    from dcmrta_amd.roofline import rollout_kernel_name, sim_kind_name
    assert sorted(KERNELS) == sorted(PE.SHAPES)
    for s, (A, T, B, kw, ranges) in PE.SHAPES.items():
        wide = kw.get("member_cap", 5) > 5
        name = "k_rollout_random" if wide else rollout_kernel_name(A, T)      # (plan::rollout_kind: a wide handle takes the general kernel)
        assert (name, sim_kind_name(A, T, ragged=ranges is not None, wide=wide)) == KERNELS[s], s
    assert len(FORMS) == len(PE.SHAPES) * len(PE.PARAMS) + len(PE.DEGENERATE_SHAPES) + len(PE.TINY_SHAPES)
    assert all(PE.split(f)[0] in PE.SHAPES for f in FORMS)
    assert all(FORMS[f][3]["max_waiting_time"] > 0.0 for f in FORMS)           # every row on the `quiet` side of plan::Shape::quiet


def test_degenerate_instances_have_the_edges_they_name():
    inst, _ = F.instances(PE.form_id("small", "degenerate"))
    plain, _ = F.instances(PE.form_id("small", "w10-t30"))
    xy, T = inst["task_xy"], inst["task_xy"].shape[1]
    assert np.array_equal(xy[:, 1::2], xy[:, 0:T - 1:2]) and np.array_equal(xy[:, 0], inst["depot"]) and np.array_equal(xy[:, 1], inst["depot"])
    assert not inst["dur"][:, ::3].any() and np.array_equal(inst["req"], plain["req"]) and np.array_equal(inst["depot"], plain["depot"])
    assert np.array_equal(degenerate(plain)["task_xy"], xy) and plain["dur"][:, ::3].any()             # a copy: the source is untouched
    few, _ = F.instances(PE.form_id("few-agents", "w10-t30"))
    assert (few["req"] > PE.SHAPES["few-agents"][0]).any(axis=1).all()                                  # tasks three agents can never start


@pytest.mark.parametrize("policy", PE.POLICIES)
@pytest.mark.parametrize("form", sorted(FORMS))
def test_every_case_reaches_its_path(form, policy):
    PE.check_case(form, policy)


def test_counts_quoted_in_the_design_notes():
    """DESIGN.md section 4 quotes these; they come from the first three random episodes of every env."""
    most = {s: max(int(e["abandoned"].max()) for env in PE.facts(PE.form_id(s, "w3-t250"), "random") for e in env) for s in PE.SHAPES}
    assert most == {"small": 46, "few-agents": 52, "exact": 33, "ragged": 39, "lay64": 20, "no-depot-lane": 45, "mid": 5, "mc": 46, "chunks": 44,
                    "wide": 21, "many-agents": 0}, most
    total = max(int(e["abandoned"].sum()) for env in PE.facts(PE.form_id("mc", "w3-t250"), "random") for e in env)
    assert total == 1628
    ends = {s: sorted({e["ending"] for p in PE.POLICIES for env in PE.facts(PE.form_id(s, "w10-t30"), p) for e in env}) for s in PE.SHAPES}
    assert all(ends[s] == ["max-time"] for s in PE.CUT_EVERYWHERE + ("few-agents", "ragged")), ends
    assert ends["mid"] == ["finished", "max-time"] and ends["many-agents"] == ["finished"], ends
    assert not any(e["ending"] == "stuck" for f in FORMS if PE.split(f)[1] != "tiny" for p in PE.POLICIES for env in PE.facts(f, p) for e in env)


def test_fork_points_and_windows_lie_where_the_gpu_tests_need_them():
    at, most = PE.fork_points(PE.form_id("mc", "w3-t250"))
    assert max(most) > PE.AB_CAP and all(0 < a < n for a, n in zip(at, PE.first_lengths(PE.form_id("mc", "w3-t250"), "random")))
    assert max(PE.fork_points(PE.form_id("wide", "w3-t250"))[1]) > 0
    for form in (PE.form_id("small", "w3-t250"), PE.form_id("few-agents", "w3-t250")):
        for width in (None, 2):
            cases = PE.lookahead_cases(form, width)
            assert all(not c["whole"] and not c["window"]["ended"] and c["tail"]["n_steps"] > c["d0"] + PE.LOOKAHEAD_WINDOW_K for c in cases)
            assert any(f["n_unmasked"] > 2 for c in cases for f in c["window"]["facts"]), form
    # at max_time 30 the values of a lookahead decision tie: the inner episodes all end at the limit
    inst, seeds = F.instances(PE.form_id("small", "w10-t30"))
    win = LP.lookahead_window(6, 12, O.one(inst, 0), int(seeds[0]), "nearest", 10.0, 0, 4, 30.0)
    assert all(f["at_max_time"] == f["n_unmasked"] for f in win["facts"] if f["n_unmasked"] > 1), win["facts"]


def test_an_agent_is_dropped_by_two_tasks_in_one_pass_at_the_smallest_waiting_time():
    """what lets test_gpu_param_edges.py compare abandonment-log rows as multisets, and only there: the oracle's walk of the launch"""
    form = PE.form_id("small", "tiny")
    drops = PE.double_drops(form, "random")
    assert drops[0] == [(1, [4, 11])] and sum(len(d) for d in drops) == 5, drops
    assert not any(PE.double_drops(form, "first")) and not any(PE.double_drops(form, "nearest"))
    # the walk plays the decisions of the launch it stands for: the budget's 200 per env, and the oracle's count without one
    form = PE.form_id("small", "w3-t250")
    assert sum(len(d) for d in PE.double_drops(form, "random")) == 1                        # rounding alone, at an ordinary waiting time


def test_explore_walk_ends_are_the_pinned_policies():
    """explore_ref at explore_q32 0 and 2^32 is the oracle's own `nearest` and random rollout, episode by episode"""
    form = PE.form_id("small", "w10-t30")
    mwt, mt = PE.params_of(form)
    inst, seeds = F.instances(form)
    for q32, policy in ((0, "nearest"), (1 << 32, "random")):
        for b in range(2):
            got = EX.explore_episodes(6, 12, O.one(inst, b), int(seeds[b]), "nearest", q32, 3, mwt, mt)
            ref = O.episodes(6, 12, O.one(inst, b), seeds[b], policy, 3, mwt, max_time=mt)
            assert [g["n_steps"] for g in got] == [r["n_steps"] for r in ref], (q32, b)
            assert all(O.summary_row(g["result"]).tobytes() == O.summary_row(r).tobytes() for g, r in zip(got, ref)), (q32, b)
    cases = PE.explore_cases(form)
    assert any(0 < e["explored"] < e["n_steps"] for eps in cases for e in eps)
    assert all(LA.pair(e["result"])[0] < 12 for eps in cases for e in eps)


def _same(x, y):
    if isinstance(x, dict):
        return sorted(x) == sorted(y) and all(_same(x[k], y[k]) for k in x if k not in ("o", "seed_of"))
    if isinstance(x, (list, tuple)):
        return len(x) == len(y) and all(_same(a, b) for a, b in zip(x, y))
    if isinstance(x, np.ndarray):
        return x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes()
    return x == y or (isinstance(x, float) and x != x and y != y)


def test_an_explicit_max_time_of_100_is_the_default():
    """one case per reference module"""
    import oracle
    from dcmrta_amd.choice import env_seeds
    from dcmrta_amd.instances import generate_batch
    A, T, B = 5, 8, 2
    inst, seeds = generate_batch(B, A, T, base_seed=77), env_seeds(7, 0, B)
    one, seed = O.one(inst, 0), int(seeds[0])
    # oracle_ref
    strip = lambda eps: [{k: v for k, v in e.items()} for e in eps]
    assert _same(strip(O.episodes(A, T, one, seed, "nearest", 2)), strip(O.episodes(A, T, one, seed, "nearest", 2, max_time=100.0)))
    assert _same(O.two_episodes(inst, seeds, A, T), O.two_episodes(inst, seeds, A, T, 10.0, 100.0))
    a, b = O.play(A, T, one, seed, 0, "random", 5, 10.0), O.play(A, T, one, seed, 0, "random", 5, 10.0, 100.0)
    assert a[1:] == b[1:] and _same(a[0].final(), b[0].final())
    s1, s2 = O.Sim(A, T, lambda j: one, seed, "random"), O.Sim(A, T, lambda j: one, seed, "random", 10.0, 100.0)
    assert s1.launch(2, -1) == s2.launch(2, -1) and _same(s1.o.final(), s2.o.final())
    # lookahead_ref, lookahead_policy_ref, lookahead_width_ref
    assert _same(LA.policy_walk(A, T, one, seed, "nearest"), LA.policy_walk(A, T, one, seed, "nearest", max_time=100.0))
    assert _same(LA.lookahead_values(A, T, one, seed, 1), LA.lookahead_values(A, T, one, seed, 1, max_time=100.0))
    assert _same(LP.lookahead_walk(A, T, one, seed, "nearest"), LP.lookahead_walk(A, T, one, seed, "nearest", 10.0, 100.0))
    assert _same(LP.lookahead_window(A, T, one, seed, "nearest", 10.0, 2, 2), LP.lookahead_window(A, T, one, seed, "nearest", 10.0, 2, 2, 100.0))
    assert _same(LW.width_walk(A, T, one, seed, "nearest", 2), LW.width_walk(A, T, one, seed, "nearest", 2, 10.0, 100.0))
    # removal_ref
    walk = lambda *mt: RR.walk_episode(oracle.OracleEnv(A, T).load(**one), inst["req"][0], seed, *mt)
    assert _same(walk(), walk(100.0))
    # renewal_ref
    assert _same(R.oracle_chain(A, T, 40, B, seed)[0], R.oracle_chain(A, T, 40, B, seed, policy="random", mwt=10.0, max_time=100.0)[0])
    # ... and another max_time is another episode
    assert O.episodes(A, T, one, seed, "nearest", 1, max_time=20.0)[0]["n_steps"] < O.episodes(A, T, one, seed, "nearest", 1)[0]["n_steps"]
    assert LA.policy_walk(A, T, one, seed, "nearest", max_time=20.0)["n_steps"] == O.episodes(A, T, one, seed, "nearest", 1, max_time=20.0)[0]["n_steps"]
