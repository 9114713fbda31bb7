"""The window cases of the device lookahead policy (lookahead_policy_ref.WINDOWS), host side: from the oracle alone, the table covers
what tests/test_gpu_lookahead_windows.py claims to test -- the overflow count table on every branch of lookahead_action's restore
(clean snapshot and a spilling inner episode, spilled snapshot, both within one decision), the MG shapes and the two-word agent mask
with a spilled snapshot, a ragged env below the layout's T with a spill, a wide task with more than five members, ties, choices that
leave the base policy, inner episodes that end at max_time -- at a cost a GPU test can pay, and every Sim<> instantiation of the
general kernel is launched.  The windowed walker is pinned to the full-episode one.  No GPU.

Measured here: the reference of all twelve cases together takes 45 s of one CPU core (spill-clean 2.1, spill-saved 0.8, spill-mixed
0.6, s20x50-spill 0.6, lay64 1.0, no-depot-lane 2.2, mc 9.4, c5 10.5, g2x3 8.2, g-ragged 6.0, rt 2.5, wide 0.1); it is computed once
per process and shared by every test of this file and of the GPU file.
The TRUNCATED inner ending (the oracle's zero-decider guard) was not reached: no inner episode of any case ends under it
(test_inner_episodes_that_end_truncated_are_on_record)."""
import numpy as np
import pytest

import lookahead_policy_ref as LP

AB_CAP = 16                 # entries of an agent's abandonment log (csrc/common.hpp); further ones go to the overflow count table
# A GPU window decision plays one inner episode per unmasked action to its end on ONE wave: at most 40 of them where T >= 130.  The
# one exception is the one-agent env of g-ragged (1, 130), where all 130 tasks stay unmasked to the end of the episode -- an agent
# alone finishes only the tasks that need one member -- and whose whole episode has about a hundred decisions, some twenty of them
# behind the window: its two window decisions cost about 259 x 20 inner decisions, less than ONE 40-action decision 200 decisions
# before the end of a larger env's episode.
UNMASKED_CAP, CAP_FROM_T = 40, 130


def facts(name):
    """(env, facts of one window decision) over a case"""
    return [(b, f) for b, x in enumerate(LP.windows(name)) for f in x["window"]["facts"]]


@pytest.mark.parametrize("name", list(LP.WINDOWS))
def test_every_window_is_whole_and_affordable(oracle_lib, name):
    c = LP.WINDOWS[name]
    d0s, lengths = LP.window_starts(name)
    inst, seeds, sz = LP.window_instances(name)
    assert len(sz) == c["B"] and 1 <= c["K"] <= 4
    for b, x in enumerate(LP.windows(name)):
        w, tail = x["window"], x["tail"]
        assert 0 <= x["d0"] == d0s[b] < lengths[b]
        # the window ends inside the episode, K lookahead decisions were taken, and the tail carries on from them
        assert not w["ended"] and w["n_steps"] == x["d0"] + c["K"] == x["stop"]["decisions"] and len(w["facts"]) == c["K"], (name, b)
        assert tail["n_steps"] > w["n_steps"] and np.array_equal(tail["action"][:w["n_steps"]], w["action"]), (name, b)
        assert np.array_equal(tail["leader"][:w["n_steps"]], w["leader"]) and tail["flags"] & LP.DONE
        assert [f["d"] for f in w["facts"]] == list(range(x["d0"], x["d0"] + c["K"]))
        for f in w["facts"]:
            assert w["mask"][f["d"], w["action"][f["d"]]] == 0
            if sz[b][1] >= CAP_FROM_T and sz[b][0] > 1:
                assert f["n_unmasked"] <= UNMASKED_CAP, (name, b, f)
        if sz[b][0] == 1:                                                   # the exception stated at UNMASKED_CAP
            assert tail["n_steps"] - x["d0"] < 25 and c["K"] <= 2, (name, b, tail["n_steps"], x["d0"])
    print(name, LP.window_sim_kind(name), "d0", d0s, "of", lengths, "unmasked", [f["n_unmasked"] for _, f in facts(name)])


def test_spill_clean_zeroes_a_table_nothing_was_saved_of(oracle_lib):
    """d0 = 0, so the first lookahead launch of the handle (which allocates the snapshot buffer) is the window's"""
    assert set(LP.window_starts("spill-clean")[0]) == {0}
    assert any(f["most0"] <= AB_CAP and f["most1"] and f["most1"][1] > AB_CAP for _, f in facts("spill-clean"))
    assert all(f["most0"] <= AB_CAP for _, f in facts("spill-clean"))


@pytest.mark.parametrize("name", ["spill-saved", "mc", "c5", "g2x3"])
def test_every_snapshot_of_these_cases_has_spilled(oracle_lib, name):
    for b, f in facts(name):
        assert f["most0"] > AB_CAP and f["n_unmasked"] > 1 and f["most1"][0] >= f["most0"], (name, b, f)


def test_spill_mixed_has_inner_episodes_on_both_sides_of_the_cap_within_one_decision(oracle_lib):
    assert any(f["most0"] <= AB_CAP and f["most1"] and f["most1"][0] <= AB_CAP < f["most1"][1] for _, f in facts("spill-mixed"))


def test_the_compile_time_20x50_case_spills(oracle_lib):
    assert all(f["most0"] > AB_CAP for _, f in facts("s20x50-spill"))


def test_the_ragged_case_spills_below_the_layouts_sizes(oracle_lib):
    c = LP.WINDOWS["g-ragged"]
    _, _, sz = LP.window_instances("g-ragged")
    assert len(sz) >= 4 and {(1, 130), (65, 128), (64, 129), (70, 65)} <= set(sz) and max(s[0] for s in sz) == c["A"]
    small = [(b, f) for b, f in facts("g-ragged") if sz[b][1] < c["T"] and f["n_unmasked"] > 1]
    assert any(f["most0"] > AB_CAP for b, f in small), small
    assert any(sz[b][0] < c["A"] and f["most0"] > AB_CAP for b, f in small), small
    # ... and envs that never spill sit beside them: a slice pitch taken from the env's own sizes lands in a neighbour
    assert any(f["most1"] and f["most1"][1] <= AB_CAP for _, f in facts("g-ragged"))


def test_the_wide_case_holds_more_than_five_members_through_a_snapshot(oracle_lib):
    assert any(f["members"] > 5 and f["n_unmasked"] > 1 for _, f in facts("wide"))
    assert LP.window_instances("wide")[0]["req"].max() > 5


def test_ties_departures_and_max_time_endings_are_met(oracle_lib):
    every = [(n, b, f) for n in LP.WINDOWS for b, f in facts(n)]
    multi = [x for x in every if x[2]["n_unmasked"] > 1]
    assert any(f["tie"] for _, _, f in multi), "no decision whose best pair belongs to two actions: a tie must keep the lowest"
    assert any(f["differs"] for _, _, f in multi), "the lookahead never leaves the base policy's pick"
    assert any(f["at_max_time"] for _, _, f in multi) and any(f["at_max_time"] == 0 for _, _, f in multi)
    # per case: which of them it shows (for the record)
    for n in LP.WINDOWS:
        fs = [f for _, f in facts(n)]
        print(n, "ties", sum(f["tie"] for f in fs), "differs", sum(f["differs"] for f in fs), "inner episodes at max_time",
              sum(f["at_max_time"] for f in fs), "most0", [f["most0"] for f in fs], "most1", [f["most1"] for f in fs])


def test_inner_episodes_that_end_truncated_are_on_record(oracle_lib):
    """out of scope for the GPU test; the search result is stated in the module docstring"""
    found = {n: sum(f["truncated"] for _, f in facts(n)) for n in LP.WINDOWS}
    print("inner episodes that ended TRUNCATED:", found)
    assert not any(found.values()), ("a case reaches the TRUNCATED inner ending: say so in the module docstring", found)


@pytest.mark.parametrize("policy", ["nearest", "first"])
def test_the_windowed_walker_is_the_full_episode_walker(oracle_lib, policy):
    """lookahead_window with d0 = 0 and K = the episode's length is lookahead_walk"""
    import oracle_ref as O
    name = "5A8T"
    A, T, B, _ = LP.TINY[name]
    inst, seeds = LP.instances(name)
    for b, old in enumerate(LP.walks(name, policy)):
        w = LP.lookahead_window(A, T, O.one(inst, b), seeds[b], policy, 10.0, 0, old["n_steps"])
        assert w["ended"] and w["n_steps"] == old["n_steps"]
        for k in ("action", "leader", "nfol", "followers", "mask"):
            assert np.array_equal(w[k], old[k]), (policy, b, k)
        assert np.array_equal([f["n_unmasked"] for f in w["facts"]], old["n_unmasked"])
        assert np.array_equal([f["differs"] for f in w["facts"]], old["action"] != old["base_action"])
        tail = LP.window_tail(A, T, O.one(inst, b), seeds[b], policy, 10.0, w["chosen"])
        assert tail["flags"] == old["flags"] and tail["result"]["reward"] == old["result"]["reward"]


def test_the_renewing_window_lies_across_the_end_of_the_first_episode(oracle_lib):
    """the k_larn_* case at 50A/200T: the lookahead plays the last decisions of episode 1 (returns to the depot, one allowed action
    each: the snapshots of this case are those of the decision behind the restart, where every task is unmasked, on the renewed
    instance) and the budget leaves exactly one decision for episode 2.  Some env ends episode 1 with a spilled count table, which
    the restart must clear."""
    from dcmrta_amd.roofline import sim_kind_name
    c = LP.RENEWING
    assert sim_kind_name(c["A"], c["T"]) == "<50,200,false>"
    _, _, ws = LP.renewing_windows()
    for x in ws:
        assert x["K"] == x["end"] - x["d0"] + 1 >= 2 and x["window"]["ended"] and len(x["window"]["facts"]) == x["K"] - 1
    assert any(f["most0"] > AB_CAP for x in ws for f in x["window"]["facts"])
    print("renewing:", [(x["d0"], x["end"], x["K"], [f["n_unmasked"] for f in x["window"]["facts"]]) for x in ws])


def test_every_instantiation_of_the_lookahead_form_is_launched():
    """plan::sim_kind through roofline.sim_kind_name (pinned to csrc/plan.hpp by test_host.py): the window cases reach all eight
    Sim<> instantiations of lookahead_general; tests/test_gpu_lookahead_policy.py reaches the three listed here (and <128,256,true>
    only with A <= 64)."""
    from dcmrta_amd.roofline import SIM_KINDS, sim_kind_name
    kinds = {n: LP.window_sim_kind(n) for n in LP.WINDOWS}
    assert kinds == {"spill-clean": "<20,50,true>", "spill-saved": "<20,50,true>", "spill-mixed": "<20,50,true>", "s20x50-spill": "<20,50,false>",
                     "lay64": "<64,64,true>", "no-depot-lane": "<64,64,true>", "mc": "<50,200,false>", "c5": "<100,500,false>",
                     "g2x3": "<128,256,true>", "g-ragged": "<128,256,true>", "rt": "<0,0,false>", "wide": "<0,0,false,MW>"}
    assert set(kinds.values()) == set(SIM_KINDS)
    # the policy file's shapes: its tiny and ragged cases, and PLAN_CASES
    policy_file = {sim_kind_name(5, 8), sim_kind_name(10, 20), sim_kind_name(10, 20, ragged=True), sim_kind_name(20, 50),
                   sim_kind_name(12, 70), sim_kind_name(10, 20, wide=True)}
    assert policy_file == {"<20,50,true>", "<20,50,false>", "<128,256,true>", "<0,0,false,MW>"}
    # two agent words: A > 64 on <128,256,true> (uniform and ragged), on <100,500,false> and on <0,0,false>
    assert all(LP.WINDOWS[n]["A"] > 64 for n in ("g2x3", "g-ragged", "c5", "rt"))
    # MG = (CT > 64) && !RS: the member arrival times in the HBM record
    assert {n for n, k in kinds.items() if k in ("<50,200,false>", "<100,500,false>")} == {"mc", "c5"}
