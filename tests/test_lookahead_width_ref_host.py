"""The width-limited device lookahead (dcm_rollout_lookahead_width; BatchedTaskEnv.rollout(policy, lookahead=True, width=W)), host side.
The reference layer of its GPU tests (lookahead_width_ref.py) must show something at the shapes those tests use, proved from the oracle
alone: width 1 is `nearest`, width >= T is the all-actions lookahead, widths 2 and 3 are neither and differ from each other, the tie
cases do tie where they say, and every window case launches the Sim<> instantiation it is there for.  Then the symbol, its prototype
and ctypes signature, its place in the v5 additions list, and the argument errors raised before anything touches a device.  No GPU."""
import ctypes as C
import re

import numpy as np
import pytest

import lookahead_policy_ref as LP
import lookahead_ref as LA
import lookahead_width_ref as LW

POLICIES = ["random", "first", "nearest"]


@pytest.mark.parametrize("policy", POLICIES)
@pytest.mark.parametrize("name", list(LP.TINY))
def test_the_tiny_cases_show_something(oracle_lib, name, policy):
    A, T, B, _ = LP.TINY[name]
    nearest, full = LW.nearest_walks(name), LP.walks(name, policy)
    w1, w2, w3, wt = (LW.walks(name, policy, width) for width in (1, 2, 3, T))
    for b in range(B):
        # width 1 is `nearest`, action for action, and costs no inner decision
        assert np.array_equal(w1[b]["action"], nearest[b]["action"]) and np.array_equal(w1[b]["leader"], nearest[b]["leader"]), b
        assert w1[b]["inner"] == 0 and not any(f["cand"] for f in w1[b]["facts"]), b
        # width >= T is the all-actions lookahead
        assert np.array_equal(wt[b]["action"], full[b]["action"]) and LA.pair(wt[b]["result"]) == LA.pair(full[b]["result"]), b
        for w, width in ((w2[b], 2), (w3[b], 3)):
            assert w["flags"] & LP.DONE and w["inner"] > 0
            for f in w["facts"]:                                # the list is `width` long unless fewer tasks are unmasked, or one is
                assert len(f["cand"]) == (0 if f["n_unmasked"] < 2 else min(width, f["n_unmasked"])), (b, f["d"])
                assert w["chosen"][f["d"]] in (f["cand"] or [w["chosen"][f["d"]]])
    differs = [not np.array_equal(w2[b]["action"], nearest[b]["action"]) and not np.array_equal(w2[b]["action"], full[b]["action"])
               for b in range(B)]
    assert any(differs), "width 2 is `nearest` or the all-actions lookahead in every env: the case shows nothing"
    assert any(not np.array_equal(w3[b]["action"], w2[b]["action"]) for b in range(B)), "width 3 is width 2 in every env"
    # the explicit index tie-break decides somewhere: the best pair belongs to two candidates and the first valued is not the lowest
    reordered = 0
    for w in w2 + w3:
        for f in w["facts"]:
            if LW.value_ties(f):
                holders = [act for act in f["cand"] if f["pairs"][act] == max(f["pairs"].values())]
                reordered += holders[0] != min(holders)
                assert w["chosen"][f["d"]] == min(holders)
    assert reordered >= 1, "no decision needs the index tie-break"


def test_width_cuts_the_inner_decisions(oracle_lib):
    """the issue's figures for 10A20T under `nearest`: the all-actions form against widths 2 and 3"""
    full, w2, w3 = (LW.walks("10A20T", "nearest", width) for width in (0, 2, 3))
    assert [(full[b]["inner"], w2[b]["inner"], w3[b]["inner"]) for b in range(2)] == [(9008, 2380, 2526), (8697, 2111, 2597)]
    for b, w in enumerate(LP.walks("10A20T", "nearest")):
        assert np.array_equal(full[b]["action"], w["action"]), b


def test_candidates_are_nearests_picks_in_order():
    task_xy = np.array([[3.0, 0.0], [1.0, 0.0], [0.0, 1.0], [2.0, 0.0], [0.0, -1.0]])
    mask = np.array([1, 0, 0, 0, 1, 0], np.uint8)               # task 3 (action 4) is masked
    assert LW.candidates(mask, (0.0, 0.0), task_xy, 2) == [2, 3]            # distance 1 three times: the lower indices
    assert LW.candidates(mask, (0.0, 0.0), task_xy, 3) == [2, 3, 5]
    assert LW.candidates(mask, (0.0, 0.0), task_xy, 9) == [2, 3, 5, 1]      # no more than are unmasked
    assert mask.tolist() == [1, 0, 0, 0, 1, 0]
    assert LW.candidates(np.array([0, 1, 1, 1, 1, 1], np.uint8), (0.0, 0.0), task_xy, 2) == []   # only the depot


@pytest.mark.parametrize("name", list(LW.WINDOWS))
def test_the_window_cases_meet_what_they_are_there_for(oracle_lib, name):
    from dcmrta_amd.roofline import sim_kind_name
    c = LW.WINDOWS[name]
    assert LW.SIM_KINDS[name] in sim_kind_name(c["A"], c["T"]).replace(" ", ""), sim_kind_name(c["A"], c["T"])
    inst, _ = LW.window_instances(name)
    ws = LW.windows(name)
    assert len(ws) == c["B"] == 2 and c["K"] <= 2
    for b, x in enumerate(ws):
        w = x["window"]
        assert not w["ended"] and w["n_steps"] == x["d0"] + c["K"] and len(w["facts"]) == c["K"] and w["inner"] > 0, b
        assert all(len(f["cand"]) == c["width"] < f["n_unmasked"] for f in w["facts"]), b
        assert x["tail"]["n_steps"] > w["n_steps"]
    facts = [[f for f in x["window"]["facts"]] for x in ws]
    if name == "ties-cut":          # the cut falls between two twins at decision d0 of every env: the lower index is the candidate
        for b, fs in enumerate(facts):
            f, half = fs[0], c["T"] // 2
            assert LW.cut_ties(f, c["width"]), b
            last = f["cand"][-1]
            assert last <= half and last + half not in f["cand"] and f["dist"][last] == f["dist"][last + half], (b, f["cand"])
    if name == "ties-in":           # both twins of a pair are in the list, the lower index first
        for b, fs in enumerate(facts):
            assert all(LW.candidate_ties(f) for f in fs), b
            f, half = fs[0], c["T"] // 2
            assert any(k + half in f["cand"] and f["cand"].index(k) + 1 == f["cand"].index(k + half) for k in f["cand"]), (b, f["cand"])
    if name.startswith("ties"):
        xy = inst["task_xy"]
        assert np.array_equal(xy[:, :c["T"] // 2], xy[:, c["T"] // 2:])
    if name == "ties-cut":
        assert any(LW.value_ties(f) for fs in facts for f in fs)
    if name == "lane-owns-two":     # tasks 3 and 67 = 3 + 64 belong to lane 3, lie at one point, and are the two nearest at decision d0
        i, j = c["same"]
        assert (j - i) % 64 == 0 and np.array_equal(inst["task_xy"][:, i], inst["task_xy"][:, j])
        for b, fs in enumerate(facts):
            assert fs[0]["cand"][:2] == [i + 1, j + 1] and LW.candidate_ties(fs[0]), (b, fs[0]["cand"])
    if name == "one-chunk-64":
        assert c["T"] == 64                                     # every lane owns a task: none is left for the depot


def test_the_ragged_case_runs_each_env_at_its_own_sizes(oracle_lib):
    _, A, T, sizes = LP.RAGGED
    for b, (w, full, (a, t)) in enumerate(zip(LW.ragged_walks(), LP.ragged_walks(), sizes)):
        assert w["mask"].shape[1] == t + 1 and w["followers"].shape[1] == a and w["flags"] & LP.DONE and w["inner"] > 0, b
        assert all(len(f["cand"]) in (0, 2) for f in w["facts"]), b
    assert any(not np.array_equal(w["action"], full["action"]) for w, full in zip(LW.ragged_walks(), LP.ragged_walks()))


def test_header_declares_dcm_rollout_lookahead_width_and_the_abi_is_still_5():
    from dcmrta_amd import _lib
    assert hasattr(C.CDLL(_lib.LIB_PATH), "dcm_rollout_lookahead_width")
    header = open(_lib.HEADER_PATH).read()
    p = r"\s*\*\s*"
    proto = re.search(r"int\s+dcm_rollout_lookahead_width\s*\(\s*dcm_env" + p + r"env,\s*int32_t\s+base_policy,\s*int32_t\s+width,\s*int32_t\s+episodes,\s*"
                      r"int64_t\s+max_decisions,\s*const\s+int64_t" + p + r"max_decisions_in,\s*float" + p + r"agents_out,\s*float" + p +
                      r"tasks_out,\s*uint8_t" + p + r"mask_out,\s*int64_t" + p + r"steps_out,\s*int64_t" + p + r"inner_out,\s*void" + p +
                      r"stream\s*\)\s*;", header)
    assert proto
    abi = re.search(r"#define\s+DCM_ABI_VERSION\s+5\b(.*)", header)
    assert abi and _lib.ABI_VERSION == 5
    assert "still v5" in abi.group(1) and "dcm_rollout_lookahead_width" in abi.group(1).split("still v5")[1]
    comment = header[:proto.start()].rsplit("/*", 1)[1]
    for word in ("width = 0 and inner_out = NULL", "W == 1", "DCM_POLICY_NEAREST", "ROUNDED fp64", "lower index", "LOWEST ACTION INDEX",
                 "inner_out", "INSIDE inner episodes", "but its first", "steps_out", "DCM_ERR_INVALID for width < 0",
                 "every message names\n * dcm_rollout_lookahead_width"):
        assert word in comment, word


def test_ctypes_signature():
    from dcmrta_amd import _lib
    res, args = _lib.SIGNATURES["dcm_rollout_lookahead_width"]
    old = _lib.SIGNATURES["dcm_rollout_lookahead"][1]
    # the old entry's with width behind the base policy and inner_out in front of the stream
    assert res is C.c_int and args == old[:2] + [C.c_int32] + old[2:-1] + [C.c_void_p] + old[-1:]
    assert args == [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int64] + [C.c_void_p] * 7


def _bare(**kw):
    from dcmrta_amd.batched_env import BatchedTaskEnv
    env = BatchedTaskEnv.__new__(BatchedTaskEnv)
    attrs = dict(_h=None, B=4, A=20, T=50, member_cap=5, device="cuda:0", max_waiting_time=10.0, max_time=100.0, auto_reset=False,
                 individual_selection=False, strict_mask=False, n_tasks=None, n_agents=None)
    attrs.update(kw)
    for k, v in attrs.items():
        setattr(env, k, v)
    return env


def test_argument_errors_need_no_device():
    from dcmrta_amd._lib import DcmError
    for policy in POLICIES:
        with pytest.raises(DcmError, match="give lookahead=True"):
            _bare().rollout(policy, width=2)
    with pytest.raises(DcmError, match="give lookahead=True"):
        _bare().rollout("nearest", return_inner=True)
    for width in (-1, 2.0, "3", None, True, np.float64(2)):
        with pytest.raises(DcmError, match="width must be an integer >= 0"):
            _bare().rollout("nearest", lookahead=True, width=width)
    with pytest.raises(DcmError, match="width must be an integer >= 0"):
        _bare().rollout("nearest", width=-1)
    with pytest.raises(DcmError, match="cannot be combined with explore"):
        _bare().rollout("nearest", lookahead=True, width=2, explore=0.1)
