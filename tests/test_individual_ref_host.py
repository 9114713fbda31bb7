"""The persistent rollout under individual selection (dcm_rollout_individual; BatchedTaskEnv.rollout(policy, individual=True)), host
side.  The reference layer of its GPU tests (individual_ref.py) must show something at the shapes those tests use: the walk differs
from the leader-follower walk of the same instance and seed, and the cases reach what the form changes.  Then the symbol, its
prototype and ctypes signature, its place in the v5 additions list, where the kernels live, and the argument errors raised before
anything touches a device.  No GPU."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import individual_ref as IS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "dcmrta_amd", "csrc")
GREEDY = [(p, q) for p, q in IS.POLICIES if q == 0]


# ---------------------------------------------------------------------------------- 1-3: the oracle alone
@pytest.mark.parametrize("name", list(IS.ALL))
def test_the_walk_is_not_the_leader_follower_walk(oracle_lib, name):
    """a grouped kernel cannot pass a GPU case by accident: per env and policy the decision count differs, or the result does"""
    for policy, _ in (GREEDY if name in IS.CASES else [("random", 0)]):
        for b, (eps, (gw, gr)) in enumerate(zip(IS.walks(name, policy), IS.grouped(name, policy))):
            f = IS.final(eps[0])
            assert gw["n_steps"] != f["n_steps"] or gr["reward"] != f["reward"] or not np.array_equal(gr["finished"], f["finished"]) \
                or not np.array_equal(gr["travel_dist"], f["travel_dist"]), (name, policy, b)


def test_the_cases_have_the_kernel_instantiations_they_are_named_for():
    from dcmrta_amd.roofline import sim_kind_name
    for name, c in IS.CASES.items():
        assert c["sim"] == sim_kind_name(c["A"], c["T"], wide=c.get("kw", {}).get("member_cap", 5) > 5), name
    kinds = {sim_kind_name(c["A"], c["T"], wide=c.get("kw", {}).get("member_cap", 5) > 5) for c in IS.CASES.values()}
    assert len(kinds) == 7 and IS.CASES["10A64T"]["T"] + 1 > 64        # seven instantiations of with_sim's table + the no-depot-lane shape
    assert sim_kind_name(IS.RAGGED["A"], IS.RAGGED["T"], ragged=True) == sim_kind_name(6, 12)


@pytest.mark.parametrize("name", list(IS.CASES))
def test_every_case_reaches_what_the_form_changes(oracle_lib, name):
    c = IS.CASES[name]
    for policy, q32 in IS.POLICIES:
        for b, eps in enumerate(IS.walks(name, policy, q32)):
            w = eps[0]
            # a later decider of the event stands beside the decider and the picked task has vacancy > 1: leader-follower draws followers
            assert w["followers"] >= 1, (name, policy, q32, b)
            assert (w["mask"][np.arange(w["n_steps"]), w["action"]] == 0).all()
            assert w["n_steps"] == len(w["decider"]) > c["A"]
    firsts = [eps[0] for eps in IS.walks(name, "first")]
    randoms = [eps[0] for eps in IS.walks(name, "random")]
    # an episode that ends at max_time with work left
    assert all(w["at_max_time"] and not IS.final(w)["finished"].all() and IS.final(w)["flags"] == IS.DONE for w in randoms), name
    if c["max_time"] == 100.0 and name != "10A64T":
        # an episode that finishes every task, and depot decisions beside another decider (leader-follower would send the group)
        assert all(IS.final(w)["finished"].all() and IS.final(w)["flags"] == IS.DONE | IS.FINISHED for w in firsts), name
        assert all(w["depot_beside"] >= 1 for w in firsts), name


@pytest.mark.parametrize("name", list(IS.SHORT_WAIT))
def test_a_short_waiting_time_abandons(oracle_lib, name):
    for b, eps in enumerate(IS.walks(name, "random")):
        f = IS.final(eps[0])
        assert f["abandonments"] >= 10 and IS.abandoned_counts(eps[0]).sum() == f["abandonments"], (name, b)
        assert f["n_steps"] > IS.final(IS.walks(name.split("-")[0], "random")[b][0])["n_steps"]


@pytest.mark.parametrize("name", ["6A12T", "50A200T"])
def test_the_endpoints_of_explore_q32_on_the_oracle(oracle_lib, name):
    """explore_q32 = 0 is the greedy walk, 2^32 the random walk, decision by decision"""
    for policy in ("first", "nearest"):
        for b in range(IS.CASES[name]["B"]):
            lo, hi = IS.walks(name, policy, 0)[b][0], IS.walks(name, policy, 1 << 32)[b][0]
            rnd = IS.walks(name, "random")[b][0]
            for k in ("decider", "action", "mask"):
                assert np.array_equal(hi[k], rnd[k]), (name, policy, b, k)
            assert IS.final(hi)["reward"] == IS.final(rnd)["reward"] and hi["n_steps"] == rnd["n_steps"]
            part = IS.walks(name, policy, IS.Q25)[b][0]
            assert not np.array_equal(part["action"], lo["action"]) and not np.array_equal(part["action"], rnd["action"])


def test_the_running_counter_and_the_stop(oracle_lib):
    """consecutive episodes share the decision counter (the second `random` episode differs from the first), and a walk stopped at k
    is the prefix of the whole walk"""
    name = "6A12T"
    c = IS.CASES[name]
    inst, seeds = IS.instances(name)
    import oracle_ref as O
    for b, eps in enumerate(IS.walks(name, "random", 0, 2)):
        assert not np.array_equal(eps[0]["action"], eps[1]["action"])
        again = IS.walk(c["A"], c["T"], O.one(inst, b), seeds[b], "random", d0=eps[0]["n_steps"])
        assert np.array_equal(again["action"], eps[1]["action"])
        cut = IS.walk(c["A"], c["T"], O.one(inst, b), seeds[b], "random", stop=7)
        assert not cut["ended"] and cut["n_steps"] == 7 and np.array_equal(cut["action"], eps[0]["action"][:7])
        assert np.array_equal(cut["obs"][0], eps[0]["mask"][6])


# ---------------------------------------------------------------------------------- 4-10: the surface
def test_header_declares_dcm_rollout_individual_and_the_abi_is_still_5():
    from dcmrta_amd import _lib
    assert hasattr(C.CDLL(_lib.LIB_PATH), "dcm_rollout_individual")
    header = open(_lib.HEADER_PATH).read()
    p = r"\s*\*\s*"
    proto = re.search(r"int\s+dcm_rollout_individual\s*\(\s*dcm_env" + p + r"env,\s*int32_t\s+policy,\s*uint64_t\s+explore_q32,\s*int32_t\s+episodes,\s*"
                      r"int64_t\s+max_decisions,\s*const\s+int64_t" + p + r"max_decisions_in,\s*float" + p + r"agents_out,\s*float" + p +
                      r"tasks_out,\s*uint8_t" + p + r"mask_out,\s*int64_t" + p + r"steps_out,\s*void" + p + r"stream\s*\)\s*;", header)
    assert proto
    abi = re.search(r"#define\s+DCM_ABI_VERSION\s+5\b(.*)", header)
    assert abi and _lib.ABI_VERSION == 5
    assert "still v5" in abi.group(1) and "dcm_rollout_individual" in abi.group(1).split("still v5")[1]
    comment = re.sub(r"\s*\n \* ?", " ", header[:proto.start()].rsplit("/*", 1)[1])        # (a phrase may stand across a line break)
    for word in ("run_test_IS", "ascending id", "agent_step", "steps_out", "DCM_PARAM_NO_GROUPING", "DCM_ERR_INVALID", "DCM_ERR_STATE",
                 "best log", "SIZES", "dcm_step", "explore_q32", "depot"):
        assert word in comment, word
    flag = header[:header.index("#define DCM_PARAM_NO_GROUPING")].rsplit("/*", 1)[1]
    assert "dcm_rollout_individual" in flag and "always groups" not in flag


def test_ctypes_signature():
    from dcmrta_amd import _lib
    res, args = _lib.SIGNATURES["dcm_rollout_individual"]
    assert res is C.c_int and args == _lib.SIGNATURES["dcm_rollout_explore"][1]
    assert args == [C.c_void_p, C.c_int32, C.c_uint64, C.c_int32, C.c_int64] + [C.c_void_p] * 6


def test_the_form_is_a_macro_of_the_general_text_in_a_unit_of_its_own():
    form = open(os.path.join(CSRC, "k_form.inc")).read()
    assert re.search(r"#elif defined\(DCM_INDIVIDUAL\)\n#define KPREFIX KFORM_PICK\(k_is_, k_isrn_\)\n"
                     r"#define KPOLICY_PARAM , int policy, uint64_t explore_q32, RouteLog lg\n", form)
    # refused: another form macro beside it, the size-renewing form, every text but k_rollout_random
    others = r"defined\(DCM_POLICY\) \|\| defined\(DCM_LOG\) \|\| defined\(DCM_EXPLORE\) \|\| defined\(DCM_BEST\) \|\| defined\(DCM_LOOKAHEAD\)"
    assert re.search(r"#if defined\(DCM_INDIVIDUAL\) && \(" + others + r"\)\n#error", form)
    assert re.search(r"#if defined\(DCM_INDIVIDUAL\) && DCM_RENEW == 2\n#error", form)
    assert re.search(r"#if defined\(DCM_INDIVIDUAL\) && !defined\(KINDIVIDUAL_FORM\)\n#error", form)
    assert "#undef KINDIVIDUAL_FORM" in open(os.path.join(CSRC, "k_form_end.inc")).read()
    texts = [f for f in os.listdir(CSRC) if f.endswith(".inc") and "KINDIVIDUAL_FORM 1" in open(os.path.join(CSRC, f)).read()]
    assert texts == ["k_rollout_random.inc"]
    hpp = open(os.path.join(CSRC, "rollout_individual.hpp")).read()
    code = "\n".join(line.split("//")[0] for line in hpp.splitlines())
    assert code.count('#include "k_rollout_random.inc"') == 2 and "k_rollout_fast" not in code
    assert "atomic" not in code and "asm" not in code                    # plain C++ and vector stores; no atomics of its own
    src = open(os.path.join(CSRC, "dcmrta_env.hip")).read()
    assert re.search(r'#ifdef DCM_HAVE_INDIVIDUAL\n#include "rollout_individual.hpp"\n#endif', src) and src.count('"rollout_individual.hpp"') == 1
    assert "launch_rollout_individual" in src and "allow_lds_individual" in src
    body = src[src.index("int rollout_form("):]
    assert body[:body.index("\n}\n")].count("plan::form_rollout_kind(") == 1
    mk = open(os.path.join(CSRC, "Makefile")).read()
    assert re.search(r"^FLAGS_env_i\s*=\s*\$\(SPLIT\) \$\(SCHED\) -DDCM_TU_I\s*$", mk, re.M) and re.search(r"^UNITS :=.*\benv_i\b", mk, re.M)
    assert re.search(r"^ASM_UNITS :=.*\b_i\b", mk, re.M)
    # the three call sites of the text
    text = open(os.path.join(CSRC, "k_rollout_random.inc")).read()
    assert "S.pick_leader(h, lane, -1, k1, gm, true)" in text and "S.advance(h, P, lane, row PH_PASS, true)" in text
    assert "row PH_PASS, lg, e * BA, true, 0, true, false, &xy)" in text


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
    with pytest.raises(DcmError, match="individual_selection=True"):
        _bare().rollout("nearest", individual=True)
    with pytest.raises(DcmError, match="no lookahead form"):
        _bare(individual_selection=True).rollout("nearest", individual=True, lookahead=True)
    with pytest.raises(DcmError, match="width / return_inner"):
        _bare(individual_selection=True).rollout("nearest", individual=True, width=2)
    with pytest.raises(DcmError, match="width / return_inner"):
        _bare(individual_selection=True).rollout("nearest", individual=True, return_inner=True)
    with pytest.raises(DcmError, match="explore needs a greedy base policy"):
        _bare(individual_selection=True).rollout("random", individual=True, explore=0.5)
    with pytest.raises(DcmError, match="policy must be one of"):
        _bare(individual_selection=True).rollout("best", individual=True)


def test_the_tools_take_the_flag():
    for tool in ("policy_time.py", "sample_plan.py"):
        text = open(os.path.join(ROOT, "tools", tool)).read()
        assert '"--individual"' in text and "individual_selection=" in text and "individual=" in text, tool
