"""The device lookahead policy (dcm_rollout_lookahead; BatchedTaskEnv.rollout(policy, lookahead=True)), host side.  The reference layer
of its GPU tests (lookahead_policy_ref.py) must show something at the tiny shapes those tests use: the lookahead never ends below the
base policy, it does take other actions than the base policy, some decisions have masked tasks, and the seed-shift identity that
gives the reference for second episodes holds on the oracle.  Then the symbol, its prototype and ctypes signature, its place in the v5
additions list, where the kernels live, and the argument errors raised before anything touches a device.  No GPU."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import lookahead_policy_ref as LP
import lookahead_ref as LA
import oracle_ref as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "dcmrta_amd", "csrc")


@pytest.mark.parametrize("policy", ["nearest", "first"])
@pytest.mark.parametrize("name", list(LP.TINY))
def test_the_tiny_cases_show_something(oracle_lib, name, policy):
    A, T, B, _ = LP.TINY[name]
    inst, seeds = LP.instances(name)
    differs = masked = 0
    for b, w in enumerate(LP.walks(name, policy)):
        base = O.episodes(A, T, O.one(inst, b), seeds[b], policy, 1)[0]
        assert LA.pair(w["result"]) >= LA.pair(base), (b, LA.pair(w["result"]), LA.pair(base))
        assert w["flags"] & LP.DONE and w["n_steps"] == w["result"]["n_steps"] == len(w["base_action"])
        differs += bool((w["action"] != w["base_action"]).any())
        masked += bool((w["mask"][:, 1:] == 1).any())
        # every decision took an unmasked action, and the depot only when no task was unmasked
        for d in range(w["n_steps"]):
            assert w["mask"][d, w["action"][d]] == 0 and (w["action"][d] != 0 or w["mask"][d, 1:].all()), (b, d)
    assert differs >= 1, "the lookahead never leaves the base policy's actions: the case shows nothing"
    assert masked >= 1, "no decision has a masked task"


def test_the_ragged_case_runs_each_env_at_its_own_sizes(oracle_lib):
    _, A, T, sizes = LP.RAGGED
    inst, seeds = LP.ragged_instances()
    assert (inst["n_agents"].tolist(), inst["n_tasks"].tolist()) == ([s[0] for s in sizes], [s[1] for s in sizes])
    for b, (w, (a, t)) in enumerate(zip(LP.ragged_walks(), sizes)):
        assert w["mask"].shape[1] == t + 1 and w["followers"].shape[1] == a and w["flags"] & LP.DONE, b
        base = O.episodes(a, t, O.one(inst, b, t), seeds[b], "nearest", 1)[0]
        assert LA.pair(w["result"]) >= LA.pair(base), b


@pytest.mark.parametrize("policy", ["nearest", "random"])
def test_a_running_decision_counter_is_a_seed_shift_on_the_oracle(oracle_lib, policy):
    """O.episodes(..., 2)'s second episode -- counter running on from the first one's decisions -- is the one-episode run from counter
    0 under (seed + GAMMA n1) mod 2^64: choices, reward, finished tasks and metrics"""
    A, T, B, _ = LP.TINY["10A20T"]
    inst, seeds = LP.instances("10A20T")
    for b in range(B):
        one = O.one(inst, b)
        first, second = O.episodes(A, T, one, seeds[b], policy, 2, record=True)
        alone = O.episodes(A, T, one, LP.shifted_seed(seeds[b], first["n_steps"]), policy, 1, record=True)[0]
        assert alone["n_steps"] == second["n_steps"] and first["n_steps"] > 0
        for k in ("action", "leader", "nfol", "followers", "mask"):
            assert np.array_equal(alone[k], second[k]), (b, k)
        assert alone["reward"] == second["reward"] and np.array_equal(alone["finished"], second["finished"])
        assert np.array_equal(alone["metrics"], second["metrics"])
    assert LP.shifted_seed((1 << 64) - 1, 3) == (3 * LP.GAMMA - 1) % (1 << 64)


def test_header_declares_dcm_rollout_lookahead_and_the_abi_is_still_5():
    from dcmrta_amd import _lib
    assert hasattr(C.CDLL(_lib.LIB_PATH), "dcm_rollout_lookahead")
    header = open(_lib.HEADER_PATH).read()
    p = r"\s*\*\s*"
    proto = re.search(r"int\s+dcm_rollout_lookahead\s*\(\s*dcm_env" + p + r"env,\s*int32_t\s+base_policy,\s*int32_t\s+episodes,\s*int64_t\s+max_decisions,\s*"
                      r"const\s+int64_t" + p + r"max_decisions_in,\s*float" + p + r"agents_out,\s*float" + p + r"tasks_out,\s*uint8_t" + p +
                      r"mask_out,\s*int64_t" + p + r"steps_out,\s*void" + p + r"stream\s*\)\s*;", header)
    assert proto
    abi = re.search(r"#define\s+DCM_ABI_VERSION\s+5\b(.*)", header)
    assert abi and _lib.ABI_VERSION == 5
    assert "still v5" in abi.group(1) and "dcm_rollout_lookahead" in abi.group(1).split("still v5")[1]
    comment = header[:proto.start()].rsplit("/*", 1)[1]
    for word in ("finished tasks", "lowest index", "depot", "DCM_ERR_INVALID", "DCM_ERR_STATE", "max_waiting_time <= 0", "best log", "SIZES",
                 "captured", "FIRST call", "outer", "return log", "abandonment log", "steps_out", "observation"):
        assert word in comment, word


def test_ctypes_signature():
    from dcmrta_amd import _lib
    res, args = _lib.SIGNATURES["dcm_rollout_lookahead"]
    # env, base policy, episodes, max_decisions, max_decisions_in, obs x3, steps_out, stream: dcm_rollout_policy's
    assert res is C.c_int and args == _lib.SIGNATURES["dcm_rollout_policy"][1]
    assert args == [C.c_void_p, C.c_int32, C.c_int32, C.c_int64] + [C.c_void_p] * 6


def test_the_form_is_a_macro_of_the_general_text_in_a_unit_of_its_own():
    form = open(os.path.join(CSRC, "k_form.inc")).read()
    assert re.search(r"#elif defined\(DCM_LOOKAHEAD\)\n#define KPREFIX KFORM_PICK\(k_la_, k_larn_\)", form)
    # refused: another form macro beside it, the size-renewing form, every text but k_rollout_random
    assert re.search(r"defined\(DCM_BEST\) \+ defined\(DCM_LOOKAHEAD\) > 1\n#error", form)
    assert re.search(r"#if defined\(DCM_LOOKAHEAD\) && DCM_RENEW == 2\n#error", form)
    assert re.search(r"#if defined\(DCM_LOOKAHEAD\) && !defined\(KLOOKAHEAD_FORM\)\n#error", form)
    texts = [f for f in os.listdir(CSRC) if f.endswith(".inc") and "KLOOKAHEAD_FORM 1" in open(os.path.join(CSRC, f)).read()]
    assert texts == ["k_rollout_random.inc"]
    hpp = open(os.path.join(CSRC, "rollout_lookahead.hpp")).read()
    assert hpp.count('#include "k_rollout_random.inc"') == 2 and "k_rollout_fast" not in "\n".join(
        line.split("//")[0] for line in hpp.splitlines())
    code = "\n".join(line.split("//")[0] for line in hpp.splitlines())
    assert "atomic" not in code and "asm" not in code                    # plain C++ and vector stores; no atomics of its own
    src = open(os.path.join(CSRC, "dcmrta_env.hip")).read()
    assert re.search(r'#ifdef DCM_HAVE_LOOKAHEAD\n#include "rollout_lookahead.hpp"\n#endif', src) and src.count('"rollout_lookahead.hpp"') == 1
    mk = open(os.path.join(CSRC, "Makefile")).read()
    assert re.search(r"^FLAGS_env_a\s*=.*-DDCM_TU_A", mk, re.M) and re.search(r"^UNITS :=.*\benv_a\b", mk, re.M)


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
    from dcmrta_amd.batched_env import BatchedTaskEnv
    from dcmrta_amd.lookahead import Lookahead
    with pytest.raises(DcmError, match="cannot be combined with explore"):
        _bare().rollout("nearest", lookahead=True, explore=0.1)
    with pytest.raises(DcmError, match="cannot be combined with explore"):
        _bare().rollout("first", lookahead=True, explore_q32=7)
    with pytest.raises(DcmError, match="policy must be one of"):
        _bare().rollout("lookahead", lookahead=True)
    assert sorted(BatchedTaskEnv.POLICIES) == ["first", "nearest", "random"]    # the lookahead is a rule over a policy, not a policy
    with pytest.raises(DcmError, match="policy must be one of"):
        Lookahead(_bare(), "lookahead")
    import dcmrta_amd.lookahead as module
    assert "lookahead=True" in module.__doc__                                   # the host-driven form points to the device form
