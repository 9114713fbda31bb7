"""The epsilon-greedy device policies (dcm_rollout_explore), host side: the explore word of the choice protocol against the oracle's
mix64, the epsilon -> explore_q32 map, the symbol and its signature, the dispatch rule of csrc/plan.hpp compiled with the host compiler,
and the register budget of the epsilon-greedy kernel forms (k_ex_*, k_exrn_*) on the compiler's report.  No GPU."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
M64 = (1 << 64) - 1


def test_explore_word_is_the_definition_composed_from_the_oracles_mix64():
    import oracle
    from dcmrta_amd import choice
    assert choice.EXPLORE_SALT == 0xD6E8FEB86659FD93
    rng = np.random.default_rng(91)
    seeds = [0, 1, M64, choice.env_seed(11, 0)] + [int(x) for x in rng.integers(0, 1 << 63, 60, dtype=np.uint64)]
    ds = [0, 1, 63, 64, 65, 4095, (1 << 32) - 1, 1 << 40]
    words = []
    for s in seeds:
        for d in ds:
            key1 = oracle.mix64((s + choice.GAMMA * (d + 1)) & M64)
            w = oracle.mix64(key1 ^ 0xD6E8FEB86659FD93) >> 32
            assert choice.explore_word(s, d) == w and 0 <= w < 1 << 32, (s, d)
            # the comparison itself, at the ends and around the word
            assert not choice.explores(s, d, 0) and choice.explores(s, d, 1 << 32)
            assert choice.explores(s, d, w + 1) and not choice.explores(s, d, w)
            words.append(w)
    assert len(words) == 512 and len(set(words)) > 500                          # (not a constant, not a short cycle)
    # the word is not one of the decision's own draws: slot 1 stays what the random policy takes
    assert all(choice.explore_word(s, 0) not in (choice.draw(s, 0, 0), choice.draw(s, 0, 1), choice.draw(s, 0, 2)) for s in seeds[3:])


def test_explore_q32_maps_epsilon_by_floor():
    from dcmrta_amd import choice
    assert choice.explore_q32(0) == 0 and choice.explore_q32(0.0) == 0
    assert choice.explore_q32(1.0) == 1 << 32
    assert choice.explore_q32(0.05) == 214748364
    assert choice.explore_q32(0.5) == 1 << 31 and choice.explore_q32(0.25) == 1 << 30
    assert choice.explore_q32(np.nextafter(1.0, 0.0)) == (1 << 32) - 1
    for bad in (-0.01, 1.0000001, float("nan")):
        with pytest.raises(ValueError):
            choice.explore_q32(bad)


def test_library_exports_dcm_rollout_explore():
    from dcmrta_amd import _lib
    assert hasattr(C.CDLL(_lib.LIB_PATH), "dcm_rollout_explore")
    header = open(_lib.HEADER_PATH).read()
    assert re.search(r"#define\s+DCM_ABI_VERSION\s+5\b", header) and _lib.ABI_VERSION == 5          # an addition only
    assert re.search(r"int\s+dcm_rollout_explore\(dcm_env\s*\*env,\s*int32_t policy,\s*uint64_t explore_q32,\s*int32_t episodes,", header)
    # dcm_rollout_policy's arguments with explore_q32 behind the policy
    res, args = _lib.SIGNATURES["dcm_rollout_explore"]
    res0, args0 = _lib.SIGNATURES["dcm_rollout_policy"]
    assert res == res0 and args == args0[:2] + [C.c_uint64] + args0[2:]


def test_rollout_rejects_explore_with_the_random_policy_or_both_keywords():
    """The keyword checks of BatchedTaskEnv.rollout run before anything touches the device: on a bare object."""
    from dcmrta_amd.batched_env import BatchedTaskEnv
    from dcmrta_amd._lib import DcmError
    env = BatchedTaskEnv.__new__(BatchedTaskEnv)
    with pytest.raises(DcmError, match="greedy base policy"):
        env.rollout("random", explore=0.1)
    with pytest.raises(DcmError, match="greedy base policy"):
        env.rollout("random", explore_q32=0)
    with pytest.raises(DcmError, match="not both"):
        env.rollout("nearest", explore=0.1, explore_q32=5)
    with pytest.raises(DcmError, match=r"\[0, 1\]"):
        env.rollout("nearest", explore=1.5)
    with pytest.raises(DcmError, match=r"\[0, 2\^32\]"):
        env.rollout("first", explore_q32=(1 << 32) + 1)


def test_plan_sends_explore_launches_where_it_sends_greedy_ones(tmp_path):
    cxx = shutil.which("c++") or shutil.which("g++") or "/opt/rocm/llvm/bin/clang++"
    if not os.path.exists(cxx):
        pytest.skip("no host C++ compiler")
    shim = tmp_path / "plan_shim.cpp"
    shim.write_text('#include "%s"\n' % os.path.join(ROOT, "dcmrta_amd", "csrc", "plan.hpp") + """
using namespace dcm::plan;
static Shape shape(int A, int T, int ragged, int wide, int quiet) { return Shape{A, T, ragged != 0, wide != 0, quiet != 0}; }
extern "C" {
int p_explore(int A, int T, int ragged, int wide, int quiet, int obs) { return (int)form_rollout_kind(shape(A, T, ragged, wide, quiet), obs != 0); }
int p_policy(int A, int T, int ragged, int wide, int quiet, int obs) { return (int)form_rollout_kind(shape(A, T, ragged, wide, quiet), obs != 0); }
int p_form_ok(int form) { return form_ok((RenewForm)form) ? 1 : 0; }
}
""")
    so = tmp_path / "plan_shim.so"
    out = subprocess.run([cxx, "-std=c++17", "-O1", "-shared", "-fPIC", str(shim), "-o", str(so)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    P = C.CDLL(str(so))
    FAST, GENERAL = 0, 3                                                        # enum plan::Rollout
    assert P.p_explore(20, 50, 0, 0, 1, 1) == FAST and P.p_explore(15, 35, 1, 0, 1, 1) == FAST and P.p_explore(30, 60, 0, 0, 1, 1) == FAST
    assert P.p_explore(10, 64, 0, 0, 1, 1) == GENERAL                           # no free depot lane
    assert P.p_explore(66, 70, 0, 0, 1, 1) == GENERAL                           # the mid-size class
    assert P.p_explore(20, 50, 0, 0, 0, 1) == GENERAL                           # max_waiting_time <= 0
    # the shape list of the sibling host tests
    for A, T in [(20, 50), (12, 23), (64, 63), (64, 64), (50, 200), (70, 130), (100, 500), (128, 256), (100, 300)]:
        for bits in range(16):
            a = (A, T, bits & 1, (bits >> 1) & 1, (bits >> 2) & 1, (bits >> 3) & 1)
            assert P.p_explore(*a) == P.p_policy(*a) and P.p_explore(*a) in (FAST, GENERAL), a
    assert [P.p_form_ok(f) for f in (0, 1, 2)] == [1, 1, 0]                     # plan::RenewForm Plain, Instance, Sizes


def test_explore_kernel_forms_keep_four_waves_and_their_twins_occupancy(tmp_path):
    """The one-chunk epsilon-greedy forms of both kernels stay within the 128 VGPRs / four waves per SIMD of their greedy twins, and every
    renewing form (k_exrn_*) keeps the waves per SIMD of its plain twin (k_ex_*).  On the compiler's own resource report for the forms'
    translation unit, with the flags the Makefile gives it."""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    src = os.path.join(ROOT, "dcmrta_amd", "csrc", "dcmrta_env.hip")
    out = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-S", "--cuda-device-only", src,
                          "-Rpass-analysis=kernel-resource-usage", "-mllvm", "-amdgpu-sched-strategy=max-ilp", "-mllvm",
                          "-phi-elim-split-all-critical-edges=1", "-DDCM_TU_E", "-o", str(tmp_path / "env_e.s")], capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stderr[-2000:]
    usage = {}
    for m in re.finditer(r"Function Name: \S*?\d+(k_[a-z_]+?)(I(?:L[ib]\d+E)+E)Ev.*?VGPRs: (\d+).*?Occupancy \[waves/SIMD\]: (\d+)", out.stderr, re.S):
        usage[(m.group(1), m.group(2))] = (int(m.group(3)), int(m.group(4)))
    # the unit holds the four epsilon-greedy forms and nothing else that is a template
    assert {n for n, _ in usage} == {"k_ex_rollout_fast", "k_exrn_rollout_fast", "k_ex_rollout_random", "k_exrn_rollout_random"}, sorted(usage)
    seen = {}
    for (name, targs), (vgprs, occ) in usage.items():
        seen[name] = seen.get(name, 0) + 1
        if any(targs.startswith(t) for t in ("ILi20ELi50ELb0E", "ILi20ELi50ELb1E", "ILi64ELi64ELb1E")):
            assert vgprs <= 128 and occ >= 4, (name, targs, vgprs, occ)
        if name.startswith("k_exrn_"):
            twin = usage[("k_ex_" + name[len("k_exrn_"):], targs)]
            assert occ >= twin[1], (name, targs, vgprs, occ, twin)
        if name.endswith("rollout_fast"):
            assert targs.endswith("Lb0EE"), (name, targs)                      # no wave-priority (PRIO) instantiation
    # three one-chunk layouts x with / without observation stores; the eight Sim<> instantiations: the greedy unit's counts
    assert seen == {"k_ex_rollout_fast": 6, "k_exrn_rollout_fast": 6, "k_ex_rollout_random": 8, "k_exrn_rollout_random": 8}, seen
