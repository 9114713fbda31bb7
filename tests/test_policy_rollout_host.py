"""The greedy device policies (dcm_rollout_policy), host side: the symbol and its constants, the dispatch rule of csrc/plan.hpp compiled
with the host compiler, and the register budget of the greedy kernel forms (k_hp_*, k_hprn_*) on the compiler's report.  No GPU."""
import ctypes as C
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_library_exports_dcm_rollout_policy():
    from dcmrta_amd import _lib
    from dcmrta_amd.batched_env import BatchedTaskEnv
    assert hasattr(C.CDLL(_lib.LIB_PATH), "dcm_rollout_policy")
    header = open(_lib.HEADER_PATH).read()
    got = {k: int(v) for k, v in re.findall(r"#define\s+DCM_POLICY_([A-Z]+)\s+(\d+)\b", header)}
    assert got == {"RANDOM": 0, "FIRST": 1, "NEAREST": 2} == {"RANDOM": _lib.POLICY_RANDOM, "FIRST": _lib.POLICY_FIRST, "NEAREST": _lib.POLICY_NEAREST}
    assert re.search(r"#define\s+DCM_ABI_VERSION\s+5\b", header) and _lib.ABI_VERSION == 5          # additions only
    # dcm_rollout_random's arguments behind (env, policy)
    res, args = _lib.SIGNATURES["dcm_rollout_policy"]
    res0, args0 = _lib.SIGNATURES["dcm_rollout_random"]
    assert res == res0 and args == [args0[0], C.c_int32] + args0[1:]
    assert BatchedTaskEnv.POLICIES == {"random": 0, "first": 1, "nearest": 2}


def test_plan_sends_greedy_launches_to_the_fast_or_the_general_form(tmp_path):
    cxx = shutil.which("c++") or shutil.which("g++") or "/opt/rocm/llvm/bin/clang++"
    if not os.path.exists(cxx):
        pytest.skip("no host C++ compiler")
    shim = tmp_path / "plan_shim.cpp"
    shim.write_text('#include "%s"\n' % os.path.join(ROOT, "dcmrta_amd", "csrc", "plan.hpp") + """
using namespace dcm::plan;
static Shape shape(int A, int T, int ragged, int wide, int quiet) { return Shape{A, T, ragged != 0, wide != 0, quiet != 0}; }
extern "C" {
int p_policy(int A, int T, int ragged, int wide, int quiet, int obs) { return (int)form_rollout_kind(shape(A, T, ragged, wide, quiet), obs != 0); }
int p_rollout(int A, int T, int ragged, int wide, int quiet, int obs) { return (int)rollout_kind(shape(A, T, ragged, wide, quiet), obs != 0); }
int p_form_ok(int form) { return form_ok((RenewForm)form) ? 1 : 0; }
int p_needs_budget(int A, int T, int ragged, int wide, int quiet) { return policy_needs_budget(shape(A, T, ragged, wide, quiet)) ? 1 : 0; }
}
""")
    so = tmp_path / "plan_shim.so"
    out = subprocess.run([cxx, "-std=c++17", "-O1", "-shared", "-fPIC", str(shim), "-o", str(so)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    P = C.CDLL(str(so))
    FAST, FAST_MC, FAST_G, GENERAL = 0, 1, 2, 3                                 # enum plan::Rollout
    # (A, T, ragged, wide, quiet, obs all-or-none)
    assert P.p_policy(20, 50, 0, 0, 1, 1) == FAST
    assert P.p_policy(15, 35, 1, 0, 1, 1) == FAST
    assert P.p_policy(64, 63, 0, 0, 1, 1) == FAST
    assert P.p_policy(50, 200, 0, 0, 1, 1) == GENERAL and P.p_rollout(50, 200, 0, 0, 1, 1) == FAST_MC
    assert P.p_policy(70, 130, 0, 0, 1, 1) == GENERAL and P.p_rollout(70, 130, 0, 0, 1, 1) == FAST_G
    assert P.p_policy(64, 64, 0, 0, 1, 1) == GENERAL                            # no free depot lane
    assert P.p_policy(10, 20, 0, 1, 1, 1) == GENERAL                            # a wide handle
    assert P.p_policy(20, 50, 0, 0, 0, 1) == GENERAL                            # max_waiting_time <= 0
    assert P.p_policy(20, 50, 0, 0, 1, 0) == GENERAL                            # a partial observation buffer set
    # everywhere: the fast form exactly where the random policy takes it, the general one otherwise -- never FastMc / FastG
    for A, T in [(20, 50), (12, 23), (64, 63), (64, 64), (50, 200), (70, 130), (100, 500), (128, 256), (100, 300)]:
        for bits in range(16):
            a = (A, T, bits & 1, (bits >> 1) & 1, (bits >> 2) & 1, (bits >> 3) & 1)
            assert P.p_policy(*a) == (FAST if P.p_rollout(*a) == FAST else GENERAL), a
            assert P.p_needs_budget(*a[:5]) == int(not a[4])
    assert [P.p_form_ok(f) for f in (0, 1, 2)] == [1, 1, 0]                     # plan::RenewForm Plain, Instance, Sizes


def test_greedy_kernel_forms_keep_four_waves_and_their_twins_occupancy(tmp_path):
    """The one-chunk greedy forms of both kernels stay within the 128 VGPRs / four waves per SIMD that test_host holds their twins to, and
    every greedy renewing form (k_hprn_*) keeps the waves per SIMD of its plain greedy twin (k_hp_*).  On the compiler's own resource
    report for the greedy forms' translation unit, with the flags the Makefile gives it."""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    src = os.path.join(ROOT, "dcmrta_amd", "csrc", "dcmrta_env.hip")
    out = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-S", "--cuda-device-only", src,
                          "-Rpass-analysis=kernel-resource-usage", "-mllvm", "-amdgpu-sched-strategy=max-ilp", "-mllvm",
                          "-phi-elim-split-all-critical-edges=1", "-DDCM_TU_P", "-o", str(tmp_path / "env_p.s")], capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stderr[-2000:]
    usage = {}
    for m in re.finditer(r"Function Name: \S*?\d+(k_[a-z_]+?)(I(?:L[ib]\d+E)+E)Ev.*?VGPRs: (\d+).*?Occupancy \[waves/SIMD\]: (\d+)", out.stderr, re.S):
        usage[(m.group(1), m.group(2))] = (int(m.group(3)), int(m.group(4)))
    # the unit holds the greedy forms and nothing else that is a template
    assert {n for n, _ in usage} == {"k_hp_rollout_fast", "k_hprn_rollout_fast", "k_hp_rollout_random", "k_hprn_rollout_random"}, sorted(usage)
    seen = {}
    for (name, targs), (vgprs, occ) in usage.items():
        seen[name] = seen.get(name, 0) + 1
        if any(targs.startswith(t) for t in ("ILi20ELi50ELb0E", "ILi20ELi50ELb1E", "ILi64ELi64ELb1E")):
            assert vgprs <= 128 and occ >= 4, (name, targs, vgprs, occ)
        if name.startswith("k_hprn_"):
            twin = usage[("k_hp_" + name[len("k_hprn_"):], targs)]
            assert occ >= twin[1], (name, targs, vgprs, occ, twin)
        if name.endswith("rollout_fast"):
            assert targs.endswith("Lb0EE"), (name, targs)                      # no wave-priority (PRIO) instantiation
    # three one-chunk layouts x with / without observation stores; the eight Sim<> instantiations
    assert seen == {"k_hp_rollout_fast": 6, "k_hprn_rollout_fast": 6, "k_hp_rollout_random": 8, "k_hprn_rollout_random": 8}, seen
