"""The best log of the persistent launches (dcm_set_best_log), host side: the symbol and its signature, the Python checks that run before
anything touches the device, the dispatch rule of csrc/plan.hpp compiled with the host compiler, and the register budget of the
best-keeping kernel form (k_bs_*) on the compiler's report, next to its epsilon-greedy twins'.  No GPU."""
import ctypes as C
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_library_exports_dcm_set_best_log():
    from dcmrta_amd import _lib
    assert hasattr(C.CDLL(_lib.LIB_PATH), "dcm_set_best_log")
    header = open(_lib.HEADER_PATH).read()
    proto = re.search(r"int\s+dcm_set_best_log\s*\(\s*dcm_env\s*\*\s*env,\s*int16_t\s*\*\s*best_task,\s*double\s*\*\s*best_arrival,\s*"
                      r"int32_t\s*\*\s*best_len,\s*double\s*\*\s*best_summary,\s*int32_t\s*\*\s*best_episode\s*\)\s*;", header)
    assert proto
    res, args = _lib.SIGNATURES["dcm_set_best_log"]
    assert res is C.c_int and args == [C.c_void_p] * 6                           # the handle and the five pointers of the prototype
    abi = re.search(r"#define\s+DCM_ABI_VERSION\s+5\b(.*)", header)
    assert abi and _lib.ABI_VERSION == 5                                        # an addition only ...
    assert "still v5" in abi.group(1) and "dcm_set_best_log" in abi.group(1).split("still v5")[1]   # ... and listed as one


def test_the_python_checks_run_before_anything_touches_the_device():
    from dcmrta_amd.batched_env import BatchedTaskEnv
    from dcmrta_amd._lib import DcmError
    env = BatchedTaskEnv.__new__(BatchedTaskEnv)                                # a bare object: no handle, no library
    with pytest.raises(DcmError, match=r"enable_rollout_log\(cap\)"):
        env.enable_best_log()
    assert env.enable_best_log(False) is env                                    # off while off: nothing to do
    for read in (env.best_routes, env.best_summary, env.best_episode, env.best_plan, lambda: env.best_plan(0)):
        with pytest.raises(DcmError, match=r"best log is off: call enable_best_log\(\)"):
            read()
    from dcmrta_amd.trajectory import route_history
    with pytest.raises(DcmError, match="best log is off"):
        route_history(env, 0, log="best")
    with pytest.raises(ValueError, match='"step", "rollout" or "best"'):
        route_history(env, 0, log="last")


def test_plan_sends_best_launches_where_it_sends_the_other_forms(tmp_path):
    cxx = shutil.which("c++") or shutil.which("g++") or "/opt/rocm/llvm/bin/clang++"
    if not os.path.exists(cxx):
        pytest.skip("no host C++ compiler")
    shim = tmp_path / "plan_shim.cpp"
    shim.write_text('#include "%s"\n' % os.path.join(ROOT, "dcmrta_amd", "csrc", "plan.hpp") + """
using namespace dcm::plan;
static Shape shape(int A, int T, int ragged, int wide, int quiet) { return Shape{A, T, ragged != 0, wide != 0, quiet != 0}; }
extern "C" {
int p_best(int A, int T, int ragged, int wide, int quiet, int obs) { return (int)form_rollout_kind(shape(A, T, ragged, wide, quiet), obs != 0); }
int p_rollout(int A, int T, int ragged, int wide, int quiet, int obs) { return (int)rollout_kind(shape(A, T, ragged, wide, quiet), obs != 0); }
}
""")
    so = tmp_path / "plan_shim.so"
    out = subprocess.run([cxx, "-std=c++17", "-O1", "-shared", "-fPIC", str(shim), "-o", str(so)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    P = C.CDLL(str(so))
    FAST, GENERAL = 0, 3                                                        # enum plan::Rollout
    assert P.p_best(20, 50, 0, 0, 1, 1) == FAST and P.p_best(15, 35, 1, 0, 1, 1) == FAST and P.p_best(30, 60, 0, 0, 1, 1) == FAST
    assert P.p_best(50, 200, 0, 0, 1, 1) == GENERAL and P.p_best(70, 130, 0, 0, 1, 1) == GENERAL    # 50A/200T, the mid sizes
    assert P.p_best(10, 20, 0, 1, 1, 1) == GENERAL and P.p_best(20, 50, 0, 0, 0, 1) == GENERAL      # a wide handle, max_waiting_time <= 0
    assert P.p_best(20, 50, 0, 0, 1, 0) == GENERAL and P.p_best(10, 64, 0, 0, 1, 1) == GENERAL      # partial observation buffers, no depot lane
    # the shape list of the sibling host tests: the fast form exactly where rollout_kind says Fast, the general one everywhere else
    for A, T in [(20, 50), (12, 23), (64, 63), (64, 64), (50, 200), (70, 130), (100, 500), (128, 256), (100, 300)]:
        for bits in range(16):
            a = (A, T, bits & 1, (bits >> 1) & 1, (bits >> 2) & 1, (bits >> 3) & 1)
            assert P.p_best(*a) == (FAST if P.p_rollout(*a) == FAST else GENERAL), a
    # ... and the host asks that function for this form as for the others: one dispatch in rollout_form, one k_form.inc entry
    src = open(os.path.join(ROOT, "dcmrta_amd", "csrc", "dcmrta_env.hip")).read()
    tail = src[src.index("int rollout_form("):]
    tail = tail[:tail.index("\n}\n")]
    assert tail.count("plan::form_rollout_kind(") == 1 and "form.launch(" in tail
    assert re.search(r"FORM_BEST\{dcm::launch_rollout_best,", src)
    form = open(os.path.join(ROOT, "dcmrta_amd", "csrc", "k_form.inc")).read()
    assert re.search(r'#if defined\(DCM_BEST\) && DCM_RENEW != 0\s*\n#error', form) and "#define KPREFIX k_bs_" in form


def _usage(hipcc, unit, out_s):
    src = os.path.join(ROOT, "dcmrta_amd", "csrc", "dcmrta_env.hip")
    return subprocess.Popen([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-S", "--cuda-device-only",
                             src, "-Rpass-analysis=kernel-resource-usage", "-mllvm", "-amdgpu-sched-strategy=max-ilp", "-mllvm",
                             "-phi-elim-split-all-critical-edges=1", unit, "-o", str(out_s)], stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, text=True)


def test_best_kernel_form_keeps_four_waves_and_its_twins_occupancy(tmp_path):
    """The one-chunk instantiations of both k_bs_* kernels stay within 128 VGPRs / four waves per SIMD, and every k_bs_rollout_random
    keeps the waves per SIMD of its epsilon-greedy twin k_ex_rollout_random, whose decision loop it runs.  On the compiler's own
    resource reports for the two translation units (-DDCM_TU_B, -DDCM_TU_E), with the flags the Makefile gives them."""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    mk = open(os.path.join(ROOT, "dcmrta_amd", "csrc", "Makefile")).read()
    assert re.search(r"^UNITS := .*\benv_b\b", mk, re.M) and re.search(r"^FLAGS_env_b\s*=\s*\$\(SPLIT\) \$\(SCHED\) -DDCM_TU_B\s*$", mk, re.M)
    procs = {u: _usage(hipcc, "-DDCM_TU_" + u, tmp_path / f"env_{u.lower()}.s") for u in ("B", "E")}
    usage = {}
    for u, p in procs.items():
        _, err = p.communicate(timeout=900)
        assert p.returncode == 0, err[-2000:]
        usage[u] = {}
        for m in re.finditer(r"Function Name: \S*?\d+(k_[a-z_]+?)(I(?:L[ib]\d+E)+E)Ev.*?VGPRs: (\d+).*?Occupancy \[waves/SIMD\]: (\d+)", err, re.S):
            usage[u][(m.group(1), m.group(2))] = (int(m.group(3)), int(m.group(4)))
    best, twins = usage["B"], usage["E"]
    # the unit holds the two best-keeping kernels and nothing else that is a template: no renewing form
    assert {n for n, _ in best} == {"k_bs_rollout_fast", "k_bs_rollout_random"}, sorted(best)
    seen = {}
    for (name, targs), (vgprs, occ) in best.items():
        seen[name] = seen.get(name, 0) + 1
        if any(targs.startswith(t) for t in ("ILi20ELi50ELb0E", "ILi20ELi50ELb1E", "ILi64ELi64ELb1E")):
            assert vgprs <= 128 and occ >= 4, (name, targs, vgprs, occ)
        if name == "k_bs_rollout_random":
            twin = twins[("k_ex_rollout_random", targs)]
            assert occ >= twin[1], (name, targs, vgprs, occ, twin)
        if name.endswith("rollout_fast"):
            assert targs.endswith("Lb0EE"), (name, targs)                      # no wave-priority (PRIO) instantiation
    # three one-chunk layouts x with / without observation stores; the eight Sim<> instantiations: the sibling units' counts
    assert seen == {"k_bs_rollout_fast": 6, "k_bs_rollout_random": 8}, seen
