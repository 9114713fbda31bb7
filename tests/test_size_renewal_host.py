"""Size renewal (DCM_PARAM_RENEW_SIZES), host side: the flag in the header and in the ctypes layer, the dispatch rule of csrc/plan.hpp
compiled with the host compiler, and the register budget of the size-renewing kernel forms (k_rs_*) on the compiler's report.  No GPU."""
import ctypes as C
import itertools
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_flag_is_declared_in_the_header_and_the_ctypes_layer():
    import inspect
    from dcmrta_amd import _lib
    from dcmrta_amd.batched_env import BatchedTaskEnv
    header = open(_lib.HEADER_PATH).read()
    m = re.search(r"#define\s+DCM_PARAM_RENEW_SIZES\s+(\d+)u\b", header)
    assert m and int(m.group(1)) == 16 == _lib.PARAM_RENEW_SIZES
    # a bit of its own among the DCM_PARAM_* flags, and the ABI version is unchanged (additions only)
    bits = [int(v) for v in re.findall(r"#define\s+DCM_PARAM_[A-Z_]+\s+(\d+)u\b", header)]
    assert len(bits) == len(set(bits)) and all(b & (b - 1) == 0 for b in bits)
    assert re.search(r"#define\s+DCM_ABI_VERSION\s+5\b", header) and _lib.ABI_VERSION == 5
    # described where a maintainer binds the call, and next to the snapshot size it changes
    doc = header[header.index("A fresh instance at every episode restart"):header.index("int dcm_set_instance_renewal")]
    assert "ragged" in doc.lower() and "DCM_PARAM_RENEW_SIZES" in doc
    assert "DCM_PARAM_RENEW_SIZES" in header[header.index("copy.deepcopy(env)"):header.index("int dcm_state_bytes")]
    # the keyword is the last one of BatchedTaskEnv and off by default
    params = list(inspect.signature(BatchedTaskEnv.__init__).parameters.values())
    assert params[-1].name == "renew_sizes" and params[-1].default is False


def test_plan_accepts_size_renewal_only_on_an_opted_in_generated_ragged_batch(tmp_path):
    cxx = shutil.which("c++") or shutil.which("g++") or "/opt/rocm/llvm/bin/clang++"
    if not os.path.exists(cxx):
        pytest.skip("no host C++ compiler")
    shim = tmp_path / "plan_shim.cpp"
    shim.write_text('#include "%s"\n' % os.path.join(ROOT, "dcmrta_amd", "csrc", "plan.hpp") + """
using namespace dcm::plan;
static Shape shape(int A, int T, int ragged, int wide, int quiet) { return Shape{A, T, ragged != 0, wide != 0, quiet != 0}; }
extern "C" {
int p_renewal(int A, int T, int ragged, int wide, int quiet, int generated) { return renewal_ok(shape(A, T, ragged, wide, quiet), generated != 0) ? 1 : 0; }
int p_renewal_sizes(int A, int T, int ragged, int wide, int quiet, int generated, int opted_in) {
    return renewal_sizes_ok(shape(A, T, ragged, wide, quiet), generated != 0, opted_in != 0) ? 1 : 0;
}
int p_form(int A, int T, int ragged, int wide, int quiet, int stride_set, int opted_in) {
    return (int)renew_form(shape(A, T, ragged, wide, quiet), stride_set != 0, opted_in != 0);
}
int p_defer(int captured, int form) { return defer_terminal(captured != 0, (RenewForm)form) ? 1 : 0; }
int p_image(int valid, int deferred, int renewal) { return step_restart_image(valid != 0, deferred != 0, renewal != 0) ? 1 : 0; }
int p_rollout(int A, int T, int ragged, int wide, int quiet, int obs) { return (int)rollout_kind(shape(A, T, ragged, wide, quiet), obs != 0); }
int p_sim(int A, int T, int ragged, int wide, int quiet) { return (int)sim_kind(shape(A, T, ragged, wide, quiet)); }
}
""")
    so = tmp_path / "plan_shim.so"
    out = subprocess.run([cxx, "-std=c++17", "-O1", "-shared", "-fPIC", str(shim), "-o", str(so)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    P = C.CDLL(str(so))
    PLAIN, INSTANCE, SIZES = 0, 1, 2                                           # enum plan::RenewForm
    FAST_MC = 1                                                                 # enum plan::Rollout
    EXACT = (0, 3, 4)                                                           # enum plan::SimKind: <20,50,false>, <50,200,false>, <100,500,false>
    shapes = [(20, 50), (12, 23), (64, 63), (64, 64), (50, 200), (70, 130), (100, 500), (128, 256), (100, 300)]
    for (A, T), ragged, wide, quiet in itertools.product(shapes, (0, 1), (0, 1), (0, 1)):
        for generated, opted_in in itertools.product((0, 1), (0, 1)):
            # renewal_ok is what it was: a generated uniform batch, whatever the flag says
            assert P.p_renewal(A, T, ragged, wide, quiet, generated) == int(generated and not ragged)
            # the new rule: generated AND opted in AND ragged, nothing else
            assert P.p_renewal_sizes(A, T, ragged, wide, quiet, generated, opted_in) == int(generated and opted_in and ragged)
            # never both: a batch is renewed one way or the other
            assert not (P.p_renewal(A, T, ragged, wide, quiet, generated) and P.p_renewal_sizes(A, T, ragged, wide, quiet, generated, opted_in))
        for stride_set, opted_in in itertools.product((0, 1), (0, 1)):
            form = P.p_form(A, T, ragged, wide, quiet, stride_set, opted_in)
            assert form == (PLAIN if not stride_set else SIZES if (ragged and opted_in) else INSTANCE)
            if form == SIZES:
                # the size-renewing forms exist for the runtime-size instantiations only: a ragged batch never runs an exact one
                assert P.p_sim(A, T, ragged, wide, quiet) not in EXACT
                assert all(P.p_rollout(A, T, ragged, wide, quiet, obs) != FAST_MC for obs in (0, 1))
    # a size-renewing launch defers no terminal metrics and gets no restart image; the other forms are as before
    for captured, form in itertools.product((0, 1), (PLAIN, INSTANCE, SIZES)):
        assert P.p_defer(captured, form) == int(not captured and form != SIZES)
    for valid, deferred, renewal in itertools.product((0, 1), repeat=3):
        assert P.p_image(valid, deferred, renewal) == int(valid and deferred and not renewal)


def test_size_renewing_kernels_keep_their_twins_waves_per_simd(tmp_path):
    """The size-renewing forms (k_rs_*) run in place of their plain twins on the same ragged batches: none may lose a wave per SIMD
    against its twin k_* of the same template arguments, and the one-chunk forms of k_rollout_fast, k_rollout_random and k_step_fast stay
    within the 128 VGPRs / four waves per SIMD that a 4096-env launch needs.  On the compiler's own resource report, for the two units
    of dcmrta_env.hip with the flags the Makefile gives them.  (The k_rn_* forms are tests/test_instance_renewal_host.py's.)"""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    src = os.path.join(ROOT, "dcmrta_amd", "csrc", "dcmrta_env.hip")
    base = [hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-S", "--cuda-device-only", src,
            "-Rpass-analysis=kernel-resource-usage", "-mllvm", "-amdgpu-sched-strategy=max-ilp"]
    units = {"env": ["-mllvm", "-phi-elim-split-all-critical-edges=1", "-DDCM_SPLIT_G"], "env_g": ["-DDCM_TU_G"]}
    procs = {u: subprocess.Popen(base + extra + ["-o", str(tmp_path / f"{u}.s")], stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, text=True)
             for u, extra in units.items()}
    usage = {}
    for u, p in procs.items():
        _, err = p.communicate(timeout=900)
        assert p.returncode == 0, err[-2000:]
        for m in re.finditer(r"Function Name: \S*?\d+(k_[a-z_]+?)(I(?:L[ib]\d+E)+E)Ev.*?VGPRs: (\d+).*?Occupancy \[waves/SIMD\]: (\d+)", err, re.S):
            usage[(m.group(1), m.group(2))] = (int(m.group(3)), int(m.group(4)))
    seen = {}
    for (name, targs), (vgprs, occ) in usage.items():
        if not name.startswith("k_rs_"):
            continue
        twin = usage[("k_" + name[len("k_rs_"):], targs)]
        assert occ >= twin[1], (name, targs, vgprs, occ, twin)
        seen.setdefault(name, set()).add(targs)
        # only what reads per-env sizes: no exact-shape instantiation (<CA, CT, false> with CA != 0)
        assert name == "k_rs_rollout_fast_g" or targs.startswith("ILi0ELi0ELb0E") or re.match(r"ILi\d+ELi\d+ELb1E", targs), (name, targs)
        one_chunk = any(targs.startswith(t) for t in ("ILi20ELi50ELb1E", "ILi64ELi64ELb1E"))
        if name in ("k_rs_rollout_random", "k_rs_rollout_fast", "k_rs_step_fast") and one_chunk:
            assert vgprs <= 128 and occ >= 4, (name, targs, vgprs, occ)
        if name == "k_rs_rollout_fast_g":
            assert occ >= 2, (name, targs, vgprs, occ)
    # every size-renewing form was seen, with the instantiations that can serve a ragged batch: <20,50,true>, <64,64,true>,
    # <128,256,true>, <0,0,false,5>, <0,0,false,16>; the one-chunk two (x OBS x PRIO for the rollout); every (NAC, NTC, OBS)
    assert {k: len(v) for k, v in seen.items()} == {"k_rs_step": 5, "k_rs_rollout_random": 5, "k_rs_step_fast": 2, "k_rs_rollout_fast": 8,
                                                    "k_rs_rollout_fast_g": 12}, seen
