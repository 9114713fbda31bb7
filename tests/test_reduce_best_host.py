"""The cross-env reduction of the best log (dcm_reduce_best; BatchedTaskEnv.reduce_best), host side: the symbol and its signature, the
Python checks that run before anything touches the device, and the register budget of k_reduce_best on the compiler's report for the
main translation unit.  No GPU."""
import ctypes as C
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "dcmrta_amd", "csrc")


def test_library_exports_dcm_reduce_best():
    from dcmrta_amd import _lib
    assert hasattr(C.CDLL(_lib.LIB_PATH), "dcm_reduce_best")
    header = open(_lib.HEADER_PATH).read()
    p = r"\s*\*\s*"
    proto = re.search(r"int\s+dcm_reduce_best\s*\(\s*dcm_env" + p + r"env,\s*int32_t\s+group,\s*int32_t" + p + r"win_env,\s*double" + p
                      + r"win_summary,\s*int32_t" + p + r"win_episode,\s*int32_t" + p + r"win_len,\s*int16_t" + p + r"win_task,\s*double" + p
                      + r"win_arrival,\s*void" + p + r"stream\s*\)\s*;", header)
    assert proto
    res, args = _lib.SIGNATURES["dcm_reduce_best"]
    # the handle, the group size, the six output pointers and the stream of the prototype
    assert res is C.c_int and args == [C.c_void_p, C.c_int32] + [C.c_void_p] * 6 + [C.c_void_p]
    abi = re.search(r"#define\s+DCM_ABI_VERSION\s+5\b(.*)", header)
    assert abi and _lib.ABI_VERSION == 5                                        # an addition only ...
    assert "still v5" in abi.group(1) and "dcm_reduce_best" in abi.group(1).split("still v5")[1]   # ... and listed as one


def test_the_python_checks_run_before_anything_touches_the_device():
    from dcmrta_amd import batched_env
    from dcmrta_amd._lib import DcmError
    env = batched_env.BatchedTaskEnv.__new__(batched_env.BatchedTaskEnv)        # a bare object: no handle, no library
    for call in (env.reduce_best, lambda: env.reduce_best(group=3), lambda: env.reduce_best(routes=False)):
        with pytest.raises(DcmError, match=r"best log is off: call enable_best_log\(\)"):
            call()
    for group in (0, -5):
        with pytest.raises(ValueError, match="group must be >= 1"):
            env.reduce_best(group=group)
    assert callable(batched_env.group_plan) and callable(env.group_plan)


def test_group_plan_is_best_plans_lists_for_one_winner():
    """group_plan reads the reduced buffers alone: route_lists over one winner's rows, actions = task id + 1, and route_lists'
    ValueError where a kept route is longer than the log."""
    import numpy as np
    import torch
    from dcmrta_amd.batched_env import BatchedTaskEnv, group_plan
    task = np.full((2, 3, 4), -2, np.int16)
    task[1, 0, :3] = [4, -1, 0]
    task[1, 2, :4] = [1, 2, 3, -1]
    red = dict(task=torch.from_numpy(task), arrival=torch.zeros((2, 3, 4), dtype=torch.float64),
               len=torch.tensor([[0, 0, 0], [3, 0, 4]], dtype=torch.int32))
    assert group_plan(red, 0) == [[], [], []]
    assert group_plan(red, 1) == [[5, 0, 1], [], [2, 3, 4, 0]] == BatchedTaskEnv.group_plan(red, 1)
    red["len"][1, 2] = 7
    with pytest.raises(ValueError, match=r"route of agent 2 has 7 entries but the log holds 4; raise enable_rollout_log\(cap\)"):
        group_plan(red, 1)


def test_the_kernel_is_in_the_main_unit_alone_and_spills_nothing(tmp_path):
    """k_reduce_best on the compiler's resource report of the main translation unit, with the flags the Makefile gives it: no spilled
    VGPR, no scratch.  The header is not a template and is kept out of the form units."""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    hpp = open(os.path.join(CSRC, "best_reduce.hpp")).read()
    assert re.search(r"^__global__ [^\n]*\bvoid k_reduce_best\(", hpp, re.M) and not re.search(r"template[^\n]*\n__global__", hpp)
    src = open(os.path.join(CSRC, "dcmrta_env.hip")).read()
    assert re.search(r'#ifndef DCM_DEVICE_ONLY_TU[^\n]*\n#include "best_reduce.hpp"\n#endif', src)
    mk = open(os.path.join(CSRC, "Makefile")).read()
    assert re.search(r"^FLAGS_env\s*=\s*\$\(SPLIT\) \$\(SCHED\) -DDCM_SPLIT_G\s*$", mk, re.M)
    out = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-S", "--cuda-device-only",
                          os.path.join(CSRC, "dcmrta_env.hip"), "-Rpass-analysis=kernel-resource-usage", "-mllvm", "-phi-elim-split-all-critical-edges=1",
                          "-mllvm", "-amdgpu-sched-strategy=max-ilp", "-DDCM_SPLIT_G", "-o", str(tmp_path / "env.s")],
                         stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, text=True, timeout=1500)
    assert out.returncode == 0, out.stderr[-2000:]
    found = re.findall(r"Function Name: \S*?13k_reduce_best\S*.*?VGPRs: (\d+).*?ScratchSize \[bytes/lane\]: (\d+).*?Dynamic Stack: (\w+).*?"
                       r"VGPRs Spill: (\d+)", out.stderr, re.S)
    assert len(found) == 1, found
    vgprs, scratch, dynamic, spilled = found[0]
    assert int(spilled) == 0 and int(scratch) == 0 and dynamic == "False", found
    assert int(vgprs) <= 128, found                                             # a 1024-thread block is four waves on every SIMD: 512 / 4
