"""The per-env copy between handles (dcm_fork_envs; BatchedTaskEnv.fork_from; dcmrta_amd.lookahead.Lookahead), host side: the symbol,
its prototype and ctypes signature, its place in the v5 additions list, where the kernel lives, and the argument errors of fork_from
and Lookahead that are raised before anything touches a device.  No GPU."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "dcmrta_amd", "csrc")


def test_header_declares_dcm_fork_envs_and_the_abi_is_still_5():
    from dcmrta_amd import _lib
    assert hasattr(C.CDLL(_lib.LIB_PATH), "dcm_fork_envs")
    header = open(_lib.HEADER_PATH).read()
    p = r"\s*\*\s*"
    proto = re.search(r"int\s+dcm_fork_envs\s*\(\s*dcm_env" + p + r"dst,\s*dcm_env" + p + r"src,\s*const\s+int32_t" + p + r"src_index,\s*"
                      r"const\s+uint64_t" + p + r"seeds_in,\s*uint8_t" + p + r"ok_out,\s*void" + p + r"stream\s*\)\s*;", header)
    assert proto
    abi = re.search(r"#define\s+DCM_ABI_VERSION\s+5\b(.*)", header)
    assert abi and _lib.ABI_VERSION == 5                                        # an addition only ...
    assert "still v5" in abi.group(1) and "dcm_fork_envs" in abi.group(1).split("still v5")[1]   # ... and listed as one
    # the comment in front of the prototype: the contract, the refusals, the bookkeeping and what is not copied
    comment = header[:proto.start()].rsplit("/*", 1)[1]
    for word in ("src_index", "-1", "seeds_in", "ok_out", "DCM_ERR_INVALID", "DCM_ERR_STATE", "ragged", "renewal stride", "stream capture",
                 "dcm_set_route_log", "dcm_set_rollout_log", "dcm_set_best_log", "dcm_set_return_log", "NOT copied", "restart image"):
        assert word in comment, word


def test_ctypes_signature():
    from dcmrta_amd import _lib
    res, args = _lib.SIGNATURES["dcm_fork_envs"]
    # dst, src, src_index, seeds_in, ok_out, stream: six pointers
    assert res is C.c_int and args == [C.c_void_p] * 6


def test_the_kernel_is_a_plain_copy_in_the_main_unit_alone():
    hpp = open(os.path.join(CSRC, "fork_envs.hpp")).read()
    assert re.search(r"^__global__ [^\n]*\bvoid k_fork_envs\(", hpp, re.M) and not re.search(r"template[^\n]*\n__global__", hpp)
    code = "\n".join(line.split("//")[0] for line in hpp.splitlines())
    for word in ("__shared__", "atomic", "nontemporal", "__syncthreads", "smem"):
        assert word not in code, word
    src = open(os.path.join(CSRC, "dcmrta_env.hip")).read()
    assert re.search(r'#ifndef DCM_DEVICE_ONLY_TU[^\n]*\n#include "fork_envs.hpp"\n#endif', src)
    assert src.count('"fork_envs.hpp"') == 1


def _bare(**kw):
    """a BatchedTaskEnv without a handle or a library: what the argument checks read, and nothing for close() to destroy"""
    from dcmrta_amd.batched_env import BatchedTaskEnv
    env = BatchedTaskEnv.__new__(BatchedTaskEnv)
    attrs = dict(_h=None, B=4, A=20, T=50, member_cap=5, device="cuda:0", max_waiting_time=10.0, max_time=100.0, auto_reset=False,
                 individual_selection=False, strict_mask=False, n_tasks=None, n_agents=None)
    attrs.update(kw)
    for k, v in attrs.items():
        setattr(env, k, v)
    return env


def test_fork_from_argument_errors_need_no_device():
    import torch
    from dcmrta_amd._lib import DcmError
    dst, idx = _bare(), np.zeros(4, np.int32)
    with pytest.raises(DcmError, match="src must be a BatchedTaskEnv"):
        dst.fork_from(object(), idx)
    for kw in (dict(A=21), dict(T=49), dict(member_cap=16)):
        with pytest.raises(DcmError, match="record layouts must be identical"):
            dst.fork_from(_bare(**kw), idx)
    for bad in (np.zeros(3, np.int32), np.zeros(5, np.int32), torch.zeros(7, dtype=torch.int32)):
        with pytest.raises(DcmError, match=r"index must be int32\[4\]"):
            dst.fork_from(_bare(B=9), bad)
    with pytest.raises(DcmError, match=r"seeds must be uint64\[4\]"):
        dst.fork_from(_bare(), idx, seeds=np.zeros(3, np.uint64))
    with pytest.raises(DcmError, match="uint64 / int64 tensor"):
        dst.fork_from(_bare(), idx, seeds=torch.zeros(4, dtype=torch.int32))
    with pytest.raises(DcmError, match="different devices"):
        dst.fork_from(_bare(device="cuda:1"), idx)
    with pytest.raises(DcmError, match="a handle is closed"):
        dst.fork_from(_bare(), idx, seeds=np.arange(4, dtype=np.uint64))


def test_lookahead_argument_errors_need_no_device():
    from dcmrta_amd._lib import DcmError
    from dcmrta_amd.lookahead import Lookahead
    with pytest.raises(DcmError, match="env must be a BatchedTaskEnv"):
        Lookahead(object())
    with pytest.raises(DcmError, match="policy must be one of"):
        Lookahead(_bare(), policy="farthest")
    for mwt in (0.0, -1.0, float("nan")):
        with pytest.raises(DcmError, match="max_waiting_time <= 0"):
            Lookahead(_bare(max_waiting_time=mwt))
    with pytest.raises(DcmError, match="auto_reset"):
        Lookahead(_bare(auto_reset=True))
    with pytest.raises(DcmError, match="ragged"):
        Lookahead(_bare(n_tasks=np.full(4, 50, np.int32)))


def test_best_actions_takes_the_largest_pair_and_the_lowest_index():
    import torch
    from dcmrta_amd.lookahead import Lookahead
    nan = float("nan")
    reward = torch.tensor([[nan, -30.0, -20.0, -20.0], [-50.0, -10.0, nan, -10.0], [nan, nan, nan, nan], [-5.0, -9.0, -9.0, nan]], dtype=torch.float64)
    finished = torch.tensor([[-1, 7, 7, 7], [9, 8, -1, 8], [-1, -1, -1, -1], [3, 4, 4, -1]], dtype=torch.int32)
    # more finished tasks first, then the larger reward, then the lowest index; nothing valid: 0
    assert Lookahead.best_actions(reward, finished).tolist() == [2, 0, 0, 1]
