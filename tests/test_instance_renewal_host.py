"""Instance renewal, host side: the seed arithmetic of instances.renewal_seeds and the declaration of the two entry points
(dcm_set_instance_renewal, dcm_instance_index) in the header and in the ctypes table; the register budget of the renewing kernels on
the compiler's report.  No GPU."""
import re

import numpy as np

M64 = 1 << 64


def test_renewal_seeds_is_python_int_arithmetic_mod_2_64():
    from dcmrta_amd.instances import renewal_seeds
    seeds = [0, 1, 4242, (1 << 63) - 1, 1 << 63, M64 - 2, M64 - 1]
    strides = [1, 4096, (1 << 63) - 25, (1 << 63) + 12345, M64 - 1]
    for stride in strides:
        for n in (0, 1, 2, 3, 1000, (1 << 32) - 1):
            got = renewal_seeds(np.array(seeds, dtype=np.uint64), n, stride)
            assert got.dtype == np.uint64 and got.shape == (len(seeds),)
            assert [int(x) for x in got] == [(s + n * stride) % M64 for s in seeds], (stride, n)
    # the wrap is really exercised, and n = 0 is the identity
    assert int(renewal_seeds(M64 - 1, 1, 1)) == 0
    assert int(renewal_seeds(1 << 63, 2, (1 << 63) + 12345)) == ((1 << 63) + 2 * 12345) % M64
    assert np.array_equal(renewal_seeds(np.array(seeds, dtype=np.uint64), 0, 12345), np.array(seeds, dtype=np.uint64))


def test_renewal_seeds_broadcasts():
    from dcmrta_amd.instances import renewal_seeds
    B = 5
    base = np.uint64(M64 - 3) + np.arange(B, dtype=np.uint64)             # wraps inside the batch already
    got = renewal_seeds(base[None, :], np.arange(4)[:, None], B)           # [episode, env]
    assert got.shape == (4, B) and got.dtype == np.uint64
    for k in range(4):
        for e in range(B):
            assert int(got[k, e]) == (M64 - 3 + e + k * B) % M64
    assert int(renewal_seeds(7, 0, 5)) == 7


def test_both_symbols_are_declared_in_the_header_and_the_ctypes_table():
    import ctypes as C
    from dcmrta_amd import _lib
    header = open(_lib.HEADER_PATH).read()
    assert re.search(r"\bint\s+dcm_set_instance_renewal\s*\(\s*dcm_env\s*\*\s*env\s*,\s*uint64_t\s+stride\s*\)\s*;", header)
    assert re.search(r"\bint\s+dcm_instance_index\s*\(\s*dcm_env\s*\*\s*env\s*,\s*uint32_t\s*\*\s*index_out[^)]*,\s*void\s*\*\s*stream\s*\)\s*;", header)
    assert re.search(r"#define\s+DCM_ABI_VERSION\s+5\b", header) and _lib.ABI_VERSION == 5            # additions only
    res, args = _lib.SIGNATURES["dcm_set_instance_renewal"]
    assert res is C.c_int and args == [C.c_void_p, C.c_uint64]
    res, args = _lib.SIGNATURES["dcm_instance_index"]
    assert res is C.c_int and args == [C.c_void_p] * 3
    # the ragged-batch rule is stated where a maintainer binds the call
    assert "ragged" in header[header.index("A fresh instance at every episode restart"):header.index("int dcm_set_instance_renewal")].lower()


def test_renewing_kernels_keep_their_twins_waves_per_simd(tmp_path):
    """The renewing forms (k_rn_*) run in place of their plain twins while a stride is set, on the same batches: none may lose a wave
    per SIMD against its twin, and the one-chunk persistent forms stay within the 128 VGPRs / four waves per SIMD that a 4096-env
    launch needs (config 4's within 168 / three), as test_host holds the plain forms to.  Checked on the compiler's own resource
    report, for the two units of dcmrta_env.hip with the flags the Makefile gives them."""
    import os
    import shutil
    import subprocess
    import pytest
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = os.path.join(root, "dcmrta_amd", "csrc", "dcmrta_env.hip")
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
        if not name.startswith("k_rn_"):
            continue
        twin = usage[("k_" + name[len("k_rn_"):], targs)]
        assert occ >= twin[1], (name, targs, vgprs, occ, twin)
        seen[name] = seen.get(name, 0) + 1
        one_chunk = any(targs.startswith(t) for t in ("ILi20ELi50ELb0E", "ILi20ELi50ELb1E", "ILi64ELi64ELb1E"))
        if name in ("k_rn_rollout_random", "k_rn_rollout_fast", "k_rn_step_fast") and one_chunk:
            assert vgprs <= 128 and occ >= 4, (name, targs, vgprs, occ)
        if name == "k_rn_rollout_fast_mc":
            assert vgprs <= 168 and occ >= 3, (name, targs, vgprs, occ)
        if name == "k_rn_rollout_fast_g":
            assert occ >= 2, (name, targs, vgprs, occ)
    # every renewing form was seen, with as many instantiations as its twin has
    assert seen == {"k_rn_step": 8, "k_rn_step_fast": 3, "k_rn_rollout_random": 8, "k_rn_rollout_fast": 12, "k_rn_rollout_fast_mc": 2,
                    "k_rn_rollout_fast_g": 12}, seen
