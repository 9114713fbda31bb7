"""Host, no GPU: the decision loop of k_rollout_fast<20, 50> takes its one distance square root without range scaling (csrc/common.hpp,
dist2_inrange).  Read from the compiler's output, compiled the way tools/loop_insts.py compiles it (the product's flags, one explicit
instantiation of the plain form): exactly one v_rsq_f64 in the loop, and no v_ldexp_f64 -- the two scalings by 2^256 / 2^-128 that the
compiler's sqrt() wraps around the Newton steps for arguments below 2^-767, which no handle that runs this kernel can hold
(plan::Shape::inrange; tests/test_gpu_sqrt_inrange.py has the results)."""
import os
import re
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_one_rsq_and_no_ldexp_in_the_decision_loop(tmp_path):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    loop = tmp_path / "loop.s"
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "loop_insts.py"), "--dump", str(loop)],
                         capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    ops = [m.group(1) for m in (re.match(r"\s+([a-z_0-9]+)", l) for l in loop.read_text().splitlines()) if m]
    assert len(ops) > 900, len(ops)                                   # (the dump is the decision loop)
    assert sum(1 for o in ops if o.startswith("v_rsq_f64")) == 1, [o for o in ops if "rsq" in o]
    assert not [o for o in ops if o.startswith("v_ldexp_f64")]
    assert any(o.startswith("v_cmp_class_f64") for o in ops)          # the select that passes 0 and inf through stays
