"""Host, no GPU: the episode-boundary code of k_rollout_fast (which terminal an ending episode takes, how the next one starts) sits
outside the decision loop and must cost that loop nothing -- the kernel is bound by the length of one wave's instruction stream, and
the register allocation of the loop answers to every edge that enters it.  Read from the compiler's output, compiled the way
tools/loop_insts.py compiles it (the product's flags, one explicit instantiation): per plain one-chunk form the VGPRs, the scratch,
the waves per SIMD and the size of the decision loop against the figures of the parent commit (DESIGN.md 6 has the headline form's:
1122 instructions / 542 VALU / 108 VGPRs; the others were taken from the parent with the same tool)."""
import os
import re
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# (kernel, template arguments <CA, CT, ragged, OBS, PRIO>, --extra-args, unit macro): (VGPRs, scratch bytes per lane, loop instructions,
# loop VALU) of the parent.  Forms WITH the rule: plain, renewing, logging, renewing-logging at compile-time sizes; the runtime-size,
# greedy, epsilon-greedy (and best-keeping) forms keep terminal() and must compile to the parent's figures all the same.
H = "20, 50, false, true, false"
PARENT = {("k_rollout_fast", H, "", ""): (108, 0, 1122, 542),      # the sub-batch form of the headline's launches
          ("k_rollout_fast", "20, 50, false, true, true", "", ""): (108, 0, 1164, 544),       # one launch that fills the machine
          ("k_rollout_fast", "20, 50, false, false, false", "", ""): (101, 0, 1064, 508),     # no observation buffers
          ("k_rollout_fast", "20, 50, true, true, false", "", ""): (114, 8, 1132, 545),       # a ragged batch
          ("k_rollout_fast", "20, 50, true, true, true", "", ""): (114, 8, 1179, 554),
          ("k_rollout_fast", "64, 64, true, true, false", "", ""): (116, 0, 1152, 564),       # the runtime-size layout
          ("k_rn_rollout_fast", H, "Renew", ""): (116, 96, 1128, 542),
          ("k_rn_rollout_fast", "20, 50, false, true, true", "Renew", ""): (116, 96, 1170, 544),
          ("k_rn_rollout_fast", "20, 50, false, false, false", "Renew", ""): (110, 96, 1070, 508),
          ("k_lg_rollout_fast", H, "int, RouteLog", "-DDCM_TU_L"): (111, 0, 1229, 597),
          ("k_lg_rollout_fast", "20, 50, false, true, true", "int, RouteLog", "-DDCM_TU_L"): (107, 0, 1258, 597),
          ("k_lg_rollout_fast", "20, 50, false, false, false", "int, RouteLog", "-DDCM_TU_L"): (104, 0, 1164, 563),
          ("k_lgrn_rollout_fast", H, "Renew, int, RouteLog", "-DDCM_TU_L"): (118, 96, 1228, 597),
          ("k_hp_rollout_fast", H, "int", "-DDCM_TU_P"): (107, 0, 1175, 587),
          ("k_hprn_rollout_fast", H, "Renew, int", "-DDCM_TU_P"): (116, 96, 1181, 587),
          ("k_ex_rollout_fast", H, "int, uint64_t, RouteLog", "-DDCM_TU_E"): (111, 0, 1257, 621),
          ("k_exrn_rollout_fast", H, "Renew, int, uint64_t, RouteLog", "-DDCM_TU_E"): (121, 96, 1256, 621)}


@pytest.mark.parametrize("form", list(PARENT), ids=lambda f: f"{f[0]}<{f[1]}>")
def test_boundary_code_costs_the_decision_loop_nothing(form):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    kernel, targs, extra, unit = form
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "loop_insts.py"), "--kernel", f"{kernel}<{targs}>"] +
                         (["--extra-args", extra] if extra else []) + ([unit] if unit else []), capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    report = out.stdout
    m = re.search(r"VGPRs: (\d+).*ScratchSize \[bytes/lane\]: (\d+).*Occupancy \[waves/SIMD\]: (\d+)", report)
    n = re.search(r"decision loop \S+ of .*: (\d+) instructions, (\d+) VALU", report)
    assert m and n, report
    vgprs, scratch, occ = (int(x) for x in m.groups())
    insts, valu = (int(x) for x in n.groups())
    print(form, "VGPRs", vgprs, "scratch", scratch, "waves", occ, "loop", insts, "/", valu, "parent", PARENT[form])
    p_vgprs, p_scratch, p_insts, p_valu = PARENT[form]
    assert occ == 4 and vgprs <= 128 and vgprs <= p_vgprs, report
    assert scratch <= p_scratch, report
    assert insts <= p_insts and valu <= p_valu, report
