"""Host, no GPU: the register copies that were taken out of the decision loop of k_rollout_fast stay out.

The headline kernel is bound by the length of one wave's instruction stream, and two source idioms once put about 80 v_mov into
its decision loop: a tied `old` operand in the fp64 DPP helper of the wave reductions (2 v_mov_b32_e32 + an s_nop in front of every
stage), and an if / else-if at the bottom of the loop that made the compiler compute every event in shadow registers and copy them
back.  Both are source-level accidents that an innocent edit can bring back without any test of results noticing; this one reads
the compiler's output, compiled the way tools/loop_insts.py compiles it (the product's flags, one explicit instantiation)."""
import os
import re
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNEL = "k_rollout_fast<20, 50, false, true, false>"      # the sub-batch form of the headline's launches


@pytest.fixture(scope="module")
def census(tmp_path_factory):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    loop = tmp_path_factory.mktemp("census") / "loop.s"
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "loop_insts.py"), "--kernel", KERNEL, "--dump", str(loop)],
                         capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    return out.stdout, loop.read_text().splitlines()


def test_four_waves_per_simd_and_no_scratch(census):
    report, _ = census
    m = re.search(r"VGPRs: (\d+).*ScratchSize \[bytes/lane\]: (\d+).*Occupancy \[waves/SIMD\]: (\d+)", report)
    assert m, report
    vgprs, scratch, occ = (int(x) for x in m.groups())
    assert occ == 4 and vgprs <= 128, report
    assert scratch == 0, report


def test_no_copy_between_the_dpp_stages_of_a_reduction(census):
    """Every stage of a reduction is the two halves' v_mov_b32_dpp and the v_min / v_max_f64.  From one DPP move of a reduction to
    the next (one that does not start a reduction, i.e. anything but row_shr:1) no plain v_mov_b32 may touch a register of the
    reduction: the value's pair or the DPP moves' destinations, which is where the copy of a tied `old` operand lands.  (The
    scheduler does place moves of OTHER values into the s_nop slots between the stages -- `v_mov_b32_e32 v13, s46` -- which cost
    the chain nothing; those are counted by the bound on the loop's v_mov instead.)"""
    _, loop = census
    dpp = [i for i, l in enumerate(loop) if re.match(r"\s+v_mov_b32_dpp\b", l)]
    assert len(dpp) >= 2 * 5 * 3, len(dpp)            # next_event: three reductions of five stages (20 agents: rows 0 and 1)
    regs = lambda l: set(re.findall(r"\bv(\d+)\b", l))
    steps = 0
    for i, j in zip(dpp, dpp[1:]):
        if "row_shr:1 " in loop[j]:
            continue                                  # the next reduction starts here
        own = regs(loop[i]) | regs(loop[j])
        for l in loop[i + 1:j]:
            if re.match(r"\s+v_mov_b32_e32\b", l):
                assert not (regs(l) & own), "\n".join(loop[i:j + 1])
        steps += 1
    assert steps >= 3 * 2 * 4                         # two halves x the four stages behind row_shr:1, three reductions


def test_few_register_copies_in_the_decision_loop(census):
    """127 v_mov before the two idioms were removed, 47 after; the slack is for compiler drift."""
    report, loop = census
    movs = sum(1 for l in loop if re.match(r"\s+v_mov_", l))
    m = re.search(r"valu:mov (\d+)", report)
    assert m and int(m.group(1)) <= 60, report
    # (the tool's class "valu:mov" leaves out the DPP moves, which are the reductions themselves)
    assert movs - sum(1 for l in loop if re.match(r"\s+v_mov_b32_dpp\b", l)) <= 60
