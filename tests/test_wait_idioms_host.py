"""Host, no GPU: three idioms on the dependent chain of the decision loop of k_rollout_fast (rollout_fast.hpp, common.hpp).

  * The abandonment log and its overflow counts were reached through pointers kept in the LDS image, whose address space the compiler
    cannot know: FLAT instructions, which count on lgkmcnt as well as vmcnt, so that the next lgkmcnt(0) -- every wait of this loop is
    one -- also waited for an HBM store to leave.  Cast to the global address space they are global_ instructions: the loop holds no
    flat_ instruction.
  * The target lane `action - 1` was fused with `action != 0` into one VALU subtract-with-borrow; every uniform use came back by
    v_readfirstlane with an s_nop in front of the v_readlane that uses it as lane select, and the borrow mask was materialised as a
    0/1 VGPR and compared back with 1 (the round trip of test_mask_idioms_host.py, spelled with a 1).  `action - 1` is pinned to the
    scalar unit now.
  * Behind every single-instruction asm v_min_f64 / v_max_f64 of task_update's slot minimum / maximum stood an s_nop (the compiler
    pads for a hazard of an asm statement it cannot read); nanmin5 / nanmax5 are one statement of four instructions each.
This test reads the compiler's output, compiled the way tools/loop_insts.py compiles it (the product's flags, one explicit
instantiation).

                                                   before (commit e42abfc)      now
    flat_ instructions in the loop                          4                    0
    `0, 1` + `ne 1` round-trip pairs                        1                    0
    v_readfirstlane -> s_nop -> v_readlane                  2                    0
    v_readfirstlane in the loop                             4                    1
    s_nop in the loop                                      38                   26
    instructions / VALU in the loop                    1134 / 550           1122 / 542
    VGPRs / waves per SIMD / scratch                   108 / 4 / 0          108 / 4 / 0
"""
import os
import re
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNEL = "k_rollout_fast<20, 50, false, true, false>"      # the sub-batch form of the headline's launches
BEFORE = dict(s_nop=38, readfirstlane=4, valu=550)
NOW = dict(s_nop=26, readfirstlane=1, valu=542)


def insts(lines):
    """the instructions of a dump (labels, directives and comments dropped, trailing comments cut)"""
    return [l.split(";")[0].strip() for l in lines if re.match(r"\s+[a-z]", l) and not l.startswith("\t.")]


def count(lines, prefix):
    return sum(1 for l in insts(lines) if l.startswith(prefix))


def one_pairs(lines):
    """`v_cndmask_b32 vN, 0, 1, <mask>` whose vN a `v_cmp_ne_u32 ..., 1, vN` reads within the next three instructions"""
    ins, n = insts(lines), 0
    for i, l in enumerate(ins):
        m = re.match(r"v_cndmask_b32(?:_e64|_e32)?\s+(v\d+), 0, 1, (?:s\[\d+:\d+\]|vcc)\s*$", l)
        if m and any(re.match(r"v_cmp_ne_u32(?:_e64|_e32)?\s+(?:(?:s\[\d+:\d+\]|vcc), )?1, " + m.group(1) + r"\s*$", x)
                     for x in ins[i + 1:i + 4]):
            n += 1
    return n


def readfirstlane_nop_readlane(lines):
    """an s_nop directly in front of a v_readlane, with a v_readfirstlane within the two instructions in front of the s_nop: a
    uniform value that sat in a VGPR, fetched and used as a lane select right away"""
    ins, n = insts(lines), 0
    for i, l in enumerate(ins):
        if l.startswith("s_nop") and i + 1 < len(ins) and ins[i + 1].startswith("v_readlane") and \
                any(x.startswith("v_readfirstlane") for x in ins[max(0, i - 2):i]):
            n += 1
    return n


def _compile(tmp, name, *defs):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    loop = tmp / (name + ".s")
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "loop_insts.py"), "--kernel", KERNEL, "--dump", str(loop), *defs],
                         capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    return loop.read_text().splitlines(), out.stdout


@pytest.fixture(scope="module")
def product(tmp_path_factory):
    return _compile(tmp_path_factory.mktemp("waits"), "loop")


def test_the_patterns_find_what_they_describe():
    """The counters on hand-written lines (so that a change of the compiler's spelling is not mistaken for zero)"""
    loop = ["\tv_cndmask_b32_e64 v12, 0, 1, s[0:1]", "\tv_readfirstlane_b32 s4, v19", "\tv_cmp_ne_u32_e64 s[2:3], 1, v12",
            "\tv_cndmask_b32_e64 v13, 0, 1, vcc", "\tv_cmp_ne_u32_e32 vcc, 0, v13",          # the other rule's spelling: not this one
            "\tv_cndmask_b32_e64 v14, 0, 1, vcc", "\tv_add_u32_e32 v1, v2, v3", "\tv_add_u32_e32 v1, v2, v3", "\tv_add_u32_e32 v1, v2, v3",
            "\tv_cmp_ne_u32_e32 vcc, 1, v14",                                                  # too far away
            "\tv_readfirstlane_b32 s6, v16", "\ts_nop 3", "\tv_readlane_b32 s6, v30, s6",
            "\tv_readfirstlane_b32 s6, v16", "\ts_mov_b32 s1, 0", "\ts_nop 2", "\tv_readlane_b32 s6, v30, s6 ; comment",
            "\tv_readfirstlane_b32 s6, v16", "\ts_mov_b32 s1, 0", "\ts_mov_b32 s1, 0", "\ts_nop 2", "\tv_readlane_b32 s6, v30, s6",   # too far
            "\ts_nop 1", "\tv_readlane_b32 s6, v30, s6",                                       # no v_readfirstlane
            "\tds_read_b64 v[0:1], v2", "\ts_waitcnt lgkmcnt(0)", "\tds_read_b32 v0, v2",
            "\tflat_store_short v[0:1], v6", "\tglobal_store_short v[0:1], v6, off", "\tflat_atomic_add v[12:13], v16",
            ".LBB10_3:", "\t.p2align 6"]
    assert one_pairs(loop) == 1
    assert readfirstlane_nop_readlane(loop) == 2
    assert count(loop, "flat_") == 2 and count(loop, "ds_") == 2 and count(loop, "s_waitcnt") == 1


def test_no_flat_instruction_in_the_loop(product):
    assert count(product[0], "flat_") == 0, [l for l in insts(product[0]) if l.startswith("flat_")]


def test_the_target_lane_stays_scalar(product):
    assert one_pairs(product[0]) == 0
    assert readfirstlane_nop_readlane(product[0]) == 0


def test_no_more_than_the_finished_build_and_the_resources_of_four_waves(product):
    lines, report = product
    m = re.search(r"decision loop \S+ of .*: \d+ instructions, (\d+) VALU", report)
    assert m, report
    got = dict(s_nop=count(lines, "s_nop"), readfirstlane=count(lines, "v_readfirstlane"), valu=int(m.group(1)))
    print("decision loop of", KERNEL, got)
    for k, v in got.items():
        assert v <= NOW[k], (k, got)
        assert v < BEFORE[k], (k, got)
    assert all("lgkmcnt(0)" in l and "vmcnt" not in l for l in insts(lines) if l.startswith("s_waitcnt")), "every wait is an lgkmcnt(0)"
    m = re.search(r"VGPRs: (\d+).*ScratchSize \[bytes/lane\]: (\d+).*Occupancy \[waves/SIMD\]: (\d+)", report)
    assert m, report
    assert int(m.group(1)) <= 128 and int(m.group(2)) == 0 and int(m.group(3)) == 4, report
