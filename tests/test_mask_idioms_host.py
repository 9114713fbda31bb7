"""Host, no GPU: lane predicates of the decision loop of k_rollout_fast stay in scalar masks.

Two source idioms put VALU instructions of the expensive class into the loop without any result needing them (common.hpp, lane_of):
  * the ballot of a logical COMBINATION of predicates: the compiler holds the combination as an SGPR mask, materialises it as a 0/1
    VGPR and compares that back -- `v_cndmask_b32 vN, 0, 1, <mask>` + `v_cmp_ne_u32 <mask>, 0, vN`, a round trip of two VOP3;
  * the lane-bit test `(mask >> lane) & 1` of a wave-uniform mask: a 64-bit vector shift of an SGPR pair, an and and a compare -- or,
    which is what this compiler emits in this loop, two v_and_b32 of the mask's halves with a lane-bit register pair and a
    v_cmp_ne_u64 of the result with 0.  Both spellings are counted (the first alone counts 0 before and after).
The rule that removes them (a ballot takes one direct compare, combinations happen on the masks, a lane predicate comes from a mask by
the inverse ballot) is invisible to every test of results; this one reads the compiler's output, compiled the way
tools/loop_insts.py compiles it (the product's flags, one explicit instantiation).

                                          round-trip pairs   lane-bit tests of an SGPR pair   VALU in the loop
    before the rule (commit 3def572)             14                       3                        658
    with it                                       0                       0                        626
"""
import os
import re
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNEL = "k_rollout_fast<20, 50, false, true, false>"      # the sub-batch form of the headline's launches
BEFORE = dict(pairs=14, shifts=3, valu=658)
NOW = dict(pairs=0, shifts=0, valu=626)


def round_trip_pairs(loop):
    """`v_cndmask_b32 vN, 0, 1, <sgpr pair or vcc>` whose vN a `v_cmp_ne_u32 ..., 0, vN` reads within the next three instructions"""
    insts = [l.split(";")[0].strip() for l in loop if re.match(r"\s+[a-z]", l)]
    n = 0
    for i, l in enumerate(insts):
        m = re.match(r"v_cndmask_b32(?:_e64|_e32)?\s+(v\d+), 0, 1, (?:s\[\d+:\d+\]|vcc)\s*$", l)
        if m and any(re.match(r"v_cmp_ne_u32(?:_e64|_e32)?\s+(?:(?:s\[\d+:\d+\]|vcc), )?0, " + m.group(1) + r"\s*$", x)
                     for x in insts[i + 1:i + 4]):
            n += 1
    return n


def sgpr_pair_shifts(loop):
    """The lane-bit test of a wave-uniform mask: v_lshrrev_b64 of an SGPR pair by a VGPR, or v_cmp_ne_u64 0, v[a:b] right behind the
    two v_and_b32 that made v[a:b] from the halves of an SGPR pair"""
    insts = [l.split(";")[0].strip() for l in loop if re.match(r"\s+[a-z]", l)]
    n = sum(1 for l in insts if re.match(r"v_lshrrev_b64\s+v\[\d+:\d+\], v\d+, s\[\d+:\d+\]$", l))
    for i, l in enumerate(insts):
        m = re.match(r"v_cmp_ne_u64(?:_e64|_e32)?\s+(?:(?:s\[\d+:\d+\]|vcc), )?0, v\[(\d+):(\d+)\]$", l)
        if m:
            halves = {re.match(r"v_and_b32(?:_e64|_e32)?\s+v(\d+), s\d+, v\d+$", x) for x in insts[max(0, i - 4):i]}
            if {h.group(1) for h in halves if h} >= {m.group(1), m.group(2)}:
                n += 1
    return n


@pytest.fixture(scope="module")
def census(tmp_path_factory):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    loop = tmp_path_factory.mktemp("masks") / "loop.s"
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "loop_insts.py"), "--kernel", KERNEL, "--dump", str(loop)],
                         capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = loop.read_text().splitlines()
    m = re.search(r"decision loop \S+ of .*: \d+ instructions, (\d+) VALU", out.stdout)
    assert m, out.stdout
    got = dict(pairs=round_trip_pairs(lines), shifts=sgpr_pair_shifts(lines), valu=int(m.group(1)))
    print("decision loop of", KERNEL, got)
    return got


def test_the_patterns_find_what_they_describe():
    """The two counters on hand-written lines (so that a change of the compiler's spelling is not mistaken for zero)"""
    loop = ["\tv_cndmask_b32_e64 v5, 0, 1, s[10:11]", "\ts_and_b64 s[2:3], s[4:5], s[6:7]", "\tv_cmp_ne_u32_e64 s[12:13], 0, v5",
            "\tv_cndmask_b32_e64 v6, 0, 1, vcc", "\tv_cmp_ne_u32_e32 vcc, 0, v6",
            "\tv_cndmask_b32_e64 v7, 0, 1, s[10:11]", "\tv_add_u32_e32 v1, v2, v3", "\tv_add_u32_e32 v1, v2, v3", "\tv_add_u32_e32 v1, v2, v3",
            "\tv_cmp_ne_u32_e32 vcc, 0, v7",                      # too far away: not counted
            "\tv_cndmask_b32_e64 v8, v1, v2, s[10:11]", "\tv_cmp_ne_u32_e32 vcc, 0, v8",      # a real select
            "\tv_lshrrev_b64 v[2:3], v0, s[20:21]", "\tv_lshrrev_b64 v[2:3], v0, v[4:5]", "\tv_lshrrev_b64 v[32:33], 30, v[18:19]",
            "\tv_and_b32_e32 v13, s8, v67", "\tv_and_b32_e32 v12, s9, v66", "\tv_cmp_ne_u64_e32 vcc, 0, v[12:13]",
            "\tv_cmp_ne_u64_e32 vcc, 0, v[14:15]"]
    assert round_trip_pairs(loop) == 2
    assert sgpr_pair_shifts(loop) == 2


@pytest.mark.parametrize("what", ["pairs", "shifts", "valu"])
def test_no_more_than_the_finished_build_and_fewer_than_before(census, what):
    assert census[what] <= NOW[what], (what, census)
    assert census[what] < BEFORE[what], (what, census)
