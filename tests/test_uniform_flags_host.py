"""Host, no GPU: wave-uniform conditions of the decision loop of k_rollout_fast stay on the scalar unit as condition codes or 32-bit words.

The mirror of the lane-predicate rule (common.hpp, "Wave-uniform conditions"; tests/test_mask_idioms_host.py has the lane predicates):
a uniform bool that crosses a basic block is held by the compiler as a 64-bit lane mask -- `s_cselect_b64 s[a:b], -1, 0` -- and
re-formed at every use -- `s_and_b64` / `s_andn2_b64 vcc, exec, s[a:b]` + `s_cbranch_vcc*` -- where `s_cmp` + `s_cbranch_scc` would do;
a constant mask folded as a literal is ANDed half by half (`s_and_b32 sHi, sHi, 0x3ffff` + `s_mov_b32 sLo, sLo` for the 50 task
lanes).  No test of results can see either; this one reads the compiler's output, compiled the way tools/loop_insts.py compiles it
(the product's flags, one explicit instantiation), for the plain, PRIO, renewing and logging forms of k_rollout_fast<20, 50>.

Per decision loop: no lane-mask flag whose only consumers are exec-ANDs that feed a vcc branch, no 0x3ffff literal AND, no
v_writelane, no scratch instruction, four waves per SIMD, and at most the instructions the finished build reaches:

                                    parent commit                       this build
                                    loop   lane-mask flags   literal    loop   lane-mask flags   literal   VGPRs   scratch
    plain                           1122         14             5       1077          0             0       107       0
    PRIO                            1164         15             5       1114          0             0       107       0
    renewing (k_rn_)                1128         14             5       1077          0             0       115      96
    logging  (k_lg_)                1229         15             5       1166          0             0       110       0

("lane-mask flags" counts every `s_cselect_b64 ..., -1, 0` of the loop; the assertion is on those consumed by exec-ANDs and a vcc branch
alone: 4, 4, 4 and 5 of them at the parent commit.)  VGPRs <= 108 and no scratch are the plain and the PRIO form's bounds, the two forms that are k_rollout_fast<20, 50> itself.  The
renewing form's 96 bytes of scratch belong to the instance generator it calls between episodes, the logging form carries the log's
registers: for those two the kernel-wide figures are bounded by the parent commit's (116 / 96, 111 / 0), and the loop itself holds no
scratch instruction in any form."""
import os
import re
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H = "20, 50, false, true, false"
# form: (kernel, template arguments, --extra-args, unit macro, loop instructions of the parent, reached, VGPR bound, scratch bound)
FORMS = {"plain": ("k_rollout_fast", H, "", "", 1122, 1077, 108, 0),
         "prio": ("k_rollout_fast", "20, 50, false, true, true", "", "", 1164, 1114, 108, 0),
         "renewing": ("k_rn_rollout_fast", H, "Renew", "", 1128, 1077, 116, 96),
         "logging": ("k_lg_rollout_fast", H, "int, RouteLog", "-DDCM_TU_L", 1229, 1166, 111, 0)}


def instructions(loop):
    return [l.split(";")[0].strip() for l in loop if re.match(r"\s+[a-z]", l)]


def lane_mask_flags(loop):
    """(all, bad): every `s_cselect_b64 s[a:b], -1, 0`, and those whose only readers -- up to the pair's next definition, in text order
    -- are `s_and_b64` / `s_andn2_b64 <dst>, exec, s[a:b]` (either operand order) with a `s_cbranch_vcc*` behind the first of them"""
    insts = instructions(loop)
    every, bad = 0, 0
    for i, l in enumerate(insts):
        m = re.match(r"s_cselect_b64\s+(s\[(\d+):(\d+)\]), -1, 0$", l)
        if not m:
            continue
        every += 1
        pair, lo, hi = m.group(1), m.group(2), m.group(3)
        readers = []
        for j in range(i + 1, len(insts)):
            ops = re.split(r"[\s,]+", insts[j], maxsplit=1)
            rest = ops[1] if len(ops) > 1 else ""
            dst, _, src = rest.partition(",")
            reads = re.search(re.escape(pair) + r"|\bs(?:%s|%s)\b" % (lo, hi), src if src else "")
            if ops[0].startswith(("s_cbranch", "s_branch", "s_cmp", "s_bitcmp")):      # (no destination operand)
                reads = re.search(re.escape(pair) + r"|\bs(?:%s|%s)\b" % (lo, hi), rest)
                dst = ""
            if reads:
                readers.append(j)
            if dst.strip() == pair or re.fullmatch(r"s(?:%s|%s)" % (lo, hi), dst.strip()):
                break
        exec_and = re.compile(r"s_and(?:n2)?_b64\s+(?:vcc|s\[\d+:\d+\]), (?:exec, " + re.escape(pair) + "|" + re.escape(pair) + ", exec)$")
        if readers and all(exec_and.match(insts[j]) for j in readers) and \
                any(x.startswith("s_cbranch_vcc") for x in insts[readers[0] + 1:readers[0] + 40]):
            bad += 1
    return every, bad


def literal_ands(loop):
    return sum(1 for l in instructions(loop) if re.match(r"s_and_b32\s+s\d+, s\d+, 0x3ffff$", l))


_census = {}


def census(form, tmp_path_factory):
    if form not in _census:
        hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
        if not os.path.exists(hipcc):
            pytest.skip("hipcc not available")
        kernel, targs, extra, unit = FORMS[form][:4]
        loop = tmp_path_factory.mktemp("uniform") / "loop.s"
        out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "loop_insts.py"), "--kernel", f"{kernel}<{targs}>", "--dump", str(loop)] +
                             (["--extra-args", extra] if extra else []) + ([unit] if unit else []), capture_output=True, text=True, timeout=600)
        assert out.returncode == 0, out.stderr[-2000:]
        m = re.search(r"VGPRs: (\d+).*ScratchSize \[bytes/lane\]: (\d+).*Occupancy \[waves/SIMD\]: (\d+)", out.stdout)
        n = re.search(r"decision loop \S+ of .*: (\d+) instructions, (\d+) VALU", out.stdout)
        assert m and n, out.stdout
        lines = loop.read_text().splitlines()
        every, bad = lane_mask_flags(lines)
        insts = instructions(lines)
        _census[form] = dict(vgprs=int(m.group(1)), scratch=int(m.group(2)), waves=int(m.group(3)), loop=int(n.group(1)),
                             flags=every, bad_flags=bad, literal=literal_ands(lines),
                             writelane=sum(1 for x in insts if x.startswith("v_writelane")),
                             scratch_insts=sum(1 for x in insts if x.startswith("scratch_")))
        print(form, _census[form], "parent loop", FORMS[form][4])
    return _census[form]


def test_the_patterns_find_what_they_describe():
    """The counters on hand-written lines (so that a change of the compiler's spelling is not mistaken for zero)"""
    loop = ["\ts_cmp_lg_u32 s2, 0", "\ts_cselect_b64 s[4:5], -1, 0", "\ts_mov_b64 s[24:25], -1", "\ts_and_b64 vcc, exec, s[4:5]",
            "\tv_add_u32_e32 v1, v2, v3", "\ts_cbranch_vccnz .LBB10_210", "\ts_andn2_b64 vcc, exec, s[4:5]", "\ts_cbranch_vccnz .LBB10_211",
            "\ts_mov_b64 s[4:5], 0",
            "\ts_cselect_b64 s[6:7], -1, 0", "\ts_and_b64 s[6:7], s[0:1], s[6:7]",                   # combined on the masks: not this pattern
            "\ts_cselect_b64 s[8:9], -1, 0", "\tv_cndmask_b32_e64 v18, 0, 1, s[8:9]",                # a bool made a number: not this pattern
            "\ts_cselect_b64 s[10:11], -1, 0", "\ts_andn2_b64 vcc, exec, s[10:11]", "\ts_cbranch_vccz .LBB10_3",
            "\ts_and_b32 s1, s1, 0x3ffff", "\ts_mov_b32 s0, s0", "\ts_and_b32 s48, s2, 0xfffff", "\ts_and_b64 s[0:1], s[0:1], s[88:89]"]
    assert lane_mask_flags(loop) == (4, 2)
    assert literal_ands(loop) == 1


@pytest.mark.parametrize("form", list(FORMS))
def test_uniform_conditions_stay_scalar(form, tmp_path_factory):
    c = census(form, tmp_path_factory)
    _, _, _, _, parent, reached, vgprs, scratch = FORMS[form]
    assert c["bad_flags"] == 0, c
    assert c["literal"] == 0, c
    assert c["writelane"] == 0 and c["scratch_insts"] == 0, c
    assert c["scratch"] <= scratch and c["vgprs"] <= vgprs and c["waves"] == 4, c
    assert c["loop"] <= reached < parent, c
