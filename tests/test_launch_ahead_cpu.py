"""CPU tests (-m "not gpu") of the launched-ahead form of the MPPI step (include/ctk_hip_ahead.h): the arming rule as the pure function
the library steps through (ctk_ahead_rule_step: sequences of eligibility, gaps and outcomes -> armed / not armed), and the header
against the Python table and the library's exports."""
import ctypes
import os
import re

from control_toolkit_amd import _capi
from control_toolkit_amd._capi import (AHEAD_ARM_AFTER, AHEAD_DISARM_AFTER, AHEAD_DEFAULT_FUSE_US, AHEAD_NONE, AHEAD_TAKEN, AHEAD_UNTAKEN,
                                       AHEAD_SYMBOLS, AheadRule, AheadCounters)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "ctk_hip.h")
AHEAD_HEADER = os.path.join(ROOT, "include", "ctk_hip_ahead.h")
FUSE = AHEAD_DEFAULT_FUSE_US


def run(seq, fuse=FUSE):
    """seq: (eligible, gap_us) per arriving step -> [armed] per step.  The outcome fed with a step is what the device would report for
    the launch the previous step issued: none if that step was not armed, taken if this one came within the fuse, else untaken."""
    lib = _capi.load_library()
    r = AheadRule()
    armed, prev = [], 0
    for eligible, gap in seq:
        outcome = AHEAD_NONE if not (prev and eligible) else (AHEAD_TAKEN if 0.0 <= gap <= fuse else AHEAD_UNTAKEN)
        prev = lib.ctk_ahead_rule_step(r, int(eligible), float(gap), float(fuse), outcome)
        armed.append(prev)
    return armed, r


def test_a_tight_loop_arms_after_arm_after_steps_and_stays_armed():
    armed, r = run([(1, -1.0)] + [(1, 4.0)] * 39)
    # step 0 has no previous result; steps 1 .. ARM_AFTER came within the fuse: the last of them arms
    assert armed == [0] * AHEAD_ARM_AFTER + [1] * (40 - AHEAD_ARM_AFTER)
    assert r.arms == 1 and r.untaken == 0
    assert sum(armed) - 1 == 40 - AHEAD_ARM_AFTER - 1          # launches of a 40-step loop that a following step can take


def test_a_slow_caller_never_arms():
    for gap in (FUSE * 1.01, 1000.0, 20000.0):
        armed, r = run([(1, -1.0)] + [(1, gap)] * 50)
        assert not any(armed) and r.arms == 0
    armed, _ = run([(1, -1.0)] + [(1, FUSE)] * AHEAD_ARM_AFTER)   # at the fuse exactly still counts
    assert armed[-1] == 1


def test_a_late_step_restarts_the_count_before_arming():
    seq = [(1, -1.0)] + [(1, 5.0)] * (AHEAD_ARM_AFTER - 1) + [(1, 2000.0)] + [(1, 5.0)] * AHEAD_ARM_AFTER
    armed, r = run(seq)
    assert armed == [0] * (2 * AHEAD_ARM_AFTER) + [1] and r.arms == 1
    # a gap every 5th step from the start: never ARM_AFTER tight steps in a row
    armed, _ = run([(1, 2000.0 if t % 5 == 4 else 5.0) for t in range(60)])
    assert not any(armed)


def test_an_ineligible_step_disarms_at_once():
    seq = [(1, -1.0)] + [(1, 5.0)] * 12 + [(0, 5.0)] + [(1, 5.0)] * AHEAD_ARM_AFTER
    armed, r = run(seq)
    assert armed[12] == 1 and armed[13] == 0
    assert armed[14:] == [0] * (AHEAD_ARM_AFTER - 1) + [1] and r.arms == 2


def test_single_gaps_keep_it_armed_and_two_in_a_row_disarm():
    tight = [(1, 5.0)] * 12
    seq = [(1, -1.0)] + tight + [(1, 2000.0 if t % 5 == 4 else 5.0) for t in range(40)]
    armed, r = run(seq)
    assert all(armed[AHEAD_ARM_AFTER:]) and r.arms == 1        # one untaken launch at a time: still armed
    assert AHEAD_DISARM_AFTER == 2
    seq += [(1, 5.0), (1, 2000.0), (1, 2000.0)] + tight      # (the 40th step of the loop was a late one: a tight step between)
    armed, r = run(seq)
    n = 1 + 12 + 40 + 1
    assert armed[n] == 1 and armed[n + 1] == 0                 # the second untaken launch in a row
    assert armed[n + 2:] == [0] * (AHEAD_ARM_AFTER - 1) + [1] * (12 - AHEAD_ARM_AFTER + 1) and r.arms == 2
    # a taken launch between two untaken ones starts the count of untaken launches over
    lib = _capi.load_library()
    r = AheadRule(streak=AHEAD_ARM_AFTER, armed=1)
    for outcome in (AHEAD_UNTAKEN, AHEAD_TAKEN, AHEAD_UNTAKEN, AHEAD_TAKEN):
        assert lib.ctk_ahead_rule_step(r, 1, 5.0, FUSE, outcome) == 1
    assert lib.ctk_ahead_rule_step(r, 1, 5.0, FUSE, AHEAD_UNTAKEN) == 1 and lib.ctk_ahead_rule_step(r, 1, 5.0, FUSE, AHEAD_UNTAKEN) == 0
    assert lib.ctk_ahead_rule_step(None, 1, 5.0, FUSE, AHEAD_NONE) == 0


def header_text():
    return re.sub(r"/\*.*?\*/", "", open(AHEAD_HEADER).read(), flags=re.S)


def test_header_declares_the_four_entries_and_the_library_exports_them():
    declared = sorted(set(re.findall(r"\b(ctk_[a-z_0-9]+)\s*\(", header_text())))
    want = ["ctk_ahead_enable", "ctk_ahead_kernel", "ctk_ahead_rule_step", "ctk_ahead_stats"]
    assert declared == want == sorted(AHEAD_SYMBOLS)
    assert re.search(r'^#include "ctk_hip_ahead.h"', open(HEADER).read(), flags=re.M)      # a caller includes one header
    lib = _capi.load_library()
    for name in want:
        assert hasattr(lib, name), f"libctk_hip.so does not export {name}"
    assert lib.ctk_abi_version() == 6
    others = set(_capi.SYMBOLS) | set(_capi.RUN_SYMBOLS) | set(_capi.EPISODE_SYMBOLS) | set(_capi.LOOP_SYMBOLS) | set(_capi.GRU_LOOP_SYMBOLS) | set(_capi.HYPER_SYMBOLS)
    assert not (set(want) & others)                                                        # the other headers' lists stay what they were


def test_constants_and_structs_match_the_header():
    text = header_text()
    assert int(re.search(r"#define CTK_AHEAD_ARM_AFTER (\d+)", text).group(1)) == AHEAD_ARM_AFTER
    assert int(re.search(r"#define CTK_AHEAD_DISARM_AFTER (\d+)", text).group(1)) == AHEAD_DISARM_AFTER
    assert float(re.search(r"#define CTK_AHEAD_DEFAULT_FUSE_US ([0-9.]+)", text).group(1)) == AHEAD_DEFAULT_FUSE_US
    enum = {m.group(1): int(m.group(2)) for m in re.finditer(r"CTK_AHEAD_(NONE|TAKEN|UNTAKEN)\s*=\s*(\d+)", text)}
    assert enum == {"NONE": AHEAD_NONE, "TAKEN": AHEAD_TAKEN, "UNTAKEN": AHEAD_UNTAKEN}
    for cls, name in ((AheadRule, "ctk_ahead_rule"), (AheadCounters, "ctk_ahead_counters")):
        body = re.search(r"typedef struct %s\s*\{(.*?)\}" % name, text, flags=re.S).group(1)
        fields = re.findall(r"\b(u?int(?:32|64)_t)\s+([a-z_]+)\s*;", body)
        assert [f for _, f in fields] == [f for f, _ in cls._fields_]
        for (ctype, _), (_, pytype) in zip(fields, cls._fields_):
            assert pytype is getattr(ctypes, "c_" + ctype.replace("_t", "")), (name, ctype, pytype)
