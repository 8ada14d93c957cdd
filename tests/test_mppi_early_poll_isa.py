"""Code-generation guards of the early poll of the headline MPPI kernel, ctk_mppi_rollout<0, 0, false, false> (ctk_mppi_merge.h:
mppi_early_u, inlined into the kernel body).  No GPU needed: the built library is disassembled (as tests/test_mppi_recurrence_isa.py does).

The poll keeps LL_EARLY_DEPTH passes of 8-byte agent-scope loads (global_load_dwordx2 ... sc1) in flight.  That only holds while
  * the wait in front of a pass's check is a PARTIAL one: every s_waitcnt between the loads of one pass and the loads of the next (or
    the loop's end) names vmcnt(n) with n >= the loads of one pass, so the pass issued last stays outstanding while the older one is
    looked at (a branch around a load makes the compiler wait vmcnt(0) at the join: the poll has none);
  * nothing waits for the pass still in flight once the poll is left: from the poll's last check to the first v_exp_f32 of the merge
    (the soft-min weights of the blocks' records) there is no s_waitcnt vmcnt(0) — nor any vmcnt below the loads of one pass."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OBJDUMP = "/opt/rocm/lib/llvm/bin/llvm-objdump"
KERNEL = "_Z16ctk_mppi_rolloutILi0ELi0ELb0ELb0EEv"          # ctk_mppi_rollout<0, 0, false, false>: four template arguments = FORM 0


@pytest.fixture(scope="module")
def body(tmp_path_factory):
    """[(opcode, operands)] of the kernel, in address order"""
    lib = os.path.join(ROOT, "control_toolkit_amd", "libctk_hip.so")
    if not os.path.exists(OBJDUMP) or not os.path.exists(lib):
        pytest.skip("llvm-objdump or the built library is not here")
    tmp = tmp_path_factory.mktemp("isa")
    shutil.copy(lib, str(tmp / "libctk_hip.so"))
    subprocess.run([OBJDUMP, "--offloading", "libctk_hip.so"], cwd=str(tmp), capture_output=True, text=True, timeout=120)
    for name in sorted(os.listdir(str(tmp))):
        if name.endswith("gfx950"):
            listing = subprocess.run([OBJDUMP, "-d", "--no-show-raw-insn", name], cwd=str(tmp), capture_output=True, text=True, timeout=300).stdout.splitlines()
            starts = [i for i, l in enumerate(listing) if re.match(r"^[0-9a-f]+ <%s" % re.escape(KERNEL), l)]
            if starts:
                start = starts[0]
                end = next((i for i in range(start + 1, len(listing)) if re.match(r"^[0-9a-f]+ <.*>:", listing[i])), len(listing))
                out = []
                for l in listing[start + 1:end]:
                    m = re.match(r"^\s+(\S+)\s*(.*?)\s*//\s*([0-9A-Fa-f]+):", l)
                    if m:
                        out.append((m.group(1), m.group(2)))
                return out
    pytest.fail("ctk_mppi_rollout<0, 0, false, false> is not in the library")


def is_poll_load(x):
    return x[0] == "global_load_dwordx2" and re.search(r"\bsc1\b", x[1]) and not re.search(r"\bsc0\b", x[1])


def vmcnt(x):
    """n of an s_waitcnt that names vmcnt(n), else None"""
    m = re.search(r"\bvmcnt\((\d+)\)", x[1]) if x[0] == "s_waitcnt" else None
    return int(m.group(1)) if m else None


def passes(body):
    """[(index of the first load, index behind the last load)] of each run of consecutive poll loads = one pass"""
    idx = [i for i, x in enumerate(body) if is_poll_load(x)]
    assert idx, "no 8-byte agent-scope load: the early poll is not in the kernel body"
    runs, first, prev = [], idx[0], idx[0]
    for i in idx[1:]:
        if i != prev + 1:
            runs.append((first, prev + 1))
            first = i
        prev = i
    runs.append((first, prev + 1))
    return runs


def poll_end(body, runs):
    """index behind the last check: the first backward-or-forward branch behind the last pass's partial waits ends the loop body"""
    return next(i for i in range(runs[-1][1], len(body)) if body[i][0].startswith("s_cbranch") or body[i][0] == "s_branch")


def test_the_wait_in_front_of_a_check_leaves_the_younger_pass_in_flight(body):
    runs = passes(body)
    per_pass = runs[0][1] - runs[0][0]
    assert len(runs) >= 2 and all(b - a == per_pass for a, b in runs), f"passes of unequal size or a single pass: {[b - a for a, b in runs]}"
    for k, (_, behind) in enumerate(runs):
        stop = runs[k + 1][0] if k + 1 < len(runs) else poll_end(body, runs)
        waits = [vmcnt(body[i]) for i in range(behind, stop) if vmcnt(body[i]) is not None]
        print(f"pass {k}: {per_pass} loads, waits behind them: {waits}")
        assert waits, f"no s_waitcnt vmcnt behind the loads of pass {k}: its check is not behind them"
        assert min(waits) >= per_pass, f"s_waitcnt vmcnt({min(waits)}) behind the {per_pass} loads of pass {k}: the check waits for the pass just issued"


def test_nothing_waits_for_the_pass_in_flight_between_the_poll_and_the_merge(body):
    runs = passes(body)
    per_pass = runs[0][1] - runs[0][0]
    last_check = max(i for i in range(runs[-1][1], poll_end(body, runs)) if vmcnt(body[i]) is not None)
    exp = next((i for i in range(last_check, len(body)) if body[i][0].startswith("v_exp_f32")), None)
    assert exp is not None, "no v_exp_f32 behind the poll: the early merge is not in the kernel body"
    waits = [vmcnt(body[i]) for i in range(last_check + 1, exp) if vmcnt(body[i]) is not None]
    print(f"{exp - last_check} instructions from the poll's last check to the merge's v_exp_f32, vmcnt waits between: {waits}")
    assert all(n >= per_pass for n in waits), f"s_waitcnt vmcnt({min(waits)}) between the poll and the merge: it waits for a pass that is not used"
