"""Code-generation guards of the publish of u in the headline MPPI kernel, ctk_mppi_rollout<0, 0, false, false> (its early order:
ctk_mppi_body_5_post.inc, EARLY_U).  No GPU needed: the built library is disassembled (as tests/test_mppi_recurrence_isa.py does).

  * between the division of the early update (its v_div_fixup_f32) and the 8-byte system-scope store {u, seq} the host spins on
    (global_store_dwordx2 ... sc0 sc1) there is no write-back of the L2 (buffer_wbl2) and no drain of the wave's stores
    (s_waitcnt vmcnt(0)) — except the drain directly behind the store of the error word (global_store_dword ... offset:8 sc0 sc1),
    which only the branch that raises the word executes (ctk_device.h: publish_u_launched, host_word_store);
  * the change is scoped: the resident kernel, which does not end behind its publish, still releases (buffer_wbl2);
  * the two fast column sums wait for LDS once: between the v_exp_f32 of the block's soft-min weights and the store of the column
    sums, the LDS reads are issued as ONE group (a group = consecutive ds_read instructions with no s_waitcnt lgkmcnt between them;
    every further group is a further dependent LDS round trip on the way to u — there were five)."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OBJDUMP = "/opt/rocm/lib/llvm/bin/llvm-objdump"
KERNEL = "_Z16ctk_mppi_rolloutILi0ELi0ELb0ELb0EEv"          # ctk_mppi_rollout<0, 0, false, false>: four template arguments = FORM 0
RESIDENT = "_Z17ctk_mppi_residentILi0ELi0EEv"               # ctk_mppi_resident<0, 0>


@pytest.fixture(scope="module")
def listing(tmp_path_factory):
    lib = os.path.join(ROOT, "control_toolkit_amd", "libctk_hip.so")
    if not os.path.exists(OBJDUMP) or not os.path.exists(lib):
        pytest.skip("llvm-objdump or the built library is not here")
    tmp = tmp_path_factory.mktemp("isa")
    shutil.copy(lib, str(tmp / "libctk_hip.so"))
    subprocess.run([OBJDUMP, "--offloading", "libctk_hip.so"], cwd=str(tmp), capture_output=True, text=True, timeout=120)
    for name in sorted(os.listdir(str(tmp))):
        if name.endswith("gfx950"):
            text = subprocess.run([OBJDUMP, "-d", "--no-show-raw-insn", name], cwd=str(tmp), capture_output=True, text=True, timeout=300).stdout
            if "<" + KERNEL in text:
                return text.splitlines()
    pytest.fail("ctk_mppi_rollout<0, 0, false, false> is not in the library")


def kernel_body(listing, sym):
    """[(opcode, operands)] of one kernel, in address order."""
    start = next(i for i, l in enumerate(listing) if re.match(r"^[0-9a-f]+ <%s" % re.escape(sym), l))
    end = next((i for i in range(start + 1, len(listing)) if re.match(r"^[0-9a-f]+ <.*>:", listing[i])), len(listing))
    out = []
    for l in listing[start + 1:end]:
        m = re.match(r"^\s+(\S+)\s*(.*?)\s*//\s*([0-9A-Fa-f]+):", l)
        if m:
            out.append((m.group(1), m.group(2)))
    return out


def is_system_store8(x):
    return x[0] == "global_store_dwordx2" and re.search(r"\bsc0\b", x[1]) and re.search(r"\bsc1\b", x[1])


def is_agent_store8(x):
    return x[0] == "global_store_dwordx2" and re.search(r"\bsc1\b", x[1]) and not re.search(r"\bsc0\b", x[1])


def drains_stores(x):
    return x[0] == "s_waitcnt" and re.search(r"\bvmcnt\(0\)", x[1]) is not None


def early_publish(body):
    """(index of the early update's v_div_fixup_f32, index of the {u, seq} store behind it)"""
    flag = next((i for i, x in enumerate(body) if is_system_store8(x)), None)
    assert flag is not None, "no 8-byte system-scope store: the early publish is not in the kernel"
    div = max((i for i in range(flag) if body[i][0] == "v_div_fixup_f32"), default=None)
    assert div is not None, "no v_div_fixup_f32 ahead of the {u, seq} store"
    return div, flag


def test_early_publish_has_no_write_back_and_no_drain_on_the_path(listing):
    body = kernel_body(listing, KERNEL)
    div, flag = early_publish(body)
    print(f"{flag - div} instructions from the early update's division to the {{u, seq}} store")
    for i in range(div + 1, flag):
        op, operands = body[i]
        assert op != "buffer_wbl2", f"buffer_wbl2 {operands} between the division and the {{u, seq}} store: the publish releases"
        if drains_stores(body[i]):
            prev = body[i - 1]
            err_word = prev[0] == "global_store_dword" and "offset:8" in prev[1] and "sc0" in prev[1] and "sc1" in prev[1]
            assert err_word, "s_waitcnt vmcnt(0) between the division and the {u, seq} store outside the error branch"
    # the error word's own drain exists somewhere ahead of the flag (the `late` branch), directly behind the word's store
    errs = [i for i in range(flag) if body[i][0] == "global_store_dword" and "offset:8" in body[i][1] and "sc0" in body[i][1] and "sc1" in body[i][1]]
    assert errs and all(drains_stores(body[i + 1]) for i in errs), "the error word is not drained ahead of the {u, seq} store"
    # nothing in this kernel releases at all: every end-of-step publish of a launched kernel is the relaxed one
    assert not any(x[0] == "buffer_wbl2" for x in body)


def test_resident_kernel_still_releases(listing):
    body = kernel_body(listing, RESIDENT)
    assert any(x[0] == "buffer_wbl2" for x in body), "the resident kernel lost its release: the change was not scoped to the launched kernels"
    # ... and it is the publish's: a system-scope write-back within the few instructions ahead of an 8-byte system-scope store
    # (its pointers come out of device memory, not out of kernel arguments: the store is a flat one)
    flags = [i for i, x in enumerate(body) if x[0] in ("global_store_dwordx2", "flat_store_dwordx2") and "sc0" in x[1] and "sc1" in x[1]]
    assert flags, "no 8-byte system-scope store in the resident kernel"
    for i in flags:
        ahead = body[max(0, i - 4):i]
        assert any(x[0] == "buffer_wbl2" and "sc0" in x[1] and "sc1" in x[1] for x in ahead), "a {u, seq} store of the resident kernel without its release"


def test_fast_column_sums_wait_for_lds_once(listing):
    body = kernel_body(listing, KERNEL)
    _, flag = early_publish(body)
    col = max((i for i in range(flag) if is_agent_store8(body[i])), default=None)      # the last record word stored ahead of the early merge
    assert col is not None, "no agent-scope 8-byte store ahead of the early publish"
    exp = max((i for i in range(col) if body[i][0].startswith("v_exp_f32")), default=None)   # the soft-min weights e = exp(-(J - rho)/lambda)
    assert exp is not None
    groups, open_group = 0, False
    for op, operands in body[exp + 1:col]:
        if op.startswith("ds_read"):
            if not open_group:
                groups += 1
                open_group = True
        elif op == "s_waitcnt" and "lgkmcnt" in operands:
            open_group = False
    print(f"{col - exp} instructions from the soft-min's v_exp_f32 to the column-sum store, {groups} group(s) of LDS reads")
    assert groups <= 1, f"{groups} dependent groups of LDS reads between the soft-min weights and the column-sum store"
