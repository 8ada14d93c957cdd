"""Code-generation guards of the headline MPPI kernel, ctk_mppi_rollout<0, 0, false, false> (BASELINE configs[1], bench.py's default
workload).  No GPU needed: the built library is disassembled.

  * the recurrence carries sin / cos of the angle one step ahead (ctk_env.h: recur_env_range, PIPE): in the fast-path loop every
    v_rcp_f32 (the quotient of a step's dynamics) is preceded by a v_rndne_f32 that it does NOT depend on — the range reduction of the
    NEXT step's angle, issued beside this step's dynamics.  The previous loop ran the two chains back to back: each v_rcp_f32 depended
    on the v_rndne_f32 just before it;
  * no more VALU per step than the previous loop (52);
  * the tail of at most 128 records (ctk_launch.h: CTK_MPPI_FORM_WIDE_TAIL clear) has no 16-deep poll batch."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OBJDUMP = "/opt/rocm/lib/llvm/bin/llvm-objdump"
READELF = "/opt/rocm/lib/llvm/bin/llvm-readelf"
KERNEL = "_Z16ctk_mppi_rolloutILi0ELi0ELb0ELb0EEv"          # ctk_mppi_rollout<0, 0, false, false>: four template arguments = FORM 0


@pytest.fixture(scope="module")
def code_object(tmp_path_factory):
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
                return str(tmp / name), text.splitlines()
    pytest.fail("ctk_mppi_rollout<0, 0, false, false> is not in the library")


def kernel_body(listing, sym):
    """[(address, opcode, operands)] of one kernel."""
    start = next(i for i, l in enumerate(listing) if re.match(r"^[0-9a-f]+ <%s" % re.escape(sym), l))
    end = next((i for i in range(start + 1, len(listing)) if re.match(r"^[0-9a-f]+ <.*>:", listing[i])), len(listing))
    base = int(listing[start].split()[0], 16)
    out = []
    for l in listing[start + 1:end]:
        m = re.match(r"^\s+(\S+)\s*(.*?)\s*//\s*([0-9A-Fa-f]+):", l)
        if m:
            tgt = re.search(r"<\S+\+0x([0-9a-f]+)>", l)
            out.append((int(m.group(3), 16), m.group(1), m.group(2), base + int(tgt.group(1), 16) if tgt else None))
    return out


def regs(text):
    """VGPR / SGPR / vcc names an operand list mentions (ranges expanded)."""
    out = set()
    for kind, a, b in re.findall(r"\b([vs])\[(\d+):(\d+)\]", text):
        out.update(f"{kind}{i}" for i in range(int(a), int(b) + 1))
    out.update(re.findall(r"\b([vs]\d+)\b", re.sub(r"[vs]\[\d+:\d+\]", "", text)))
    if re.search(r"\bvcc\b", text):
        out.add("vcc")
    return out


def depends_on(loop, j, i):
    """Does instruction j of the straight-line loop body read (through the body, not around the back edge) what instruction i wrote?"""
    need = set()
    ops = loop[j][2].split(",", 1)
    need |= regs(ops[1] if len(ops) > 1 else "")
    for k in range(j - 1, i - 1, -1):
        _, op, operands, _ = loop[k]
        if not op.startswith("v_") and not op.startswith("ds_"):
            continue
        parts = operands.split(",", 1)
        dst = regs(parts[0])
        if op.startswith("v_cmp") and "_e32" in op:
            dst = {"vcc"}
        if dst & need:
            if k == i:
                return True
            need -= dst
            need |= regs(parts[1] if len(parts) > 1 else "")
            if "mac" in op or "fmac" in op:              # v_fmac / v_mac: the destination is also the addend
                need |= dst
    return False


def recurrence_loops(body):
    """The fast-path loops of the recurrence: backward branches over a body with two v_rndne_f32, two v_rcp_f32 and no other loop."""
    loops = []
    for addr, op, _, tgt in body:
        if op.startswith("s_cbranch") and tgt is not None and tgt < addr:
            seg = [x for x in body if tgt <= x[0] <= addr]
            ops = [x[1] for x in seg]
            inner = any(x[1].startswith("s_cbranch") and x[3] is not None and x[3] < x[0] for x in seg[:-1])
            if not inner and sum(o.startswith("v_rndne_f32") for o in ops) == 2 and sum(o.startswith("v_rcp_f32") for o in ops) == 2:
                loops.append(seg)
    return loops


def test_headline_recurrence_overlaps_the_next_steps_sincos(code_object):
    _, listing = code_object
    loops = recurrence_loops(kernel_body(listing, KERNEL))
    assert len(loops) == 2, f"expected the fast-path loop twice (steps [0, S1) and [S1, H)), found {len(loops)}"
    for loop in loops:
        valu = sum(x[1].startswith("v_") for x in loop)
        assert valu <= 2 * 52, f"{valu} VALU per two steps: more than the previous loop's 52 per step"
        for j, x in enumerate(loop):
            if not x[1].startswith("v_rcp_f32"):
                continue
            prev = [i for i in range(j) if loop[i][1].startswith("v_rndne_f32")]
            assert prev, "a step's v_rcp_f32 issues before any v_rndne_f32 of the loop body: the next angle's sin / cos is not ahead"
            i = prev[-1]
            assert not depends_on(loop, j, i), (f"the v_rcp_f32 at {x[0]:#x} depends on the v_rndne_f32 at {loop[i][0]:#x} before it: "
                                                "the step's dynamics wait for its own sin / cos (the chains are not overlapped)")
        assert sum(x[1] == "s_cbranch_scc1" or x[1] == "s_cbranch_scc0" for x in loop) == 1, "the one-ahead input read is guarded inside the loop"


def test_headline_tail_has_no_16_deep_poll_and_fewer_registers(code_object):
    """The {value, seq} poll of block 0: without the wide form, 8 words per thread in flight (8 loads + 8 re-reads of a word not yet
    there: 16 agent-scope 8-byte loads, 8 sleeps); the wide form adds the 16-deep batch (48 loads, 24 sleeps).
    VGPRs: `.vgpr_count` of the kernel in the code object's metadata — what the assembler allocates (70 with the wide tail compiled
    in, as before this form existed).  rocprofv3's kernel trace prints another figure for the same kernel (36 at 70); the two are
    not compared."""
    co, listing = code_object
    body = kernel_body(listing, KERNEL)
    loads = sum(1 for x in body if x[1].startswith("global_load_dwordx2") and re.search(r"\bsc1\b", x[2]))
    sleeps = sum(1 for x in body if x[1] == "s_sleep")
    assert loads <= 16 and sleeps <= 8, f"{loads} agent-scope 8-byte loads and {sleeps} sleeps: the 16-deep poll batch is compiled in"
    notes = subprocess.run([READELF, "--notes", co], capture_output=True, text=True, timeout=120).stdout
    entry = next(b for b in notes.split("- .agpr_count")[1:] if re.search(r"\.name:\s+%s" % re.escape(KERNEL), b))
    vgpr = int(re.search(r"\.vgpr_count:\s+(\d+)", entry).group(1))
    spill = int(re.search(r"\.vgpr_spill_count:\s+(\d+)", entry).group(1))
    print(f"ctk_mppi_rollout<0, 0, false, false>: .vgpr_count {vgpr}, .vgpr_spill_count {spill}")
    assert spill == 0
    assert vgpr < 70, f".vgpr_count {vgpr}: no fewer than with the wide tail compiled in (70)"
