"""The DPP broadcasts of the wavefront ADMM tier (csrc/sco_admm_wv.hip: wv_matvec) read their broadcast operand through
the DPP path: a VALU write of that register needs two wait states before a `v_fmac_f64_dpp` may read it.  The chain is
inline assembly, which the compiler's hazard recogniser does not look into, so this test looks at what was built: it
disassembles the library's gfx950 code object and checks every `v_fmac_f64_dpp` of every qp_admm_wv* kernel against the
instructions in front of it.

Wait states are counted the way the ISA manual counts them for this hazard: every instruction between the write and the
read is one, `s_nop N` is N + 1.  The scan is linear (a branch target inside the window is not followed), which is enough
for the straight-line sweep code the broadcasts sit in."""
import os
import re
import shutil
import subprocess

import pytest

from sco_py_amd import _lib

OBJDUMP = "/opt/rocm/lib/llvm/bin/llvm-objdump"
NEED = 2          # wait states between a VALU write of a VGPR and a DPP read of it


def _regs(op):
    """VGPR numbers named by one operand ('v5', 'v[6:7]', '-v[6:7]', '|v3|'), or an empty set."""
    m = re.fullmatch(r"[-|]*v\[(\d+):(\d+)\][|]*", op)
    if m:
        return set(range(int(m.group(1)), int(m.group(2)) + 1))
    m = re.fullmatch(r"[-|]*v(\d+)[|]*", op)
    return {int(m.group(1))} if m else set()


def _parse(line):
    """(mnemonic, [operands]) of one disassembly line, or None."""
    text = line.split("//")[0].strip()
    if not text or text.endswith(":") or re.match(r"^[0-9a-f]+ <", text):
        return None
    parts = text.split(None, 1)
    ops = [o.strip().split()[0] for o in parts[1].split(",")] if len(parts) > 1 and parts[1].strip() else []
    return parts[0], ops


def _written(mn, ops):
    """VGPRs a VALU instruction writes (first operand; both operands of the swaps)."""
    if not mn.startswith("v_") or not ops:
        return set()
    if "swap" in mn:
        return set().union(*[_regs(o) for o in ops])
    return _regs(ops[0])


def find_hazards(instrs):
    """instrs: [(mnemonic, operands)] of one kernel in program order -> [(index, wait states found)]."""
    bad = []
    for i, (mn, ops) in enumerate(instrs):
        if not mn.startswith("v_fmac_f64_dpp") or len(ops) < 2:
            continue
        src = _regs(ops[1])
        ws = 0
        for pm, po in reversed(instrs[max(0, i - 8):i]):
            if ws >= NEED:
                break
            if pm == "s_nop":
                ws += int(po[0], 0) + 1 if po else 1
                continue
            if _written(pm, po) & src:
                bad.append((i, ws))
                break
            ws += 1
    return bad


def test_hazard_scan_sees_a_planted_hazard():
    """The scan itself: a write directly in front of the broadcast, one with s_nop 0 and one with s_nop 1 between."""
    dpp = ("v_fmac_f64_dpp", ["v[2:3]", "v[6:7]", "v[8:9]"])
    wr = ("v_fma_f64", ["v[6:7]", "-v[42:43]", "v[2:3]", "v[62:63]"])
    assert find_hazards([wr, dpp]) == [(1, 0)]
    assert find_hazards([wr, ("s_nop", ["0"]), dpp]) == [(2, 1)]
    assert find_hazards([wr, ("s_nop", ["1"]), dpp]) == []
    assert find_hazards([wr, ("v_mov_b32_e32", ["v9", "v1"]), ("ds_read_b64", ["v[10:11]", "v4"]), dpp]) == []
    # the accumulator of the chain's previous step is not the broadcast operand
    assert find_hazards([wr, ("s_nop", ["1"]), dpp, ("v_fmac_f64_dpp", ["v[4:5]", "v[6:7]", "v[10:11]"])]) == []
    assert find_hazards([("v_permlane16_swap_b32_e32", ["v1", "v6"]), dpp]) == [(1, 0)]


def test_wavefront_dpp_chains_keep_their_wait_states(tmp_path):
    if not os.path.exists(OBJDUMP):
        pytest.skip("llvm-objdump not found")
    lib = _lib.lib_path()
    assert os.path.exists(lib), "library not built"
    work = str(tmp_path)
    shutil.copy(lib, os.path.join(work, "lib.so"))
    subprocess.run([OBJDUMP, "--offloading", "lib.so"], cwd=work, check=True, stdout=subprocess.DEVNULL)
    kernels = {}
    for f in sorted(os.listdir(work)):
        if "amdgcn" not in f:
            continue
        out = subprocess.run([OBJDUMP, "-d", f], cwd=work, check=True, capture_output=True, text=True).stdout
        if "v_fmac_f64_dpp" not in out:
            continue
        cur = None
        for line in out.splitlines():
            m = re.match(r"^[0-9a-f]+ <(\S+)>:", line)
            if m:
                cur = m.group(1) if "qp_admm_wv" in m.group(1) else None
                if cur:
                    kernels[cur] = []
                continue
            if cur:
                p = _parse(line)
                if p:
                    kernels[cur].append(p)
    assert kernels, "no qp_admm_wv* kernel in the library's code objects"
    chains = 0
    for name, instrs in kernels.items():
        n = sum(1 for mn, _ in instrs if mn.startswith("v_fmac_f64_dpp"))
        assert n > 0, "%s: no v_fmac_f64_dpp" % name
        chains += n
        bad = find_hazards(instrs)
        assert not bad, "%s: %d DPP reads of a VGPR written fewer than %d wait states earlier, first at instruction %d: %s" % (
            name, len(bad), NEED, bad[0][0], instrs[max(0, bad[0][0] - 3):bad[0][0] + 1])
    print("checked %d v_fmac_f64_dpp in %d kernels" % (chains, len(kernels)))
