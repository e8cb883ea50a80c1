"""Lane swaps and DPP reads of the wavefront ADMM tier (csrc/sco_admm_wv.hip), next to its inline assembly.

A statement of inline assembly is no VALU write to the compiler's hazard recogniser: a `v_permlane16_swap` /
`v_permlane32_swap` or a compiler-generated DPP move (`v_mov_b32_dpp` of the reductions, ...) that read the result of such a
statement directly would get no wait states.  Today every result that leaves wv_matvec is a compiler-visible `v_add_f64`, and the
hand-overs of the sweeps are builtins, so the compiler places these wait states itself; an edit that returns a statement's
output, or a compiler that schedules differently, would not be noticed by tests/test_wavefront_dpp_hazard.py, which looks at
the `v_fmac_f64_dpp` of the chains only.  This test looks at what was built in the same way, for every other reader of that
kind: in every qp_admm_wv* kernel, every operand of every lane swap and the DPP source of every `*_dpp` instruction must
not have been written by a VALU instruction fewer than two wait states earlier (every instruction in between is one,
`s_nop N` is N + 1; the scan is linear, as there)."""
import os
import re
import shutil
import subprocess

import pytest

from sco_py_amd import _lib
from test_wavefront_dpp_hazard import NEED, OBJDUMP, _parse, _regs, _written


def _reads(mn, ops):
    """VGPRs an instruction reads through the swap or DPP path: both operands of a lane swap, src0 of a DPP instruction."""
    if mn.startswith("v_permlane") and "swap" in mn:
        return set().union(*[_regs(o) for o in ops]) if ops else set()
    if "_dpp" in mn and len(ops) >= 2:
        return _regs(ops[1])
    return set()


def find_hazards(instrs):
    """instrs: [(mnemonic, operands)] of one kernel in program order -> [(index, wait states found)]."""
    bad = []
    for i, (mn, ops) in enumerate(instrs):
        src = _reads(mn, ops)
        if not src:
            continue
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


def test_scan_sees_planted_hazards():
    add = ("v_add_f64", ["v[6:7]", "v[6:7]", "v[8:9]"])
    swap = ("v_permlane32_swap_b32_e32", ["v20", "v7"])
    mov = ("v_mov_b32_dpp", ["v30", "v6", "quad_perm:[1,0,3,2]"])
    other = ("v_mov_b32_e32", ["v40", "v41"])
    assert find_hazards([add, swap]) == [(1, 0)]
    assert find_hazards([add, other, swap]) == [(2, 1)]
    assert find_hazards([add, ("s_nop", ["0"]), swap]) == [(2, 1)]
    assert find_hazards([add, ("s_nop", ["1"]), swap]) == []
    assert find_hazards([add, other, other, swap]) == []
    assert find_hazards([add, mov]) == [(1, 0)]
    assert find_hazards([add, other, other, mov]) == []
    # the second of two swaps in series reads what the first wrote
    assert find_hazards([other, other, ("v_permlane16_swap_b32_e32", ["v21", "v6"]), swap]) == []
    assert find_hazards([other, other, ("v_permlane16_swap_b32_e32", ["v21", "v7"]), swap]) == [(3, 0)]
    # a write of the destination of a DPP move is no DPP read
    assert find_hazards([("v_mov_b32_e32", ["v30", "v1"]), mov]) == []


def test_lane_swaps_and_dpp_reads_keep_their_wait_states(tmp_path):
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
        if "qp_admm_wv" not in out:
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
    swaps = dpp = 0
    for name, instrs in kernels.items():
        swaps += sum(1 for mn, _ in instrs if mn.startswith("v_permlane") and "swap" in mn)
        dpp += sum(1 for mn, _ in instrs if "_dpp" in mn)
        bad = find_hazards(instrs)
        assert not bad, "%s: %d swap / DPP reads of a VGPR written fewer than %d wait states earlier, first at instruction %d: %s" % (
            name, len(bad), NEED, bad[0][0], instrs[max(0, bad[0][0] - 3):bad[0][0] + 1])
    assert swaps > 0 and dpp > 0, (swaps, dpp)
    print("checked %d lane swaps and %d DPP instructions in %d kernels" % (swaps, dpp, len(kernels)))
