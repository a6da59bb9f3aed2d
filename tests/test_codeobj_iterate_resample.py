"""Build-time check of k_iterate_xr, the exact iteration that resamples the coarser flow as it fetches it (no GPU needed).

k_iterate_xr<MH> is the strip walker of k_iterate_x<MH, false> with another flow source (FlowResample2x,
iterate_common.h), so it lives under the same budget -- 168 VGPRs for three waves per SIMD, no AGPRs, nothing spilled, no
scratch, a code size two CUs' instruction cache holds -- and its I/O wave fetches the neighbour's carries with the same
hand-written loads and the same counted wait, which must stay covered by younger vector-memory instructions on every path
(test_codeobj_waits.py has the rule; its helpers are used here).
"""
import os
import re
import subprocess

import pytest

from test_codeobj_iterate_stream import CODE_BYTES_MAX, VGPR_BUDGET, kernel_metadata
from test_codeobj_waits import X_SRC, _gfx950_code_objects, _llvm_tool, counted_waits, parse_disasm

_SYM = re.compile(r"k_iterate_xrILi(\d+)EE")


@pytest.fixture(scope="module")
def xr_kernels(nsof_lib, tmp_path_factory):
    """{MH: (instructions, metadata)} of every k_iterate_xr in libnsof.so."""
    objcopy, objdump, readelf = _llvm_tool("llvm-objcopy"), _llvm_tool("llvm-objdump"), _llvm_tool("llvm-readelf")
    if not (objcopy and objdump and readelf):
        pytest.skip("the ROCm LLVM tools (llvm-objcopy, llvm-objdump, llvm-readelf) are not installed")
    tmp = tmp_path_factory.mktemp("codeobj_xr")
    so = os.path.join(os.path.dirname(nsof_lib.__file__), "libnsof.so")
    fat = tmp / "fatbin"
    subprocess.run([objcopy, f"--dump-section=.hip_fatbin={fat}", so, str(tmp / "stripped")], check=True)
    out = {}
    for i, co in enumerate(_gfx950_code_objects(fat.read_bytes())):
        elf = tmp / f"co{i}.elf"
        elf.write_bytes(co)
        text = subprocess.run([objdump, "-d", str(elf)], check=True, capture_output=True, text=True).stdout
        funcs = {s: v for s, v in parse_disasm(text).items() if _SYM.search(s)}
        if not funcs:
            continue
        md = kernel_metadata(subprocess.run([readelf, "--notes", str(elf)], check=True, capture_output=True, text=True).stdout)
        for sym, insts in funcs.items():
            out[int(_SYM.search(sym).group(1))] = (insts, md[sym])
    return out


def test_k_iterate_xr_instances_and_budget(xr_kernels, capsys):
    assert sorted(xr_kernels) == list(range(1, 8)), sorted(xr_kernels)
    report = []
    for mh in sorted(xr_kernels):
        insts, md = xr_kernels[mh]
        assert md["vgpr_count"] <= VGPR_BUDGET, (mh, md)
        assert md["agpr_count"] == 0, (mh, md)
        assert md["sgpr_spill_count"] == 0 and md["vgpr_spill_count"] == 0, (mh, md)
        assert md["private_segment_fixed_size"] == 0, (mh, md)
        assert not any(mn.startswith("scratch_") for _, mn, _ in insts), mh
        report.append(f"<{mh}> {md['vgpr_count']} VGPRs, {insts[-1][0] + 4 - insts[0][0]} B")
    insts, _ = xr_kernels[7]
    code = insts[-1][0] + 4 - insts[0][0]
    assert code <= CODE_BYTES_MAX, code
    with capsys.disabled():
        print("\nk_iterate_xr: " + "; ".join(report))


def test_k_iterate_xr_carry_wait_is_covered(xr_kernels, capsys):
    wait = int(re.search(r's_waitcnt vmcnt\((\d+)\)" : "\+v"\(g0\)', open(X_SRC).read()).group(1))
    report = []
    for mh in sorted(xr_kernels):
        counts = counted_waits(xr_kernels[mh][0], wait)   # raises where a path uses the carry registers too early
        assert len(counts) >= 2, f"k_iterate_xr<{mh}>: {len(counts)} carry-load pairs retired by vmcnt({wait})"
        assert min(counts) >= wait, (mh, counts)
        report.append(f"<{mh}>: {len(counts)} sites, min {min(counts)}")
    with capsys.disabled():
        print(f"\nk_iterate_xr carry waits vmcnt({wait}): " + "; ".join(report))
