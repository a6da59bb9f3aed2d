"""Build-time check of the exact polynomial expansion's register budget (no GPU needed).

k_polyexp_rs<N, HET, U8> runs 512-thread workgroups (8 waves, 2 per SIMD) with 40 KiB of LDS, so at most 4 workgroups
fit on a CU (160 KiB).  It reaches those 4 (8 waves per SIMD) only while every wave fits 64 VGPRs and 80 SGPRs
(MI355X: waves per SIMD = min(512 / vgpr granule, 800 / (ceil(sgpr / 16) * 16 + 16))); at the 82 VGPRs the kernel once
needed, 2 workgroups fitted.  This module reads the gfx950 code object inside the built libnsof.so and holds every
instance to that budget, so that an edit cannot take the occupancy back without failing here.  The radii above 7 keep
their scalar taps in registers over 80 SGPRs (7 waves per SIMD, 3 workgroups per CU); their scalar spills (to VGPR lanes)
must not grow beyond what they were before the budget was set."""
import os
import re
import subprocess

import pytest

from test_codeobj_waits import _gfx950_code_objects, _llvm_tool

LDS_PER_CU = 160 * 1024
SGPR_SPILL_CAP = {8: 8, 9: 14, 10: 19}   # N > 7: scalar spills of the kernel before the budget (largest instance)


def parse_kernel_metadata(notes):
    """llvm-readelf --notes text -> {kernel name: {field: int or str}} of the AMDGPU metadata's kernel list."""
    out = {}
    for chunk in re.split(r"\n  - ", notes):
        m = re.search(r"^\s*\.name:\s+(\S+)\s*$", chunk, re.M)
        if not m:
            continue
        fields = {}
        for key, val in re.findall(r"^\s*\.([a-z_]+):\s+(\S+)\s*$", chunk, re.M):
            fields.setdefault(key, int(val) if val.isdigit() else val)
        out[m.group(1)] = fields
    return out


def test_parse_kernel_metadata():
    text = ("amdhsa.kernels:\n  - .agpr_count:     0\n    .args:\n      - .size:           8\n"
            "    .name:           _Zk_a\n    .sgpr_count:     78\n    .vgpr_count:     46\n    .vgpr_spill_count: 0\n"
            "  - .agpr_count:     0\n    .name:           _Zk_b\n    .vgpr_count:     82\n")
    md = parse_kernel_metadata(text)
    assert md["_Zk_a"]["vgpr_count"] == 46 and md["_Zk_a"]["sgpr_count"] == 78
    assert md["_Zk_b"]["vgpr_count"] == 82 and "sgpr_count" not in md["_Zk_b"]


def test_k_polyexp_rs_register_budget(nsof_lib, tmp_path):
    objcopy, readelf = _llvm_tool("llvm-objcopy"), _llvm_tool("llvm-readelf")
    if not (objcopy and readelf):
        pytest.skip("the ROCm LLVM tools (llvm-objcopy, llvm-readelf) are not installed")
    so = os.path.join(os.path.dirname(nsof_lib.__file__), "libnsof.so")
    fat = tmp_path / "fatbin"
    subprocess.run([objcopy, f"--dump-section=.hip_fatbin={fat}", so, str(tmp_path / "stripped")], check=True)
    cos = _gfx950_code_objects(fat.read_bytes())
    assert cos, "no gfx950 code object in libnsof.so"
    kernels = {}
    for i, co in enumerate(cos):
        elf = tmp_path / f"co{i}.elf"
        elf.write_bytes(co)
        notes = subprocess.run([readelf, "--notes", str(elf)], check=True, capture_output=True, text=True).stdout
        for name, md in parse_kernel_metadata(notes).items():
            m = re.search(r"k_polyexp_rsILi(\d+)ELb([01])ELb([01])E", name)
            if m:
                kernels[(int(m.group(1)), m.group(2) == "1", m.group(3) == "1")] = md
    assert set(kernels) == {(n, het, u8) for n in range(1, 11) for het in (False, True) for u8 in (False, True)}, \
        sorted(kernels)
    bad = []
    for (n, het, u8), md in sorted(kernels.items()):
        tag = f"k_polyexp_rs<{n}, {het}, {u8}>: {md}"
        if md["vgpr_count"] > 64 or md["vgpr_spill_count"] or md.get("agpr_count", 0):
            bad.append(tag)
        if md["private_segment_fixed_size"] or md["group_segment_fixed_size"] * 4 > LDS_PER_CU:
            bad.append(tag)
        if n <= 7 and (md["sgpr_count"] > 80 or md["sgpr_spill_count"] > 31):
            bad.append(tag)
        if n > 7 and md["sgpr_spill_count"] > SGPR_SPILL_CAP[n]:
            bad.append(tag)
    assert not bad, "over the register budget:\n" + "\n".join(bad)
