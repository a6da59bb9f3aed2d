"""Build-time check of k_iterate_x's instruction streams and register budget (no GPU needed).

k_iterate_x is bound by instruction issue on the SIMDs that hold a consumer wave and two producer waves (DESIGN.md
section 5.1), so the length of the producers' steady-state loop is performance, and it is decided by the compiler: this
module disassembles the gfx950 code object inside the built libnsof.so (helpers of test_codeobj_waits.py) and holds

  * every k_iterate_x<MH, HET> to its budget: at most 168 VGPRs (three waves per SIMD: 512 / 3 at the granule of 8), no
    AGPRs, no spilled register, no scratch, and the LDS of one workgroup per CU as before;
  * the full producer waves' loop of MH = 7 to a ceiling of VALU instructions per window (a window = four image rows =
    one barrier of the loop).  The loop is the one that contains s_barrier and global_load_dwordx4 and no f64
    instruction (the remainder wave solves, the consumers sum in double).  With floor_f's range-check branch in the
    sample coordinates the count was 272.5 and 270.5 per window in the loops of the two row groups (545 and 541 in two
    windows); with floorf it is 242.5 and 240.5 (485 and 481).  Ceiling: 242.5 + 2 %;
  * that loop to be free of floor_f's range-check sequence (nsof_internal.h): no v_subbrev_co_u32;
  * that loop to be ONE loop with ONE backward branch.  An exit between its two windows is laid out as a branch back to
    the loop's latch, and the compiler's wait insertion then assumes at the head what holds after the first window --
    that window's own loads in flight: vmcnt(18), (9), (0) at the head of every trip.  x_producer_loop has one exit, at
    the bottom, and one wait of that kind is left: vmcnt(0) for the flow registers' copies (a form that rotates four
    flow registers has neither copies nor that wait, 230 VALU per window, and measured no faster: DESIGN.md 5.1).
"""
import os
import re
import subprocess

import pytest

from test_codeobj_waits import X_SRC, _gfx950_code_objects, _llvm_tool, expected_instantiations, parse_disasm

VGPR_BUDGET = 168
LDS_BYTES_MAX = 160 * 1024          # one workgroup per CU
CODE_BYTES_MAX = 64 * 1024          # k_iterate_x<7, false>: the instruction cache two CUs share
PARENT_VALU_PER_WINDOW = 272.5
VALU_PER_WINDOW_CEILING = 242.5 * 1.02
LOADS_PER_WINDOW = 18


def back_edge_ranges(insts):
    """[(first, last)] instruction index ranges closed by a backward branch."""
    at = {a: i for i, (a, _, _) in enumerate(insts)}
    out = []
    for i, (addr, mn, ops) in enumerate(insts):
        if mn == "s_branch" or mn.startswith("s_cbranch_"):
            imm = int(ops.split()[0], 0)
            imm = imm - 65536 if imm >= 32768 else imm
            tgt = addr + 4 + 4 * imm
            if tgt <= addr and tgt in at:
                out.append((at[tgt], i))
    return out


def loop_stats(body):
    mns = [m for _, m, _ in body]
    valu = [m for m in mns if m.startswith("v_")]
    return {
        "valu": len(valu),
        "f64": sum("f64" in m for m in valu),
        "salu": sum(m.startswith("s_") for m in mns),
        "lds": sum(m.startswith("ds_") for m in mns),
        "vmem": sum(m.startswith(("global_", "buffer_", "scratch_")) for m in mns),
        "windows": mns.count("s_barrier"),
        "x4": mns.count("global_load_dwordx4"),
        "subbrev": sum(m.startswith("v_subbrev_co_u32") for m in mns),
        "vmcnt": [int(re.search(r"vmcnt\((\d+)\)", o).group(1)) for _, m, o in body if m == "s_waitcnt" and "vmcnt" in o],
    }


def merged_loops(insts, want):
    """The loops whose body satisfies `want(stats)`: overlapping back-edge ranges (the several latches and exits the
    compiler gives one source loop) merged into one range each.  -> [stats of the merged range, + "back_edges"]."""
    picked = sorted(r for r in back_edge_ranges(insts) if want(loop_stats(insts[r[0]:r[1] + 1])))
    merged = []
    for a, b in picked:
        if merged and a <= merged[-1][1]:
            merged[-1][1] = max(merged[-1][1], b)
            merged[-1][2] += 1
        else:
            merged.append([a, b, 1])
    return [dict(loop_stats(insts[a:b + 1]), back_edges=n) for a, b, n in merged]


def is_full_producer_loop(st):
    return st["windows"] > 0 and st["x4"] > 0 and st["f64"] == 0


def kernel_metadata(notes_text):
    """llvm-readelf --notes -> {kernel symbol: {field: int}} of the amdhsa.kernels metadata."""
    out = {}
    for block in re.split(r"\n\s+- \.agpr_count:", "\n" + notes_text)[1:]:
        block = ".agpr_count:" + block
        name = re.search(r"\.name:\s+(\S+)", block)
        if not name:
            continue
        out[name.group(1)] = {k: int(v) for k, v in re.findall(
            r"\.(agpr_count|vgpr_count|sgpr_spill_count|vgpr_spill_count|private_segment_fixed_size|"
            r"group_segment_fixed_size):\s+(\d+)", block)}
    return out


# ---- synthetic snippet: the loop finder and its counts, without the kernel ---------------------------------------------
def _snippet():
    lines = ["0000000000002000 <_ZN12_GLOBAL__N_111k_iterate_xILi7ELb0EEEvv>:"]
    addr = 0x2000

    def emit(s, size=4):
        nonlocal addr
        lines.append(f"\t{s:<58} // {addr:012X}: 00000000")
        addr += size

    emit("v_mov_b32_e32 v1, 0")
    loop = addr
    for w in range(2):
        emit("s_waitcnt vmcnt(27)")
        emit("v_floor_f32_e32 v2, v3")
        emit("v_sub_f32_e32 v4, v3, v2")
        emit("global_load_dwordx4 v[8:11], v5, s[2:3]", 8)
        emit("s_barrier")
        if w == 0:                                     # a mid-loop exit laid out as a second backward branch
            emit(f"s_cbranch_scc1 {(loop - (addr + 4)) // 4 & 0xffff}")
    emit(f"s_cbranch_scc0 {(loop - (addr + 4)) // 4 & 0xffff}")
    emit("v_add_f64 v[2:3], v[2:3], v[4:5]", 8)
    emit("s_endpgm")
    return "\n".join(lines) + "\n"


def test_loop_finder_merges_latches_and_counts_per_window():
    (insts,) = parse_disasm(_snippet()).values()
    assert len(back_edge_ranges(insts)) == 2
    (st,) = merged_loops(insts, is_full_producer_loop)
    assert (st["windows"], st["valu"], st["x4"], st["f64"], st["vmcnt"], st["back_edges"]) == (2, 4, 2, 0, [27, 27], 2)


def test_metadata_parser():
    text = ("amdhsa.kernels:\n  - .agpr_count:     0\n    .args:\n      - .offset: 0\n    .group_segment_fixed_size: 16\n"
            "    .name:           _Zk1\n    .private_segment_fixed_size: 0\n    .sgpr_spill_count: 0\n    .vgpr_count:     165\n"
            "    .vgpr_spill_count: 2\n  - .agpr_count:     4\n    .name: _Zk2\n    .vgpr_count: 7\n")
    md = kernel_metadata(text)
    assert md["_Zk1"]["vgpr_count"] == 165 and md["_Zk1"]["vgpr_spill_count"] == 2 and md["_Zk2"]["agpr_count"] == 4


# ---- the real code object ----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def x_kernels(nsof_lib, tmp_path_factory):
    """{(MH, HET): (instructions, metadata)} of every k_iterate_x in libnsof.so."""
    objcopy, objdump, readelf = _llvm_tool("llvm-objcopy"), _llvm_tool("llvm-objdump"), _llvm_tool("llvm-readelf")
    if not (objcopy and objdump and readelf):
        pytest.skip("the ROCm LLVM tools (llvm-objcopy, llvm-objdump, llvm-readelf) are not installed")
    tmp = tmp_path_factory.mktemp("codeobj")
    so = os.path.join(os.path.dirname(nsof_lib.__file__), "libnsof.so")
    fat = tmp / "fatbin"
    subprocess.run([objcopy, f"--dump-section=.hip_fatbin={fat}", so, str(tmp / "stripped")], check=True)
    out = {}
    for i, co in enumerate(_gfx950_code_objects(fat.read_bytes())):
        elf = tmp / f"co{i}.elf"
        elf.write_bytes(co)
        text = subprocess.run([objdump, "-d", str(elf)], check=True, capture_output=True, text=True).stdout
        funcs = {s: v for s, v in parse_disasm(text).items() if re.search(r"k_iterate_xILi\d+ELb[01]E", s)}
        if not funcs:
            continue
        md = kernel_metadata(subprocess.run([readelf, "--notes", str(elf)], check=True, capture_output=True, text=True).stdout)
        for sym, insts in funcs.items():
            m = re.search(r"k_iterate_xILi(\d+)ELb([01])E", sym)
            out[(int(m.group(1)), m.group(2) == "1")] = (insts, md[sym])
    with open(X_SRC) as f:
        expected = expected_instantiations(f.read())
    assert set(out) == expected, f"instantiations found {sorted(out)}, the launchers make {sorted(expected)}"
    return out


def test_k_iterate_x_register_budget(x_kernels, capsys):
    report = []
    for key in sorted(x_kernels):
        insts, md = x_kernels[key]
        assert md["vgpr_count"] <= VGPR_BUDGET, (key, md)
        assert md["agpr_count"] == 0, (key, md)
        assert md["sgpr_spill_count"] == 0 and md["vgpr_spill_count"] == 0, (key, md)
        assert md["private_segment_fixed_size"] == 0, (key, md)
        assert md["group_segment_fixed_size"] <= LDS_BYTES_MAX, (key, md)   # static part; the launch adds XGeom::SMEM
        assert not any(mn.startswith("scratch_") for _, mn, _ in insts), key
        report.append(f"<{key[0]},{int(key[1])}> {md['vgpr_count']} VGPRs, {insts[-1][0] + 4 - insts[0][0]} B")
    insts, _ = x_kernels[(7, False)]
    code = insts[-1][0] + 4 - insts[0][0]
    assert code <= CODE_BYTES_MAX, code
    with capsys.disabled():
        print("\nk_iterate_x: " + "; ".join(report))


def test_full_producer_loop_stream(x_kernels, capsys):
    insts, _ = x_kernels[(7, False)]
    loops = merged_loops(insts, is_full_producer_loop)
    assert len(loops) == 2, f"{len(loops)} loops with a barrier, 16-byte loads and no f64: one per row group expected"
    report = []
    for st in loops:
        per_window = st["valu"] / st["windows"]
        report.append(f"{st['valu']} VALU / {st['windows']} windows = {per_window:.2f} (parent {PARENT_VALU_PER_WINDOW}), "
                      f"{st['salu'] / st['windows']:.1f} SALU, {st['vmem'] / st['windows']:.1f} loads, min vmcnt {min(st['vmcnt'])}")
    with capsys.disabled():
        print("\nk_iterate_x<7,false> full producer loops: " + "; ".join(report))
    for st in loops:
        assert st["vmem"] == LOADS_PER_WINDOW * st["windows"], st
        assert st["valu"] / st["windows"] <= VALU_PER_WINDOW_CEILING, st
        assert st["subbrev"] == 0, "floor_f's range-check sequence is back in the producers' loop"
        assert st["back_edges"] == 1, f"{st['back_edges']} backward branches: an exit between the loop's windows is back"
        low = [n for n in st["vmcnt"] if n < LOADS_PER_WINDOW]
        assert low == [0], f"waits for loads of the loop's own window: vmcnt {low} (one vmcnt(0), the flow copies', expected)"
