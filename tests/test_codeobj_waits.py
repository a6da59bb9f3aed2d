"""Build-time check of k_iterate_x's counted carry wait (no GPU needed).

x_remainder_loop (farneback_iterate_x.hip) fetches the left neighbour's carries with two hand-written loads
``global_load_dwordx2 .. sc1`` / ``.. offset:8 sc1`` and waits for them with ``s_waitcnt vmcnt(9)``, counting on the
compiler to place at least 9 vector-memory instructions between the loads and that wait.  If it ever places fewer, the
wait lets the registers be read before the loads have returned: a stale carry of the previous step still carries a
valid epoch tag, and the flow is silently wrong.  This module disassembles the gfx950 code object inside the built
libnsof.so and checks every instantiation k_iterate_x<MH, HET> on every control-flow path.

Counting rule (CDNA / gfx9 family, MI355X_MICROARCH "s_waitcnt"): ``s_waitcnt vmcnt(N)`` waits until all but the wave's
N youngest vector-memory operations are done.  Loads, stores and atomics of the ``global_``, ``buffer_`` and
``scratch_`` kinds all count in vmcnt (gfx9 has no separate store counter) and retire in issue order, so the carry
loads are done once N younger ones of those have been issued.  ``flat_`` operations also count but may retire out of
order, and cache-control instructions (``buffer_inv``, ``buffer_wbl2``) are not loads: neither is counted as a younger
operation here (the safe side).  A wait retires the carries when its N is at most the number of younger operations
issued on the path; the carry registers must not be read or written before some wait has retired them.  A path that
reaches the next pair of carry loads first ends there: that pair is a site of its own, and the wait that retires it
retires the older pair as well.
"""
import os
import re
import shutil
import struct
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
X_SRC = os.path.join(ROOT, "neuromorphic-spatiotemporal-optical-flow_amd", "csrc", "farneback_iterate_x.hip")

_ADDR = re.compile(r"//\s*([0-9A-Fa-f]+):")
_VREG = re.compile(r"\bv(?:(\d+)|\[(\d+):(\d+)\])")
_VMCNT = re.compile(r"vmcnt\((\d+)\)")
_VMEM = re.compile(r"^(global|buffer|scratch)_(load|store|atomic)")
_CARRY = re.compile(r"^global_load_dwordx2\s+(v\[\d+:\d+\]),\s*(v\[\d+:\d+\]),\s*off(\s+offset:8)?\s+sc1\s*$")
_MANY = 1 << 20   # "retired before any counted wait": more younger operations than any vmcnt can name


def parse_disasm(text):
    """llvm-objdump -d text -> {symbol: [(address, mnemonic, operands)]}."""
    funcs, cur = {}, None
    for line in text.splitlines():
        m = re.match(r"^[0-9a-fA-F]+ <(.+)>:\s*$", line)
        if m:
            cur = funcs.setdefault(m.group(1), [])
            continue
        if cur is None or not line.startswith(("\t", " ")):
            continue
        a = _ADDR.search(line)
        body = line.split("//", 1)[0].strip()
        if not a or not body:
            continue
        mn, _, ops = body.partition(" ")
        cur.append((int(a.group(1), 16), mn, ops.strip()))
    return funcs


def _vregs(ops):
    out = set()
    for one, lo, hi in _VREG.findall(ops):
        out.update([int(one)] if one else range(int(lo), int(hi) + 1))
    return out


def _successors(insts, i, at):
    addr, mn, ops = insts[i]
    nxt = [i + 1] if i + 1 < len(insts) else []
    if mn == "s_endpgm":
        return []
    if mn in ("s_setpc_b64", "s_swappc_b64"):
        raise ValueError(f"indirect branch at {addr:#x}: control flow cannot be followed")
    if mn == "s_branch" or mn.startswith("s_cbranch_"):
        imm = int(ops.split()[0], 0)
        imm = imm - 65536 if imm >= 32768 else imm
        tgt = addr + 4 + 4 * imm
        if tgt not in at:
            raise ValueError(f"branch at {addr:#x} to {tgt:#x} is not an instruction start")
        return [at[tgt]] if mn == "s_branch" else [at[tgt]] + nxt
    return nxt


def carry_wait_sites(insts):
    """Every pair of carry loads in one kernel -> (index of the pair's first load, wait N, fewest younger vector-memory
    operations on any path from the pair to the wait that retires it).  Raises AssertionError when some path reads or
    overwrites the carry registers before a wait has retired the loads."""
    at = {a: i for i, (a, _, _) in enumerate(insts)}
    sites = []
    for i in range(len(insts) - 1):
        m0, m1 = _CARRY.match(f"{insts[i][1]} {insts[i][2]}"), _CARRY.match(f"{insts[i + 1][1]} {insts[i + 1][2]}")
        if not (m0 and m1 and not m0.group(3) and m1.group(3) and m0.group(2) == m1.group(2)):
            continue
        regs = _vregs(m0.group(1)) | _vregs(m1.group(1))
        best = {}                       # instruction index -> fewest younger operations any path brings there
        work = [(s, 0) for s in _successors(insts, i + 1, at)]
        retired = {}                    # wait N -> fewest younger operations among the paths it retired
        while work:
            j, n = work.pop()
            while True:
                if best.get(j, _MANY + 1) <= n:
                    break
                best[j] = n
                _, mn, ops = insts[j]
                if mn == "s_waitcnt" and _VMCNT.search(ops):
                    k = int(_VMCNT.search(ops).group(1))
                    if k <= n:
                        retired[k] = min(retired.get(k, _MANY), n)
                        break
                elif _CARRY.match(f"{mn} {ops}"):
                    break               # the next fetch: its own site, and its wait retires these older loads too
                elif mn != "s_waitcnt" and regs & _vregs(ops):
                    raise AssertionError(f"carry loads at {insts[i][0]:#x}: `{mn} {ops}` at {insts[j][0]:#x} uses their "
                                         f"registers with only {n} younger vector-memory operations issued and no wait "
                                         f"that retires them")
                if _VMEM.match(mn):
                    n = min(n + 1, _MANY)
                succ = _successors(insts, j, at)
                if not succ:
                    break
                work.extend((s, n) for s in succ[1:])
                j = succ[0]
        for k, n in retired.items():
            sites.append((i, k, n))
    return sites


def counted_waits(insts, count):
    """The carry sites of one kernel retired by the counted wait vmcnt(count): [fewest younger operations per site]."""
    return [n for _, k, n in carry_wait_sites(insts) if k == count]


def expected_instantiations(src_text):
    """(MH, HET) of every k_iterate_x the launchers instantiate: each nsof_with_int<LO, HI>(winsize / 2, ..) whose lambda
    calls launch_x<MH, HET> with the constant it is handed makes LO..HI for that HET."""
    calls = re.findall(r"nsof_with_int<\s*(\d+)\s*,\s*(\d+)\s*>\(winsize / 2, \[&\]\(auto mh\) \{\s*"
                       r"rc = launch_x<decltype\(mh\)::value, (true|false)>\(", src_text)
    assert len(calls) == len(re.findall(r"\blaunch_x<", src_text)), "a launch_x<..> call this parser does not know"
    return {(m, het == "true") for lo, hi, het in calls for m in range(int(lo), int(hi) + 1)}


# ---- synthetic snippets: the checker bites without touching the kernel ----------------------------------------------
def _snippet(n_loads, branch=False):
    lines = ["0000000000001000 <_ZN12_GLOBAL__N_111k_iterate_xILi3ELb0EEEvv>:"]
    addr = 0x1000

    def emit(s):
        nonlocal addr
        lines.append(f"\t{s:<58} // {addr:012X}: 00000000")
        addr += 8 if s.startswith(("global_", "v_add_u32_e64")) else 4

    emit("s_and_saveexec_b64 s[6:7], s[14:15]")
    emit("global_load_dwordx2 v[78:79], v[46:47], off sc1")
    emit("global_load_dwordx2 v[76:77], v[46:47], off offset:8 sc1")
    emit("s_or_b64 exec, exec, s[6:7]")
    emit("s_waitcnt vmcnt(9)")                         # a compiler wait for OLDER loads: does not retire the carries
    for k in range(n_loads):
        if branch and k == 4:                           # skip two loads on one path: s_cbranch_scc1 over them
            emit("s_cbranch_scc1 4")
        emit(f"global_load_dwordx4 v[{10 + 4 * k}:{13 + 4 * k}], v6, s[26:27]")
    emit("s_waitcnt vmcnt(9)")
    emit("v_cmp_eq_u32_e32 vcc, s8, v79")
    emit("s_endpgm")
    return "\n".join(lines) + "\n"


def test_checker_accepts_nine_younger_loads():
    (insts,) = parse_disasm(_snippet(9)).values()
    assert counted_waits(insts, 9) == [9]


def test_checker_rejects_eight_younger_loads():
    (insts,) = parse_disasm(_snippet(8)).values()
    with pytest.raises(AssertionError, match="uses their registers with only 8 younger"):
        carry_wait_sites(insts)


def test_checker_walks_branches():
    """Ten loads in the text, but a branch skips two of them: the short path has 8 and must be rejected."""
    (insts,) = parse_disasm(_snippet(10, branch=True)).values()
    with pytest.raises(AssertionError, match="only 8 younger"):
        carry_wait_sites(insts)


def test_expected_instantiations_from_source():
    with open(X_SRC) as f:
        exp = expected_instantiations(f.read())
    assert exp == {(m, h) for m in range(1, 8) for h in (False, True)}


# ---- the real code object ----------------------------------------------------------------------------------------------
def _llvm_tool(name):
    for d in (os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "llvm", "bin"), "/opt/rocm/llvm/bin"):
        p = os.path.join(d, name)
        if os.access(p, os.X_OK):
            return p
    return shutil.which(name)


def _gfx950_code_objects(fatbin):
    """The gfx950 device ELFs of a .hip_fatbin section (clang offload bundles, one per translation unit)."""
    magic = b"__CLANG_OFFLOAD_BUNDLE__"
    out, pos = [], fatbin.find(magic)
    while pos >= 0:
        (n,) = struct.unpack_from("<Q", fatbin, pos + len(magic))
        p = pos + len(magic) + 8
        for _ in range(n):
            off, size, tlen = struct.unpack_from("<QQQ", fatbin, p)
            triple = fatbin[p + 24:p + 24 + tlen].decode()
            p += 24 + tlen
            if triple.endswith("gfx950") and size:
                out.append(fatbin[pos + off:pos + off + size])
        pos = fatbin.find(magic, pos + 1)
    return out


def test_k_iterate_x_carry_wait_is_covered(nsof_lib, tmp_path, capsys):
    objcopy, objdump = _llvm_tool("llvm-objcopy"), _llvm_tool("llvm-objdump")
    if not (objcopy and objdump):
        pytest.skip("the ROCm LLVM tools (llvm-objcopy, llvm-objdump) are not installed")
    so = os.path.join(os.path.dirname(nsof_lib.__file__), "libnsof.so")
    fat = tmp_path / "fatbin"
    subprocess.run([objcopy, f"--dump-section=.hip_fatbin={fat}", so, str(tmp_path / "stripped")], check=True)
    cos = _gfx950_code_objects(fat.read_bytes())
    assert cos, "no gfx950 code object in libnsof.so"
    kernels = {}
    for i, co in enumerate(cos):
        elf = tmp_path / f"co{i}.elf"
        elf.write_bytes(co)
        text = subprocess.run([objdump, "-d", str(elf)], check=True, capture_output=True, text=True).stdout
        for sym, insts in parse_disasm(text).items():
            m = re.search(r"k_iterate_xILi(\d+)ELb([01])E", sym)
            if m:
                kernels[(int(m.group(1)), m.group(2) == "1")] = insts
    with open(X_SRC) as f:
        expected = expected_instantiations(f.read())
    assert set(kernels) == expected, f"instantiations found {sorted(kernels)}, the launchers make {sorted(expected)}"
    wait = int(re.search(r's_waitcnt vmcnt\((\d+)\)" : "\+v"\(g0\)', open(X_SRC).read()).group(1))
    # at least the prologue's fetch and the window loop's retired by the counted wait (the compiler may peel a window
    # more, and may retire a peeled fetch with a wait of its own); every other pair checked as well, by carry_wait_sites
    report, total = [], 0
    for key in sorted(kernels):
        counts = counted_waits(kernels[key], wait)
        assert len(counts) >= 2, f"k_iterate_x<{key[0]}, {key[1]}>: {len(counts)} carry-load pairs retired by vmcnt({wait})"
        assert min(counts) >= wait
        total += len(counts)
        report.append(f"<{key[0]},{int(key[1])}>: {len(counts)} sites, min {min(counts)}")
    with capsys.disabled():   # the figures belong in the suite's output
        print(f"\nk_iterate_x carry waits vmcnt({wait}): {total} sites verified in {len(kernels)} instantiations; "
              + "; ".join(report))
