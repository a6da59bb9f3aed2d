#!/usr/bin/env python3
"""Instruction mix of the main loop of a kernel in a device assembly listing (hipcc -S --cuda-device-only).
Usage: isa_mix.py file.s substring-of-mangled-name ...   (prints whole-kernel and hottest-loop counts)
       isa_mix.py --loops libnsof.so [MH [HET]]          (k_iterate_x<MH, HET>, default <7, 0>, out of the built library:
                                                          per-WINDOW counts of the producer, remainder and consumer loops,
                                                          a window = one s_barrier of the loop; the loop finder is the one
                                                          tests/test_codeobj_iterate_stream.py asserts with)"""
import os
import re
import subprocess
import sys
import tempfile
from collections import Counter


def classify(i):
    if i.startswith('v_') and 'f64' in i:
        return 'valu_f64'
    if i.startswith('v_pk'):
        return 'valu_pk'
    if i.startswith('v_'):
        return 'valu'
    if i.startswith('ds_'):
        return 'lds'
    if i.startswith(('global_', 'buffer_', 'flat_', 'scratch_')):
        return 'vmem'
    if i.startswith('s_'):
        return 'salu'
    return 'other'


def per_loop(so, mh, het):
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'tests'))
    from test_codeobj_iterate_stream import merged_loops
    from test_codeobj_waits import _gfx950_code_objects, _llvm_tool, parse_disasm
    with tempfile.TemporaryDirectory() as d:
        fat = os.path.join(d, 'fatbin')
        subprocess.run([_llvm_tool('llvm-objcopy'), f'--dump-section=.hip_fatbin={fat}', so, os.path.join(d, 'rest')], check=True)
        insts = None
        for i, co in enumerate(_gfx950_code_objects(open(fat, 'rb').read())):
            elf = os.path.join(d, f'co{i}.elf')
            open(elf, 'wb').write(co)
            text = subprocess.run([_llvm_tool('llvm-objdump'), '-d', elf], check=True, capture_output=True, text=True).stdout
            for sym, v in parse_disasm(text).items():
                if f'k_iterate_xILi{mh}ELb{het}E' in sym:
                    insts = v
    print(f'k_iterate_x<{mh},{het}>: {insts[-1][0] + 4 - insts[0][0]} bytes of code')
    roles = (('producer', lambda s: s['windows'] and s['x4'] and not s['f64']),
             ('remainder', lambda s: s['windows'] and s['x4'] and s['f64']),
             ('consumer', lambda s: s['windows'] and not s['x4'] and s['f64'] > 100 and s['lds'] > 60))
    for role, want in roles:
        for st in merged_loops(insts, want):
            w = st['windows']
            print(f"  {role:9s} {w} windows per trip; per window: VALU {st['valu'] / w:6.1f} (f64 {st['f64'] / w:5.1f})  SALU {st['salu'] / w:6.1f}"
                  f"  LDS {st['lds'] / w:5.1f}  VMEM {st['vmem'] / w:5.1f}  lowest vmcnt waited for {min(st['vmcnt']) if st['vmcnt'] else '-'}")


def main():
    if sys.argv[1] == '--loops':
        return per_loop(sys.argv[2], int(sys.argv[3]) if len(sys.argv) > 3 else 7, int(sys.argv[4]) if len(sys.argv) > 4 else 0)
    lines = open(sys.argv[1]).read().split('\n')
    for sub in sys.argv[2:]:
        start = next(k for k, l in enumerate(lines) if l.startswith('_Z') and sub in l and l.rstrip().endswith(tuple([':'])) or (l.startswith('_Z') and sub in l and ': ' in l))
        end = next(k for k in range(start, len(lines)) if 's_endpgm' in lines[k])
        body = lines[start + 1:end]
        labels, ins = {}, []
        for l in body:
            t = l.strip()
            if not t or t.startswith((';', '.s', '.p', '.a', '.t', '.g', '.w', '.c')):
                continue
            if t.endswith(':') or re.match(r'^\.LBB\d+_\d+:', t):
                labels[t.split(':')[0]] = len(ins)
                continue
            ins.append(t)
        total = Counter(classify(i.split()[0]) for i in ins)
        # loops = backward branches; report the largest-trip candidate = the longest backward span
        loops = []
        for k, i in enumerate(ins):
            m = re.match(r's_cbranch_\w+\s+(\.LBB\d+_\d+)|s_branch\s+(\.LBB\d+_\d+)', i)
            if m:
                tgt = m.group(1) or m.group(2)
                if tgt in labels and labels[tgt] <= k:
                    loops.append((k - labels[tgt], labels[tgt], k))
        print(sub, 'total', len(ins), dict(total))
        for span, a, b in sorted(loops, reverse=True)[:8]:
            c = Counter(classify(i.split()[0]) for i in ins[a:b + 1])
            print('   loop span', span, dict(c))


if __name__ == '__main__':
    main()
