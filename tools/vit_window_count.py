"""VALU instructions per unrolled trellis window of a Viterbi kernel, from hipcc's device assembly:
    hipcc --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off --cuda-device-only -S -o new.s gr_dvbt_amd/csrc/dvbt_hip.hip
    python tools/vit_window_count.py new.s _ZN4dvbt15viterbi3_kernelILi24ELi72ELi1E
The rule: a window is 8 add-compare-select steps of two registers plus the window end's key = 17 v_pk_max_i16, so a basic block (a run of instructions between labels and
branches) that holds n x 17 of them is n windows.  Per such block: its windows, whether traceback hops ride along (it reads path bytes: ds_read_u8), VALU per window and the
opcode histogram.  windows() is what tests/test_viterbi_isa_budget.py asserts on."""
import re
import sys
from collections import Counter


def windows(asm, prefix):
    """[(kernel, first line of the block, windows, has hops, Counter of VALU opcodes, the block's instructions)]"""
    out = []
    for m in re.finditer(r'^(%s\S*):[^\n]*\n(.*?)\.Lfunc_end' % re.escape(prefix), asm, re.S | re.M):
        block, start = [], 0
        for i, l in enumerate(m.group(2).split('\n') + ['.Lend:']):
            l = re.sub(r'\s*;.*$', '', l.strip())
            if l and not re.match(r'\.?\w+:$', l):
                block.append(l)
            if block and (re.match(r'\.?\w+:$', l) or l.startswith(('s_cbranch', 's_branch', 's_endpgm'))):
                n = sum(x.startswith('v_pk_max_i16') for x in block)
                if n and n % 17 == 0:
                    out.append((m.group(1), start, n // 17, any(x.startswith('ds_read_u8') for x in block), Counter(x.split()[0] for x in block if x.startswith('v_')), block))
                block, start = [], i + 1
    return out


if __name__ == "__main__":
    for name, line, n, hops, ops, _ in windows(open(sys.argv[1]).read(), sys.argv[2]):
        print(f"{name[:48]} +{line}: {n} windows{' with hops' if hops else ''}, {sum(ops.values()) / n:.1f} VALU per window", dict(ops.most_common()))
