#!/usr/bin/env python3
"""Static instruction counts per basic block of one kernel in a gfx950 assembly file (hipcc -S --cuda-device-only).

usage: isa_block_counts.py FILE.s KERNEL_SUBSTRING [min_mfma]

Prints, for every basic block of the first kernel whose (mangled) name contains KERNEL_SUBSTRING that holds at least
min_mfma matrix instructions or at least one v_rsq_f64: MFMA, VALU (v_* without MFMA), v_add_u32, v_mov_b32, v_alignbyte,
v_cndmask, v_cmp, ds_read_b32 / ds_read2_b32 / other ds_read, v_rsq_f64 - and the kernel's totals and register counts.
Blocks are named by their label (.LBBn_m) or, where control only falls into them, by the compiler's comment (bb.m).
The loops of the PM kernels are fully unrolled, so a block is a loop: the winner's single item is the block with 38 MFMAs at
side 34 (76 with the all-ones operand), the sweep's single item the one with 78 + strip, and so on."""
import re
import sys


def main():
    path, sub = sys.argv[1], sys.argv[2]
    min_mfma = int(sys.argv[3]) if len(sys.argv) > 3 else 16
    name, blocks, cur, meta = None, [], None, {}
    for line in open(path):
        t = line.strip()
        if name is None:
            m = re.match(r'^(\S+):\s', line)
            if m and sub in m.group(1) and not t.startswith('.'):
                name = m.group(1)
                cur = ['entry', []]
                blocks.append(cur)
            continue
        if t.startswith('.Lfunc_end'):
            break
        m = re.match(r'^(\.LBB\S+):', t)
        if m:
            cur = [m.group(1), []]
            blocks.append(cur)
            continue
        m = re.match(r'^; %(bb\.\d+):', t)                             # a block entered by falling through only
        if m:
            cur = [m.group(1), []]
            blocks.append(cur)
            continue
        if not t or t.startswith((';', '.', '//')):
            continue
        cur[1].append(t.split()[0])
    if name is None:
        sys.exit('no kernel matching %r' % sub)
    for line in open(path):
        m = re.match(r'\s*[;.]\s*\.?(vgpr_count|vgpr_spill_count|sgpr_spill_count|private_segment_fixed_size|NumVgprs|ScratchSize|Occupancy):?\s*(\d+)', line)
        if m and meta.get('_in'):
            meta.setdefault(m.group(1), m.group(2))
        if name in line and '.name:' in line:
            meta['_in'] = True
        elif '.name:' in line:
            meta['_in'] = False
    cols = ['mfma', 'valu', 'v_add_u32', 'v_mov_b32', 'v_alignbyte', 'v_cndmask', 'v_cmp', 'ds_read_b32', 'ds_read2_b32', 'ds_read_other', 'v_rsq_f64']

    def count(ops):
        c = dict.fromkeys(cols, 0)
        for o in ops:
            if 'mfma' in o:
                c['mfma'] += 1
            elif o.startswith('v_'):
                c['valu'] += 1
                for k in ('v_add_u32', 'v_mov_b32', 'v_alignbyte', 'v_cndmask', 'v_cmp', 'v_rsq_f64'):
                    if o.startswith(k):
                        c[k] += 1
            elif o.startswith('ds_read') or o.startswith('ds_load'):
                k = 'ds_read_b32' if o in ('ds_read_b32', 'ds_load_b32') else 'ds_read2_b32' if o in ('ds_read2_b32', 'ds_load_2addr_b32') else 'ds_read_other'
                c[k] += 1
        return c
    print(name)
    print('%-14s' % 'block' + ''.join('%14s' % k for k in cols))
    tot = dict.fromkeys(cols, 0)
    for label, ops in blocks:
        c = count(ops)
        for k in cols:
            tot[k] += c[k]
        if c['mfma'] >= min_mfma or c['v_rsq_f64'] >= 1:
            print('%-14s' % label[-14:] + ''.join('%14d' % c[k] for k in cols))
    print('%-14s' % 'kernel total' + ''.join('%14d' % tot[k] for k in cols))
    print({k: v for k, v in meta.items() if k != '_in'})


if __name__ == '__main__':
    main()
