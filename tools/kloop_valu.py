#!/usr/bin/env python3
"""Instruction mix of the matrix blocks of a `hipcc -S --cuda-device-only` listing.

For every kernel whose mangled name contains FILTER: the scratch size and register counts of its metadata, then one line per basic block
that holds at least MIN_MFMA matrix instructions: MFMA, VALU (everything `v_*` that is no MFMA), the four opcodes of the bf16x6 operand split
(v_cvt_pk_bf16_f32, v_lshlrev_b32, v_and_b32, v_sub_f32), what is left of the VALU ("other": address arithmetic, lane moves, masks), the
v_readlane / v_writelane among them, LDS, VMEM and scratch instructions.  A basic block starts at a label and ends behind a branch.
A line `a..b` sums the blocks of a loop (a backward branch from block b to the label of block a) that holds no other loop: a steady k-loop
iteration is such a line.

usage: python tools/kloop_valu.py listing.s [FILTER] [MIN_MFMA=48]
"""
import re
import sys
from collections import Counter

SPLIT = ('v_cvt_pk_bf16_f32', 'v_lshlrev_b32', 'v_and_b32', 'v_sub_f32')


def kernels(path):
    """{mangled name: [[instruction, ...] per basic block]}, {mangled name: [(first block, last block) per loop]}"""
    out, loops, cur, labels = {}, {}, None, {}
    for line in open(path):
        m = re.match(r'^(_Z\w+):', line)
        if m:
            cur = out.setdefault(m.group(1), [[]])
            lp = loops.setdefault(m.group(1), [])
            labels = {}
            continue
        if line.startswith('.Lfunc_end'):
            cur = None
        if cur is None:
            continue
        t = line.split(';')[0].strip()
        if not t:
            continue
        if re.match(r'^\.LBB\d+_\d+:', t):
            cur.append([])
            labels[t[:-1]] = len(cur) - 1
        elif not t.startswith('.'):
            cur[-1].append(t.split()[0])
            if t.startswith(('s_cbranch', 's_branch')):
                if t.split()[-1] in labels:
                    lp.append((labels[t.split()[-1]], len(cur) - 1))
                cur.append([])
    return out, loops


def metadata(path):
    txt = open(path).read()
    md = {}
    for m in re.finditer(r'\.name:\s+(\S+)\n(.*?)\.wavefront_size', txt, re.S):
        g = lambda k: (re.search(r'\.%s:\s+(\d+)' % k, m.group(2)) or [0, '?'])[1]   # noqa: E731
        md[m.group(1)] = {k: g(k) for k in ('vgpr_count', 'agpr_count', 'sgpr_count', 'vgpr_spill_count', 'sgpr_spill_count',
                                            'private_segment_fixed_size')}
    return md


def mix(block):
    c = Counter()
    for op in block:
        if op.startswith('v_mfma'):
            c['mfma'] += 1
        elif op.startswith('v_'):
            c['valu'] += 1
            if op.startswith(SPLIT):
                c['split'] += 1
            if op.startswith(('v_readlane', 'v_writelane', 'v_readfirstlane')):
                c['lane'] += 1
        elif op.startswith('ds_'):
            c['lds'] += 1
        elif op.startswith('scratch_'):
            c['scratch'] += 1
        elif op.startswith(('global_', 'flat_', 'buffer_')):
            c['vmem'] += 1
    c['other'] = c['valu'] - c['split']
    return c


def main():
    path = sys.argv[1]
    flt = sys.argv[2] if len(sys.argv) > 2 else ''
    min_mfma = int(sys.argv[3]) if len(sys.argv) > 3 else 48
    md = metadata(path)
    ks, loops = kernels(path)
    for name, blocks in ks.items():
        if flt not in name:
            continue
        m = md.get(name, {})
        print('%s\n  scratch %s  vgpr %s  agpr %s  sgpr %s  vgpr_spill %s  sgpr_spill %s' % (
            name, m.get('private_segment_fixed_size', '?'), m.get('vgpr_count', '?'), m.get('agpr_count', '?'), m.get('sgpr_count', '?'),
            m.get('vgpr_spill_count', '?'), m.get('sgpr_spill_count', '?')))
        print('  %5s %5s %5s %5s %5s %5s %4s %4s %7s' % ('block', 'mfma', 'valu', 'split', 'other', 'lane', 'lds', 'vmem', 'scratch'))
        for i, b in enumerate(blocks):
            c = mix(b)
            if c['mfma'] >= min_mfma:
                print('  %5d %5d %5d %5d %5d %5d %4d %4d %7d' % (i, c['mfma'], c['valu'], c['split'], c['other'], c['lane'], c['lds'],
                                                                   c['vmem'], c['scratch']))
        for a, b in loops[name]:
            if any((a2, b2) != (a, b) and a <= a2 and b2 <= b for a2, b2 in loops[name]):
                continue
            c = mix([op for blk in blocks[a:b + 1] for op in blk])
            if c['mfma'] >= min_mfma:
                print('  %5s %5d %5d %5d %5d %5d %4d %4d %7d' % ('%d..%d' % (a, b), c['mfma'], c['valu'], c['split'], c['other'], c['lane'],
                                                                   c['lds'], c['vmem'], c['scratch']))


if __name__ == '__main__':
    main()
