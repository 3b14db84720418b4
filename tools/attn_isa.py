#!/usr/bin/env python3
"""Static view of the compiled attention kernels (no GPU needed): the compiler's resource report for every attn_kernel
instantiation, and the per-basic-block instruction mix of one of them.

  python tools/attn_isa.py                      # compile csrc/attention.hip (Makefile flags), report <40,2,true,1>
  python tools/attn_isa.py --kernel 80,1,true,2 --src path/to/attention.hip

Blocks that a later branch jumps back to are marked "loop"; "valu" counts every v_ instruction except MFMAs, and the
columns after it break out the ones the softmax is made of."""
import argparse
import os
import re
import subprocess
import sys
import tempfile
from collections import Counter

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, 'stable-diffusion-on-device_amd')
FLAGS = ['--offload-arch=gfx950', '-O3', '-std=c++17', '-fPIC', '-mf16c', '-fvisibility=hidden',
         '-DSDOD_API=__attribute__((visibility("default")))', '-I' + os.path.join(ROOT, 'include'),
         '-I' + os.path.join(PKG, 'csrc'), '-Wno-unused-function', '-Wno-inline-asm', '-mllvm', '-amdgpu-mfma-vgpr-form']
COLS = ['mfma', 'valu', 'v_exp', 'v_fma', 'v_max', 'v_cvt', 'v_permlane', 'v_cndmask', 'lds', 'global', 'salu', 's_nop', 'waitcnt']


def classify(op):
    out = []
    if op.startswith('v_mfma'):
        return ['mfma']
    if op.startswith('v_'):
        out.append('valu')
        for c in ('v_exp', 'v_fma', 'v_max', 'v_cvt', 'v_permlane', 'v_cndmask'):
            if op.startswith(c):
                out.append(c)
    elif op.startswith('ds_'):
        out.append('lds')
    elif op.startswith(('global_', 'buffer_')):
        out.append('global')
    elif op == 's_nop':
        out.append('s_nop')
    elif op.startswith('s_waitcnt'):
        out.append('waitcnt')
    elif op.startswith('s_'):
        out.append('salu')
    return out


def mangled(spec):
    d, qt, tr, kvs = spec.split(',')
    return f'_ZN12_GLOBAL__N_111attn_kernelILi{d}ELi{qt}ELb{1 if tr == "true" else 0}ELi{kvs}EEEvNS_5AttnPE'


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--src', default=os.path.join(PKG, 'csrc', 'attention.hip'))
    ap.add_argument('--kernel', default='40,2,true,1', help='D,QT,TR,KVS of the instantiation to break down')
    ap.add_argument('--hipcc', default=os.environ.get('HIPCC', '/opt/rocm/bin/hipcc'))
    a = ap.parse_args()
    with tempfile.TemporaryDirectory() as td:
        asm = os.path.join(td, 'attention.s')
        r = subprocess.run([a.hipcc] + FLAGS + ['--offload-device-only', '-S', a.src, '-o', asm,
                                                '-Rpass-analysis=kernel-resource-usage'], capture_output=True, text=True)
        if r.returncode != 0:
            sys.exit(r.stderr)
        text = open(asm).read()
    # resource report
    res, cur = {}, None
    for line in r.stderr.splitlines():
        m = re.search(r'Function Name: (\S+)', line)
        if m:
            cur = m.group(1)
            res[cur] = {}
            continue
        m = re.search(r'remark:\s+(VGPRs|AGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]): (\d+)', line)
        if m and cur:
            res[cur][m.group(1).split(' ')[0]] = int(m.group(2))
    print(f'{"instantiation":24s} {"VGPRs":>6s} {"AGPRs":>6s} {"occupancy":>9s} {"scratch":>8s}')
    for name, v in res.items():
        m = re.match(r'_ZN12_GLOBAL__N_111attn_kernelILi(\d+)ELi(\d+)ELb(\d)ELi(\d+)E', name)
        if m:
            tag = f'<{m.group(1)},{m.group(2)},{"true" if m.group(3) == "1" else "false"},{m.group(4)}>'
            print(f'{tag:24s} {v.get("VGPRs", 0):6d} {v.get("AGPRs", 0):6d} {v.get("Occupancy", 0):9d} {v.get("ScratchSize", 0):8d}')
    # per-block mix of the chosen kernel
    name = mangled(a.kernel)
    start = text.find(f'\n{name}:')
    if start < 0:
        sys.exit(f'{name} not found')
    end = text.find('\n.Lfunc_end', start)
    blocks, order, label = {}, [], 'entry'
    branches = []
    for line in text[start:end].splitlines()[2:]:
        s = line.strip()
        m = re.match(r'; (%bb\.\d+):', s) # a fall-through block: its label is only a comment
        s = m.group(1) + ':' if m else s.split(';')[0].strip()
        if not s or s.startswith(('.p2align', '.loc', '.file')):
            continue
        if s.endswith(':') and not s.startswith('.set'):
            label = s[:-1]
            order.append(label)
            blocks[label] = Counter()
            continue
        if s.startswith('.'):
            continue
        op = s.split()[0]
        if label not in blocks:
            order.append(label)
            blocks[label] = Counter()
        blocks[label]['insts'] += 1
        for c in classify(op):
            blocks[label][c] += 1
        if op.startswith('s_cbranch') or op == 's_branch':
            branches.append((label, s.split()[-1]))
    pos = {b: i for i, b in enumerate(order)}
    loops = {tgt for src, tgt in branches if tgt in pos and pos[tgt] <= pos[src]}
    print(f'\n{a.kernel}: per-block instruction mix')
    print(f'{"block":18s} {"insts":>5s} ' + ' '.join(f'{c:>{max(len(c), 4)}s}' for c in COLS))
    tot = Counter()
    for b in order:
        c = blocks[b]
        tot.update(c)
        mark = ' loop' if b in loops else ''
        print(f'{(b + mark):18s} {c["insts"]:5d} ' + ' '.join(f'{c[k]:>{max(len(k), 4)}d}' for k in COLS))
    print(f'{"total":18s} {tot["insts"]:5d} ' + ' '.join(f'{tot[k]:>{max(len(k), 4)}d}' for k in COLS))


if __name__ == '__main__':
    main()
