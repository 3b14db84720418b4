#!/usr/bin/env python3
"""Compare the device assembly of two builds of one .hip file, kernel by kernel (refactors that must not change code).

    hipcc <the Makefile's HIPFLAGS> --cuda-device-only -S csrc/gemm.hip -o before.s     (at the parent commit)
    hipcc <the Makefile's HIPFLAGS> --cuda-device-only -S csrc/gemm.hip -o after.s
    python tools/gemm_isa_diff.py before.s after.s > profiles/gemm_refactor_isa.txt

Per kernel: instruction count before -> after, the resource block (VGPRs, accumulator offset, SGPRs, scratch, LDS) and a
verdict:
    identical      every instruction and operand is the same (labels renumbered)
    same-mnemonics the same mnemonic sequence in every basic block, operands (registers, offsets) differ
    mfma-same      every basic block that holds a v_mfma has the parent's mnemonic sequence; outside them the mnemonic
                   histogram differs as listed
    MFMA-DIFF / RESOURCE-DIFF / FP-DIFF   what a refactor must not do
Reports mnemonics and resource numbers only."""
import collections
import re
import sys

RES = ('.amdhsa_next_free_vgpr', '.amdhsa_accum_offset', '.amdhsa_next_free_sgpr', '.amdhsa_private_segment_fixed_size',
       '.amdhsa_group_segment_fixed_size')
# floating-point arithmetic (a changed count of these is a changed computation, not addressing or branch form)
FP = re.compile(r'^v_(pk_)?(add|sub|subrev|mul|fma|fmac|mac|mad|max|min|exp|log|rcp|rsq|sqrt|cvt|dot2|dot2c|mfma|cndmask|ldexp|trunc|floor|rndne|fract)'
                r'.*(_f16|_f32|_f64|_bf16|_legacy)')


def parse(path):
    kernels, res = {}, {}
    name, blocks, cur, desc = None, None, None, None
    for line in open(path, errors='replace'):
        t = line.strip()
        if desc is not None:
            if t.startswith('.end_amdhsa_kernel'):
                desc = None
            else:
                f = t.split()
                if f and f[0] in RES:
                    res[desc][f[0]] = f[1]
            continue
        if t.startswith('.amdhsa_kernel '):
            desc = t.split()[1]
            res[desc] = {}
            continue
        if name is None:
            m = re.match(r'^(_Z\w+|\w+):\s*(;.*)?$', line)
            if m and not line.startswith('.'):
                name, blocks, cur = m.group(1), [], []
            continue
        if t.startswith('.Lfunc_end'):
            blocks.append(cur)
            kernels[name] = [b for b in blocks if b]
            name = None
            continue
        if re.match(r'^\.LBB\d+_\d+:', t):
            blocks.append(cur)
            cur = []
            continue
        if not t or t[0] in '.;':
            continue
        t = t.split(';')[0].strip()
        if t:
            cur.append(re.sub(r'\.LBB\d+_', '.LBB_', t))
    return {k: v for k, v in kernels.items() if k in res}, res


def mnem(block):
    return tuple(i.split()[0] for i in block)


def main(a_path, b_path):
    ka, ra = parse(a_path)
    kb, rb = parse(b_path)
    print(f'kernels: {len(ka)} before, {len(kb)} after; names {"the same" if set(ka) == set(kb) else "DIFFER"}')
    for n in sorted(set(ka) ^ set(kb)):
        print('  only in', 'before' if n in ka else 'after', n)
    tally = collections.Counter()
    for n in sorted(set(ka) & set(kb)):
        a, b = ka[n], kb[n]
        na, nb = sum(map(len, a)), sum(map(len, b))
        notes = []
        if ra[n] != rb[n]:
            verdict = 'RESOURCE-DIFF'
            notes.append(f'before {ra[n]} after {rb[n]}')
        elif a == b:
            verdict = 'identical'
        elif [mnem(x) for x in a] == [mnem(x) for x in b]:
            verdict = 'same-mnemonics'
        else:
            ma = [mnem(x) for x in a if any(i.startswith('v_mfma') for i in x)]
            mb = [mnem(x) for x in b if any(i.startswith('v_mfma') for i in x)]
            ha = collections.Counter(m for x in a for m in mnem(x))
            hb = collections.Counter(m for x in b for m in mnem(x))
            diff = {m: (ha[m], hb[m]) for m in sorted(set(ha) | set(hb)) if ha[m] != hb[m]}
            if ma != mb:
                verdict = 'MFMA-DIFF'
            elif any(FP.match(m) for m in diff):
                verdict = 'FP-DIFF'
            else:
                verdict = 'mfma-same'
            notes.append('histogram ' + ', '.join(f'{m} {x}->{y}' for m, (x, y) in diff.items()) if diff else 'same histogram, other order')
        tally[verdict] += 1
        r = rb[n]
        print(f'{n}: instructions {na} -> {nb}; vgpr {r.get(RES[0])} accum_offset {r.get(RES[1])} sgpr {r.get(RES[2])} '
              f'scratch {r.get(RES[3])} lds {r.get(RES[4])}; {verdict}' + ''.join('; ' + x for x in notes))
    print('verdicts:', dict(tally))
    return 0 if set(ka) == set(kb) and not any(v.isupper() for v in tally) else 1


if __name__ == '__main__':
    sys.exit(main(sys.argv[1], sys.argv[2]))
