#!/usr/bin/env python
"""Order of operand fetches, waits and MFMAs in a kernel's loops, read from the compiler's assembly.

    hipcc -O3 -std=c++17 --offload-arch=gfx950 -ffp-contract=off --cuda-device-only -S arflow_amd/csrc/splitconv.hip -o sc.s
    python tools/schedule_listing.py sc.s 'splitconv_kernelILi2ELi32'

For every basic block of the kernel whose mangled name contains the pattern and that holds at least --min-mfma MFMAs, one
line per run of equal instructions: `12x v_mfma`, `3x global_load_dwordx4`, `s_waitcnt vmcnt(6)`, ...  Instructions other
than global loads, LDS reads, waits, MFMAs, barriers and branches are left out.  Below every block: how many waits on vmcnt
(lgkmcnt) retire a global load (LDS read) issued within the two instructions before them, listed or not, i.e. wait for an
operand that was requested immediately before.
"""
import argparse
import re

ap = argparse.ArgumentParser()
ap.add_argument('asm')
ap.add_argument('pattern')
ap.add_argument('--min-mfma', type=int, default=6)
args = ap.parse_args()

KEEP = re.compile(r'^(global_load_\w+|ds_read\w*|ds_load\w*|s_waitcnt|v_mfma\w+|s_barrier|s_cbranch\w+|s_branch)\b')

lines = open(args.asm).read().split('\n')
inside, blocks, cur = False, [], None
for ln in lines:
    s = ln.strip()
    m = re.match(r'^(\S+):', s)
    if m and not s.startswith('.L') and not s.startswith(';'):
        inside = args.pattern in m.group(1) and not m.group(1).endswith('.kd')
        if inside:
            blocks.append((m.group(1), None))
        cur = None
        continue
    if not inside:
        continue
    if s.startswith('.Lfunc_end'):
        inside = False
        continue
    if m:
        cur = [m.group(1), []]
        blocks.append(cur)
        continue
    if not s or s.startswith(';') or s.startswith('.'):
        continue
    if cur is None:
        cur = ['(entry)', []]
        blocks.append(cur)
    cur[1].append(s.split(';')[0].strip())

for name, ins in blocks:
    if ins is None:
        print('== ' + name)
        continue
    n_mfma = sum(1 for i in ins if i.startswith('v_mfma'))
    if n_mfma < args.min_mfma:
        continue
    print('-- block %s: %d instructions, %d MFMA, %d global_load, %d ds_read, %d s_waitcnt' % (
        name, len(ins), n_mfma, sum(i.startswith('global_load') for i in ins), sum(i.startswith(('ds_read', 'ds_load')) for i in ins),
        sum(i.startswith('s_waitcnt') for i in ins)))
    runs = []
    near_vm = near_lgkm = 0
    for k, i in enumerate(ins):
        m = KEEP.match(i)
        if not m:
            continue
        op = m.group(1)
        if op == 's_waitcnt':
            key = i
            # a counter at N retires every fetch but the N most recent: a fetch among the two instructions before the wait is
            # retired by it iff fewer than N fetches of its kind follow it, i.e. iff its recency rank (1 = last) exceeds N
            for cnt, kinds in (('vmcnt', ('global_load',)), ('lgkmcnt', ('ds_read', 'ds_load'))):
                m2 = re.search(cnt + r'\((\d+)\)', i)
                if not m2:
                    continue
                rank = 0
                for back in (1, 2):
                    if k - back >= 0 and ins[k - back].startswith(kinds):
                        rank += 1
                        if rank > int(m2.group(1)):
                            if cnt == 'vmcnt':
                                near_vm += 1
                            else:
                                near_lgkm += 1
                            break
        elif op.startswith('v_mfma'):
            key = 'v_mfma'
        elif op.startswith('s_cbranch') or op == 's_branch':
            key = i
        else:
            key = op
        if runs and runs[-1][0] == key:
            runs[-1][1] += 1
        else:
            runs.append([key, 1])
    print('   ' + '\n   '.join(('%dx %s' % (c, k)) if c > 1 else k for k, c in runs))
    print('   waits within two instructions of the fetch they retire: vmcnt %d, lgkmcnt %d' % (near_vm, near_lgkm))
