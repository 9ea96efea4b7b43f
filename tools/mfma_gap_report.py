"""Where the vector work of an MFMA loop issues: a static report on a `hipcc -S` listing, no GPU needed.

    hipcc --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off -S --cuda-device-only dense.hip -o dense.s
    python tools/mfma_gap_report.py dense.s -k 'dense_wgrad_bf16x6_kernel<1, false, 3, false>' [--json out.json]

For every kernel whose (demangled) name contains one of the -k strings the report finds the loops -- a conditional branch back to a
label at or above it -- that hold MFMAs and no inner loop with MFMAs, and treats a loop body as a CYCLE: the instruction behind the
back edge is the loop's first.  The cycle is cut into k-steps at its barriers (a body without one is a single step), so the step that
straddles the back edge is one step and not two halves.  Per k-step:

  mfma, valu, cvt, lds, vmem   instruction counts (cvt = v_cvt_pk_bf16_f32, counted apart from valu; lds = ds_*; vmem = global/buffer/flat)
  gaps                         histogram {issue cost : number of gaps}.  A gap is what follows one MFMA up to the next MFMA or the step's
                               barrier; its cost is 4 cycles per VALU or LDS instruction and 8 per conversion (the 'vector-instruction
                               ISSUE cost' prices: an MFMA 16x16x32 holds the SIMD's vector issue for 8 of its 16 cycles)
  head                         cost of what stands between the step's opening barrier and its first MFMA: nothing hides it
  largest_clump                the largest gap in 4-cycle slots (the head counts as a gap here)
  estimate, floor, ratio       estimate = head + sum over MFMAs of max(16, 8 + cost of its gap);  floor = 16 x MFMAs

It is a model of issue order and mix, not of waits: s_waitcnt, scalar instructions and memory latency cost nothing in it.  The
compiler's register figures of each kernel (the `; NumVgprs` ... comment lines of the listing) are reported beside it."""
from __future__ import print_function

import argparse
import collections
import json
import re
import subprocess
import sys

SLOT = 4
COST = {'valu': 4, 'lds': 4, 'cvt': 8}
MFMA_CYCLES, MFMA_HOLD = 16, 8
CXXFILT = ('llvm-cxxfilt', 'c++filt', '/opt/rocm/llvm/bin/llvm-cxxfilt')


def kind(op):
    if op.startswith('v_mfma') or op.startswith('v_smfma'): return 'mfma'
    if op.startswith('v_cvt_pk_bf16_f32'): return 'cvt'
    if op.startswith('v_'): return 'valu'
    if op.startswith('ds_'): return 'lds'
    if op.startswith(('global_', 'buffer_', 'flat_', 'scratch_')): return 'vmem'
    if op == 's_barrier': return 'barrier'
    if op.startswith(('s_cbranch', 's_branch')): return 'branch'
    if op.startswith('s_waitcnt'): return 'wait'
    return 'other'


def demangle(names):
    for tool in CXXFILT:
        try:
            out = subprocess.run([tool] + names, stdout=subprocess.PIPE, universal_newlines=True, check=True).stdout.split('\n')
            return dict(zip(names, out))
        except (OSError, subprocess.CalledProcessError):
            continue
    return dict((n, n) for n in names)


def kernels(lines):
    """{symbol: (first line, last line)} of every .amdgpu_hsa_kernel / global function body in the listing"""
    out, cur = collections.OrderedDict(), None
    for i, l in enumerate(lines):
        m = re.match(r'^(_Z\w+):', l)
        if m and cur is None:
            cur = (m.group(1), i)
        elif cur and l.strip().startswith('.Lfunc_end'):
            out[cur[0]] = (cur[1], i)
            cur = None
    return out


def resources(lines, lo, hi):
    res = {}
    for l in lines[hi:hi + 80]:
        m = re.match(r'^; (NumVgprs|NumAgprs|TotalNumVgprs|ScratchSize|Occupancy|LDSByteSize|NumSgprs): *(\d+)', l)
        if m: res[m.group(1)] = int(m.group(2))
        if l.startswith('_Z'): break
    return res


def parse_body(lines, lo, hi):
    """[(kind, op, label-or-target)] with labels as ('label', name, None)"""
    ins = []
    for l in lines[lo + 1:hi]:
        s = l.split(';')[0].strip()
        if not s: continue
        m = re.match(r'^(\.LBB\w+):', s)
        if m:
            ins.append(('label', m.group(1), None)); continue
        if s.startswith('.'): continue
        t = s.split()
        k = kind(t[0])
        ins.append((k, t[0], t[-1] if k == 'branch' else None))
    return ins


def mfma_loops(ins):
    """innermost [head, back edge] index ranges that hold MFMAs"""
    at = dict((x[1], i) for i, x in enumerate(ins) if x[0] == 'label')
    loops = []
    for i, x in enumerate(ins):
        if x[0] == 'branch' and x[2] in at and at[x[2]] < i:
            h = at[x[2]]
            if any(y[0] == 'mfma' for y in ins[h:i]): loops.append((h, i))
    inner = [a for a in loops if not any(b != a and a[0] <= b[0] and b[1] <= a[1] for b in loops)]
    return inner


def step_report(seg):
    """seg: the instructions of one k-step, from behind its opening barrier to its closing barrier (or the whole cycle)"""
    counts = collections.Counter(x[0] for x in seg)
    gaps, head, cur, seen = [], 0, 0, False
    for x in seg:
        if x[0] == 'mfma':
            if seen: gaps.append(cur)
            else: head = cur
            seen, cur = True, 0
        else:
            cur += COST.get(x[0], 0)
    if seen: gaps.append(cur)
    else: head = cur
    n = counts['mfma']
    est = head + sum(max(MFMA_CYCLES, MFMA_HOLD + c) for c in gaps)
    floor = MFMA_CYCLES * n
    hist = collections.Counter(gaps)
    return {
        'mfma': n, 'valu': counts['valu'], 'cvt': counts['cvt'], 'lds': counts['lds'], 'vmem': counts['vmem'],
        'gaps': dict((str(c), hist[c]) for c in sorted(hist)),
        'gaps_over_two_slots': sum(1 for c in gaps if c > 2 * SLOT),
        'head': head,
        'largest_clump': max(gaps + [head]) // SLOT,
        'estimate': est, 'floor': floor, 'ratio': round(est / float(floor), 3) if floor else None,
    }


def loop_report(ins, h, e):
    body = [x for x in ins[h:e + 1] if x[0] != 'label']
    bars = [i for i, x in enumerate(body) if x[0] == 'barrier']
    if not bars:
        return [step_report(body)]
    steps = []
    for a, b in zip(bars, bars[1:] + [bars[0] + len(body)]):           # the last step runs through the back edge
        steps.append(step_report([body[i % len(body)] for i in range(a + 1, b)]))
    return [s for s in steps if s['mfma']]


def report(path, wanted):
    lines = open(path).read().split('\n')
    ks = kernels(lines)
    names = demangle(list(ks))
    out = collections.OrderedDict()
    for sym, (lo, hi) in ks.items():
        dn = names[sym].replace('ptts::dns::', '').replace('void ', '')
        dn = re.sub(r'\(.*\)$', '', dn)
        if wanted and not any(w in dn or w in sym for w in wanted): continue
        ins = parse_body(lines, lo, hi)
        loops = [{'first_label': ins[h][1], 'k_steps': loop_report(ins, h, e)} for h, e in mfma_loops(ins)]
        loops = [l for l in loops if l['k_steps']]
        out[dn] = {'registers': resources(lines, lo, hi), 'loops': loops}
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('listing')
    ap.add_argument('-k', '--kernel', action='append', default=[], help='substring of a demangled (or mangled) kernel name; may repeat; default: every kernel with an MFMA loop')
    ap.add_argument('--json', default=None, help='also write the report to this file')
    a = ap.parse_args()
    rep = report(a.listing, a.kernel)
    for name, r in rep.items():
        if not r['loops'] and not a.kernel: continue
        print(name)
        print('  registers', json.dumps(r['registers'], sort_keys=True))
        for lp in r['loops']:
            print('  loop at', lp['first_label'])
            for i, s in enumerate(lp['k_steps']):
                print('    k-step {}: mfma {mfma} valu {valu} cvt {cvt} lds {lds} vmem {vmem} | head {head} cyc, largest clump {largest_clump} slots, '
                      'gaps over two slots {gaps_over_two_slots} | estimate {estimate} / floor {floor} = {ratio}'.format(i, **s))
                print('      gap cost histogram (cycles: gaps)', json.dumps(s['gaps']))
    if a.json:
        with open(a.json, 'w') as f:
            json.dump(rep, f, indent=1)
    return 0


if __name__ == '__main__':
    sys.exit(main())
