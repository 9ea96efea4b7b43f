"""Weight gradient of the frequency-domain context Conv1D (ops._C1FFT.wgrad) at the default workload's shape: the older stage list
(split of the input's transform, transpose, 'corr' ptts_dense_bf16x6_batched) against the one on ptts_dense_tn_bf16x6_batched, per-stage HIP-event times (median
of the repetitions) and the difference of the two gradients.  python3 tools/conv1d_wgrad_tn_probe.py [B T Cin N KW]  (on the GPU box)"""
import math
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from percivaltts_amd import ops, _hip

B, T, Cin, N, KW = [int(v) for v in sys.argv[1:6]] if len(sys.argv) >= 6 else (64, 400, 601, 256, 21)
REPS = 9
g = torch.Generator().manual_seed(1)
x = torch.randn(B, T, Cin, generator=g).cuda()
w = (torch.randn(KW, Cin, N, generator=g) / math.sqrt(KW * Cin)).cuda().requires_grad_(True)
b = torch.randn(N, generator=g).cuda()
dy = torch.randn(B, T, N, generator=g).cuda()
ops.conv1d_fft(True)


def run(tn):
    ops._C1FFT.tn_enabled = tn
    ops.clear_caches()
    stages = {}
    order = []
    for rep in range(REPS + 2):
        w.grad = None
        y = ops.conv1d(x.clone(), w, b)             # a new input every step, as in training: the older list splits its transform again
        with _hip.KernelTimer() as kt:
            y.backward(dy, inputs=[w])
        if rep < 2:
            continue                                 # warm-up: scratch buffers, code objects
        for n, t, ms in kt.durations_ms():
            key = (n.replace('ptts_', ''), t[0] if t and isinstance(t[0], str) else '')
            if key not in stages:
                stages[key] = []; order.append(key)
            stages[key].append(ms * 1e3)
    med = [(k, sorted(stages[k])[len(stages[k]) // 2]) for k in order]
    return w.grad.detach().clone(), med


results = {}
for tn in (False, True, False, True):               # alternating: clocks drift over the first seconds of a process
    grad, med = run(tn)
    results[tn] = grad
    print('tn=%d: %7.1f us  ' % (tn, sum(v for _, v in med)) + '  '.join('%s%s %.1f' % (k[0], '[' + k[1] + ']' if k[1] else '', v) for k, v in med))
d = float((results[True] - results[False]).norm() / results[False].norm())
print('new against old: relative L2 %.3e' % d)
