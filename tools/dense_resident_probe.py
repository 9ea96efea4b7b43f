"""The three transform products of the frequency-domain context Conv1D (ops._C1FFT: 'dft', 'idft', 'dft_dy' -- ptts_dense_bf16x6_batched with a
shared left operand) at the default workload's shapes, with the resident-left kernel (ptts_set_dense_batched_resident) on and off: HIP-event
time per call (median of the repetitions, after warm-up), the bytes the call has to move and the rate that makes, and whether the two
kernels' outputs are equal.  python3 tools/dense_resident_probe.py [B T Cin N KW S]  (on the GPU box)"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from percivaltts_amd import ops, _hip

B, T, Cin, N, KW, S = [int(v) for v in sys.argv[1:7]] if len(sys.argv) >= 7 else (64, 400, 601, 256, 21, 100)
REPS, WARM = 21, 5
Z, P = B * (T // S), (S + KW - 1 + 3) // 4 * 4
NB = P // 2 + 1
R, Rp, Kh = 2 * NB, (2 * NB + 3) // 4 * 4, (Cin + 7) // 8 * 8
lib = _hip.lib()
g = torch.Generator().manual_seed(1)


def planes_of(nmat, K, Ncols):
    src = torch.randn(nmat, K, Ncols, generator=g).cuda()
    npb = lib.ptts_dense_planes_bytes(Ncols, K)
    pl = torch.empty(nmat * npb, dtype=torch.uint8, device='cuda')
    _hip.call('ptts_split3_dense_weight_strided', _hip.ptr(src), K * Ncols, _hip.ptr(pl), npb, nmat, Ncols, K, Ncols, 0, _hip.stream())
    return pl, npb


def live_plane_bytes(Ncols, K):
    """What a call reads of one member's planes: the column tiles of its 32-column slices, every k-step, three planes."""
    return 3 * 2 * ((Ncols + 31) // 32) * ((K + 31) // 32) * 1024


D = torch.randn(R, P, generator=g).cuda()
E = torch.randn(S, Rp, generator=g).cuda()
bias = torch.randn(N, generator=g).cuda()
calls = []
pl, npb = planes_of(Z, P, Cin)                       # 'dft': D [R x P] . window_z [P x Cin] -> rows of Ap, interleaved by member
calls.append(('dft', (D, pl, npb, None, torch.empty(R * Z * 2 * Kh, device='cuda'), 2 * Kh, Z, R, Cin, P, P, Z * 2 * Kh),
              Z * (live_plane_bytes(Cin, P) + R * Cin * 4)))
pl, npb = planes_of(Z, R, N)                         # 'idft': E [S x Rp] . Yh_z [R x N] + b -> S frames of y
calls.append(('idft', (E, pl, npb, bias, torch.empty(Z * S * N, device='cuda'), S * N, Z, S, N, Rp, Rp, N),
              Z * (live_plane_bytes(N, Rp) + S * N * 4)))
pl, npb = planes_of(Z, P, N)                         # 'dft_dy': D . dy-window_z [P x N] -> rows of DYh, interleaved by member
calls.append(('dft_dy', (D, pl, npb, None, torch.empty(R * Z * N, device='cuda'), N, Z, R, N, P, P, Z * N),
              Z * (live_plane_bytes(N, P) + R * N * 4)))


def run(name, a, on):
    A, pl, npb, b, C, sC, nb, M, Nc, K, lda, ldc = a
    lib.ptts_set_dense_batched_resident(1 if on else 0)
    C.fill_(-1.0)
    times = []
    for rep in range(REPS + WARM):
        with _hip.KernelTimer() as kt:
            _hip.call('ptts_dense_bf16x6_batched', _hip.ptr(A), 0, _hip.ptr(pl), npb, _hip.ptr(b), _hip.ptr(C), sC, nb, M, Nc, K, lda, ldc, 3,
                      _hip.stream())
        if rep >= WARM:
            times.append(kt.durations_ms()[0][2] * 1e3)
    return sorted(times)[len(times) // 2], C.clone()


print('CUs %d; Z %d, P %d, R %d, Rp %d' % (torch.cuda.get_device_properties(0).multi_processor_count, Z, P, R, Rp))
for name, a, nbytes in calls:
    assert lib.ptts_dense_batched_resident_eligible(0, a[7], a[8], a[9], 3) == 1
    res = {}
    for on in (False, True, False, True):                # alternating: clocks drift over the first seconds of a process
        us, out = run(name, a, on)
        res.setdefault(on, []).append(us)
        res[('out', on)] = out
    print('%-7s M %3d N %3d K %3d: %6.1f MB;  general %s us (%.0f GB/s)  resident %s us (%.0f GB/s)  equal %s' % (
        name, a[7], a[8], a[9], nbytes / 1e6, '/'.join('%.1f' % v for v in res[False]), nbytes / min(res[False]) / 1e3,
        '/'.join('%.1f' % v for v in res[True]), nbytes / min(res[True]) / 1e3, torch.equal(res[('out', True)], res[('out', False)])))
lib.ptts_set_dense_batched_resident(1)
