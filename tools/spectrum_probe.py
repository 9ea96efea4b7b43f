#!/usr/bin/env python
"""Times the launches of csrc/spectrum.hip with HIP events at a generation-corpus size and prints the figures of DESIGN.md
section 6: ptts_mcep2spec and ptts_fwbnd2spec as GB/s against the 4 T K bytes they have to write and as a fraction of the HBM
figure bench.py's roofline uses (8 TB/s), beside a device-to-device copy_ of the same size on the same box; ptts_mcep_postfilter
as frames/s, beside the numpy closed form on the host (a sample of the frames, on the threads the environment allows); and, for
the same inputs, e32 (the float32 closed form's worst error against fp64) next to the kernel's, on a sample of the frames.
The spec2mcep leg runs ptts_spec2mcep on the log-envelopes of --fit-frames of the cepstra and reports the time of one build of
its table, the time of a call, the rate against the 4 T K bytes it has to read, and the round trip's worst error.

Default size: T = 100 000 frames, M1 = 60 mel-cepstra, nb = 129 bands, dftlen = 4096, fs = 32 000.

    python tools/spectrum_probe.py [--frames 100000] [--M1 60] [--nb 129] [--dftlen 4096] [--fs 32000] [--reps 20] [--host-frames 2000] [--fit-frames 4000]
"""
from __future__ import print_function

import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

PEAK_HBM_GBPS = 8000.0          # the figure of bench.py's roofline
PF = 1.4


def timed(fn, reps, warmup=3):
    import torch
    for _ in range(warmup): fn()
    times = []
    for _ in range(reps):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record(); fn(); e.record()
        e.synchronize()
        times.append(s.elapsed_time(e) * 1e-3)
    return float(np.median(times))


def warped(alpha, L, dtype):
    w = dtype(2.0 * np.pi) * np.arange(L // 2 + 1).astype(dtype) / dtype(L)
    return w + dtype(2.0) * np.arctan2(dtype(alpha) * np.sin(w), dtype(1.0) - dtype(alpha) * np.cos(w))


def logspec(c, alpha, L, dtype):
    m = np.arange(c.shape[1]).astype(dtype)
    return c.astype(dtype) @ np.cos(m[:, None] * warped(alpha, L, dtype)[None, :])


def r0(la, L):
    E = np.exp(la.dtype.type(2.0) * la)
    return (E[:, 0] + E[:, -1] + la.dtype.type(2.0) * E[:, 1:-1].sum(axis=1)) / la.dtype.type(L)


def postfilter(c, alpha, L, dtype):
    c = c.astype(dtype)
    w = np.full(c.shape[1], PF, dtype=dtype)
    w[:2] = 1.0
    out = c * w
    out[:, 0] += dtype(0.5) * np.log(r0(logspec(c, alpha, L, dtype), L) / r0(logspec(out, alpha, L, dtype), L))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--frames', type=int, default=100000)
    ap.add_argument('--M1', type=int, default=60)
    ap.add_argument('--nb', type=int, default=129)
    ap.add_argument('--dftlen', type=int, default=4096)
    ap.add_argument('--fs', type=float, default=32000.0)
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--host-frames', type=int, default=2000)
    ap.add_argument('--fit-frames', type=int, default=4000)
    args = ap.parse_args()

    import torch
    from percivaltts_amd import ops
    assert torch.cuda.is_available(), 'spectrum_probe needs the GPU'
    T, M1, nb, L = args.frames, args.M1, args.nb, args.dftlen
    K = L // 2 + 1
    alpha = ops.bark_alpha(args.fs)
    rng = np.random.RandomState(0)
    c = rng.randn(T, M1) * (0.5 / (1.0 + np.arange(M1)))[None, :]
    c[:, 0] = rng.uniform(-6.0, -1.0, size=T)
    c = c.astype(np.float32)
    fw = (rng.uniform(-6.0, -1.0, size=(T, 1)) + np.cumsum(rng.randn(T, nb) * 0.3, axis=1)).astype(np.float32)
    cd, fd = torch.from_numpy(c).cuda(), torch.from_numpy(fw).cuda()

    out_bytes = 4.0 * T * K
    res = {'frames': T, 'M1': M1, 'nb': nb, 'dftlen': L, 'fs': args.fs, 'alpha': alpha, 'device': torch.cuda.get_device_name(0),
           'out_GB': out_bytes * 1e-9}
    src = torch.empty((T, K), dtype=torch.float32, device='cuda').normal_()
    dst = torch.empty_like(src)
    t = timed(lambda: dst.copy_(src), args.reps)
    res['copy'] = {'s': t, 'GBps_written': out_bytes / t * 1e-9}
    del src, dst
    for name, fn in (('mcep2spec', lambda: ops.mcep2spec(cd, alpha, dftlen=L)),
                     ('mcep2spec_log', lambda: ops.mcep2spec(cd, alpha, dftlen=L, log=True)),
                     ('mcep2spec_pp', lambda: ops.mcep2spec(cd, alpha, dftlen=L, pp=True)),
                     ('fwbnd2spec', lambda: ops.fwbnd2spec(fd, args.fs, dftlen=L)),
                     ('fwbnd2spec_pp', lambda: ops.fwbnd2spec(fd, args.fs, dftlen=L, pp=True))):
        t = timed(fn, args.reps)
        res[name] = {'s': t, 'GBps_written': out_bytes / t * 1e-9, 'frac_of_8TBps': out_bytes / t * 1e-9 / PEAK_HBM_GBPS}
    t = timed(lambda: ops.mcep_postfilter(cd, alpha, dftlen=L), args.reps)
    res['mcep_postfilter'] = {'s': t, 'frames_per_s': T / t, 'fp64_fma_per_s': 1.0 * T * K * M1 / t}

    # the fit: table build (its four launches on a fresh buffer), then the product on log-envelopes of the same cepstra
    from percivaltts_amd import _hip
    nf = min(args.fit_frames, T)
    nbytes = _hip.lib().ptts_spec2mcep_table_bytes(M1, L)
    tab = torch.empty(nbytes // 8, dtype=torch.float64, device='cuda')
    tb = timed(lambda: _hip.call('ptts_spec2mcep_table', _hip.ptr(tab), nbytes, M1, float(alpha), L, _hip.stream()), args.reps)
    la = ops.mcep2spec(cd[:nf], alpha, dftlen=L, log=True)
    t = timed(lambda: ops.spec2mcep(la, alpha, M1 - 1, log=True), args.reps)
    tl = timed(lambda: ops.spec2mcep(la, alpha, M1 - 1), args.reps)            # with the logarithm of every element
    res['spec2mcep'] = {'frames': nf, 'table_bytes': nbytes, 'table_build_s': tb, 's': t, 's_linear_input': tl,
                        'frames_per_s': nf / t, 'GBps_read': 4.0 * nf * K / t * 1e-9,
                        'frac_of_8TBps': 4.0 * nf * K / t * 1e-9 / PEAK_HBM_GBPS, 'fp64_fma_per_s': 1.0 * nf * K * M1 / t,
                        'round_trip_worst': float((ops.spec2mcep(la, alpha, M1 - 1, log=True) - cd[:nf]).abs().max())}
    del la, tab

    # host: the numpy closed form in fp64 on a sample of the frames
    n = min(args.host_frames, T)
    t0 = time.time()
    want = postfilter(c[:n], alpha, L, np.float64)
    th = time.time() - t0
    res['host_postfilter'] = {'frames': n, 's': th, 'frames_per_s': n / th, 'threads': int(os.environ.get('OMP_NUM_THREADS', '16'))}

    # accuracy on the same sample: e32 and the kernel's worst error (absolute for cepstra / log-spectra, relative for spectra)
    def two(got, w64, w32, rel):
        e, e32 = np.abs(got.astype(np.float64) - w64), np.abs(w32.astype(np.float64) - w64)
        if rel: e, e32 = e / np.abs(w64), e32 / np.abs(w64)
        return {'e32': float(e32.max()), 'kernel': float(e.max())}
    res['accuracy'] = {
        'mcep_postfilter': two(ops.mcep_postfilter(cd[:n], alpha, dftlen=L).cpu().numpy(), want, postfilter(c[:n], alpha, L, np.float32), False),
        'mcep2spec_log': two(ops.mcep2spec(cd[:n], alpha, dftlen=L, log=True).cpu().numpy(), logspec(c[:n], alpha, L, np.float64),
                             logspec(c[:n], alpha, L, np.float32), False),
        'mcep2spec': two(ops.mcep2spec(cd[:n], alpha, dftlen=L).cpu().numpy(), np.exp(logspec(c[:n], alpha, L, np.float64)),
                         np.exp(logspec(c[:n], alpha, L, np.float32)), True),
    }
    print(json.dumps(res, indent=1, sort_keys=True))


if __name__ == '__main__':
    main()
