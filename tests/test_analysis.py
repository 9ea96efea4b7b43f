"""Waveform analysis for the PML parameters (csrc/analysis.hip; ops.analysis_check / f0_track / frame_harmonics / phase_coherence /
fwbnd_compress, VocoderF0Spec.compress_spectrum, VocoderPML.analysis_device / analysisf_device / analysisfid_device, vocoders.wavread,
run.features_extraction).

The reference delegates the analysis to a submodule that is absent from its checkout, so there is nothing of it to compare with: the
definition is the build's own and is restated here in numpy, in a chosen dtype, frame by frame and harmonic by
harmonic.  The transform of a frame is torch.fft.rfft, which keeps the dtype.  Integer decisions (sample and bin indices, harmonic
counts) are taken in float64 from the float32 inputs in both dtypes, as the kernels take them.

Tolerance of the device results: the rule of tests/test_pulsesynth.py (`check` there).  The yardstick is the restatement in float64;
the same restatement in float32 has a largest error e32 against it on the same input; every element of a device result has to lie
within 4 * e32 + 2^-23 * max|want64| of the float64 value.

The test signal is the float64 synthesis restatement of tests/test_pulsesynth.py on a smooth envelope of 8 nepers with the noise mask
set above fs/5: a pulse train below, noise above."""
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_pulsesynth as ps                                    # noqa: E402  (the synthesis restatement, `check`, the two shapes)

check, rnd, band_centres = ps.check, ps.rnd, ps.band_centres
SHIFT, SHAPES = ps.SHIFT, ps.SHAPES
F0_MIN, F0_MAX = 100.0, 400.0
NOISY_BELOW = math.exp(-0.75 ** 2 / 2)
FLT_MIN = float(np.finfo(np.float32).tiny)


# ---------------------------------------------------------------------------------------------------------------------------
# the definition, restated
# ---------------------------------------------------------------------------------------------------------------------------
def harmonics_of(f0, fs):
    return int(math.floor((0.5 * fs - 0.5 * f0) / f0))


def hcap_of(fs, f0_min):
    return harmonics_of(f0_min, fs) - 1


def track_restated(f0, f0_min, f0_max):
    """Unvoiced values (<= 0) interpolated between their voiced neighbours, ends held, clipped."""
    f0 = [float(x) for x in f0]
    voiced = [i for i, x in enumerate(f0) if x > 0]
    if not voiced:
        raise ValueError('no voiced frame')
    out = []
    for i, x in enumerate(f0):
        if x <= 0:
            before = [j for j in voiced if j < i]
            after = [j for j in voiced if j > i]
            if not before: x = f0[after[0]]
            elif not after: x = f0[before[-1]]
            else:
                a, b = before[-1], after[0]
                x = f0[a] + (f0[b] - f0[a]) * (i - a) / float(b - a)
        out.append(min(max(x, f0_min), f0_max))
    return np.array(out)


def frames_restated(wav, f0, shift, fs, L, hcap, dtype):
    """wav [N], f0 [T] -> (ln SPEC [T,K], u [T,hcap,2]) in `dtype`."""
    dt = np.dtype(dtype).type
    wav = np.asarray(wav, dtype=dtype)
    N, T, K = len(wav), len(f0), L // 2 + 1
    lspec = np.zeros((T, K), dtype=dtype)
    u = np.zeros((T, hcap, 2), dtype=dtype)
    tiny = 1e-300 if dtype == np.float64 else 1e-37
    for i in range(T):
        f0i = float(f0[i])
        c, hw = rnd(i * shift * fs), int(1.5 * fs / f0i)
        w = np.blackman(2 * hw + 1)
        w = (w / w.sum()).astype(dtype)
        x = np.zeros(L, dtype=dtype)
        for j in range(-hw, hw + 1):
            if 0 <= c + j < N:
                x[j % L] = wav[c + j] * w[j + hw]
        X = torch.fft.rfft(torch.from_numpy(x)).numpy()
        assert X.dtype == (np.complex128 if dtype == np.float64 else np.complex64)
        mag = np.abs(X)
        H = harmonics_of(f0i, fs)
        a = np.zeros(H + 1, dtype=dtype)
        for h in range(1, H + 1):
            lo, hi = rnd((h - 0.5) * f0i * L / fs), min(rnd((h + 0.5) * f0i * L / fs), K)
            p = mag[lo:hi].max() if hi > lo else dt(0)
            a[h] = np.log(max(p * dt(fs) / dt(f0i), dt(1e-10)))
        xs = np.arange(K).astype(dtype) * dt(fs) / dt(L) / dt(f0i)
        h0 = np.clip(np.floor(xs).astype(np.int64), 1, max(H - 1, 1))
        mid = a[h0] + (xs - h0.astype(dtype)) * (a[np.minimum(h0 + 1, H)] - a[h0])
        lspec[i] = np.where(xs < 1, a[1], np.where(xs >= H, a[H], mid))
        k1 = rnd(1.0 * f0i * L / fs)
        for h in range(1, H):
            ka, kb = rnd(h * f0i * L / fs), rnd((h + 1) * f0i * L / fs)
            z = X[kb] * np.conj(X[ka]) * np.conj(X[k1])
            m = np.abs(z)
            if not m < tiny:
                u[i, h - 1] = (z.real / m, z.imag / m)
    return lspec, u


def coherence_restated(u, f0, shift, fs, dtype):
    """u [T,hcap,2] -> R [T,hcap] in `dtype`; 1 behind a frame's harmonics."""
    dt = np.dtype(dtype).type
    u = np.asarray(u, dtype=dtype)
    T, hcap = u.shape[:2]
    Hs = [harmonics_of(float(x), fs) for x in f0]
    R = np.ones((T, hcap), dtype=dtype)
    for i in range(T):
        J = max(2, rnd(1.0 / (float(f0[i]) * shift)))
        for h in range(1, Hs[i]):
            sx, sy, n = dt(0), dt(0), 0
            for m in range(max(0, i - J), min(T - 1, i + J) + 1):
                if h < Hs[m]:
                    sx, sy, n = sx + u[m, h - 1, 0], sy + u[m, h - 1, 1], n + 1
            R[i, h - 1] = np.sqrt(sx * sx + sy * sy) / dt(n)
    return R


def band_weights(nb, fs, L):
    """W [K,nb] float64: the weight with which fwbnd2spec reads band b at bin k.  ValueError when a band weighs less than a bin."""
    K = L // 2 + 1
    fb = band_centres(nb, fs)
    W = np.zeros((K, nb))
    for k in range(K):
        f = k * float(fs) / L
        b = min(max(int(np.searchsorted(fb, f, side='right')) - 1, 0), nb - 2)
        fr = min(max((f - fb[b]) / (fb[b + 1] - fb[b]), 0.0), 1.0)
        W[k, b] += 1.0 - fr
        W[k, b + 1] += fr
    if W.sum(0).min() < 1.0:
        raise ValueError('nb is too large for dftlen')
    return W


def noise_bands_restated(R, f0, fs, L, W, dtype):
    """R [T,hcap] -> NM [T,nb]: the bin mask of the flags R < exp(-0.75^2/2), averaged with the hat weights."""
    T, K = R.shape[0], L // 2 + 1
    Wd = W.astype(dtype)
    s = Wd.sum(0)
    nm = np.zeros((T, W.shape[1]), dtype=dtype)
    for i in range(T):
        f0i = float(f0[i])
        H = harmonics_of(f0i, fs)
        mask = np.zeros(K, dtype=dtype)
        for k in range(K):
            h = min(max(int(math.floor(k * fs / (L * f0i))), 1), H - 1)
            mask[k] = 1.0 if R[i, h - 1] < NOISY_BELOW else 0.0
        nm[i] = Wd.T.dot(mask) / s
    return nm


def compress_restated(x, W, mode, is_log, dtype):
    """x [T,K] -> [T,nb] in `dtype`: the hat-weighted mean, or the least-squares solve through the Thomas recurrences."""
    x = np.asarray(x, dtype=dtype)
    Wd = W.astype(dtype)
    nb = W.shape[1]
    if mode == 'mean':
        return x.dot(Wd) / Wd.sum(0)
    v = x if is_log else np.log(np.maximum(np.abs(x), np.dtype(dtype).type(FLT_MIN)))
    A = W.T.dot(W)                                              # the table: float64 in both
    d, e = np.diag(A).copy(), np.diag(A, 1).copy()
    inv, cp = np.zeros(nb), np.zeros(nb)
    m = d[0]
    for b in range(nb):
        inv[b] = 1.0 / m
        if b + 1 < nb:
            cp[b] = e[b] * inv[b]
            m = d[b + 1] - e[b] * cp[b]
    e, inv, cp = e.astype(dtype), inv.astype(dtype), cp.astype(dtype)
    y = v.dot(Wd)
    for b in range(nb):
        y[:, b] = (y[:, b] - (e[b - 1] * y[:, b - 1] if b else 0)) * inv[b]
    for b in range(nb - 2, -1, -1):
        y[:, b] = y[:, b] - cp[b] * y[:, b + 1]
    return y


# ---------------------------------------------------------------------------------------------------------------------------
# the two shapes; their signals and references are computed once
# ---------------------------------------------------------------------------------------------------------------------------
NBS = (9, 65)
_cases = {}


def known_envelope(name):
    """f0 [T], the known envelope [T,K] (two smooth rows of 8 nepers and a slow morph between them: the rows of
    test_pulsesynth's inputs are unrelated from frame to frame, which no window of three periods can follow), a mask that is 1
    above fs/5, the noise, the pulse rows."""
    c = dict(ps.make_inputs(name))
    K, fs, L = c['K'], c['fs'], c['L']
    la, x = np.log(c['spec'][[0, -1]].astype(np.float64)), np.linspace(0, 1, c['T'])[:, None]
    c['spec'] = np.exp((1 - x) * la[0] + x * la[1]).astype(np.float32)
    c['mask'] = np.tile((np.arange(K) * float(fs) / L >= fs / 5.0).astype(np.float32), (c['T'], 1))
    c['rows'] = ps.table_restated(c['f0'], SHIFT, fs, c['wavlen'], L)[1]
    return c


def case(name):
    if name not in _cases:
        c = known_envelope(name)
        fs, L = c['fs'], c['L']
        wav = ps.synth_restated(c['spec'], c['mask'], c['g'], c['rows'], fs, L, c['wavlen'], torch.float64)
        c['wav64'] = wav
        c['wav'] = wav.astype(np.float32)
        c['hcap'] = hcap_of(fs, F0_MIN)
        for tag, dtype in (('64', np.float64), ('32', np.float32)):
            c['lspec' + tag], c['u' + tag] = frames_restated(c['wav'], c['f0'], SHIFT, fs, L, c['hcap'], dtype)
            # the coherence of the SAME phasors in both dtypes: the float32 values a kernel would be given
            c['R' + tag] = coherence_restated(c['u64'].astype(np.float32), c['f0'], SHIFT, fs, dtype)
        for v in c.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _cases[name] = c
    return _cases[name]


def interior(c):
    """The frames whose window lies inside the waveform."""
    out = []
    for i in range(c['T']):
        hw = int(1.5 * c['fs'] / float(c['f0'][i]))
        if rnd(i * SHIFT * c['fs']) - hw >= 0 and rnd(i * SHIFT * c['fs']) + hw < len(c['wav']):
            out.append(i)
    return out


def envelope_rms_db(lspec, c):
    """rms over the interior frames and the bins of [f0, fs/5 - f0) of 20 log10(analysed / known)."""
    err = []
    for i in interior(c):
        f = np.arange(c['K']) * float(c['fs']) / c['L']
        sel = (f >= float(c['f0'][i])) & (f < c['fs'] / 5.0 - float(c['f0'][i]))
        err.append((20.0 / math.log(10.0)) * (np.asarray(lspec[i], dtype=np.float64)[sel] - np.log(c['spec'][i].astype(np.float64))[sel]))
    return float(np.sqrt(np.mean(np.concatenate(err) ** 2)))


# ---------------------------------------------------------------------------------------------------------------------------
# CPU: the restatement
# ---------------------------------------------------------------------------------------------------------------------------
def test_restated_stationary_harmonics_are_recovered_and_coherent():
    fs, L, m, T = 8000, 512, 10, 20
    f0 = m * fs / float(L)                                       # 156.25 Hz: every harmonic on a bin
    H, hw = harmonics_of(f0, fs), int(1.5 * fs / f0)
    rng = np.random.RandomState(1)
    N = rnd((T - 1) * SHIFT * fs) + 1
    n = np.arange(N)
    wav = sum(np.cos(2 * np.pi * h * f0 * n / fs + ph) for h, ph in zip(range(1, H + 1), rng.uniform(0, 2 * np.pi, H)))
    f0v = np.full(T, f0, dtype=np.float32)
    hcap = hcap_of(fs, F0_MIN)
    lspec, u = frames_restated(wav, f0v, SHIFT, fs, L, hcap, np.float64)
    inside = [i for i in range(T) if rnd(i * SHIFT * fs) - hw >= 0 and rnd(i * SHIFT * fs) + hw < N]
    assert len(inside) >= 12
    got = np.exp(lspec[inside][:, m * np.arange(1, H + 1)])
    worst = np.abs(got / (fs / (2 * f0)) - 1).max()
    print('stationary harmonics: worst relative amplitude error {:.3e}'.format(worst))
    assert worst <= 1e-2
    R = coherence_restated(u, f0v, SHIFT, fs, np.float64)
    J = max(2, rnd(1.0 / (f0 * SHIFT)))
    deep = [i for i in inside if i - J in inside and i + J in inside]
    assert len(deep) >= 6
    print('stationary harmonics: smallest R {:.9f}'.format(R[deep][:, :H - 1].min()))
    assert R[deep][:, :H - 1].min() >= 1 - 1e-5
    assert (R[:, H - 1:] == 1).all()


def test_restated_white_noise_is_flagged():
    fs, L, T = 8000, 512, 40
    rng = np.random.RandomState(2)
    wav = rng.randn(rnd((T - 1) * SHIFT * fs) + 1)
    f0v = (170.0 + 60.0 * np.sin(np.arange(T) / 7.0)).astype(np.float32)
    hcap = hcap_of(fs, F0_MIN)
    _, u = frames_restated(wav, f0v, SHIFT, fs, L, hcap, np.float64)
    R = coherence_restated(u, f0v, SHIFT, fs, np.float64)
    flags = np.concatenate([R[i, :harmonics_of(float(f0v[i]), fs) - 1] < NOISY_BELOW for i in range(2, T - 2)])
    print('white noise: {:.1f} % of the harmonics flagged'.format(100 * flags.mean()))
    assert flags.mean() >= 0.70


@pytest.mark.parametrize('name', ['A', 'B'])
def test_restated_pulse_train_is_voiced_below_and_noisy_above(name):
    """The test signal itself: the known envelope comes back and the mask follows the cut-off at fs/5."""
    c = case(name)
    rms = envelope_rms_db(c['lspec64'], c)
    print('{}: envelope rms error {:.3f} dB over the voiced band'.format(name, rms))
    assert rms < (2.0 if name == 'A' else 0.8)                  # 1.5 dB and 0.4 dB where the definition was prototyped
    low, high = [], []
    for i in interior(c)[2:-2]:
        f0i = float(c['f0'][i])
        for h in range(1, harmonics_of(f0i, c['fs'])):
            if (h + 1) * f0i < c['fs'] / 5.0 - f0i: low.append(c['R64'][i, h - 1] < NOISY_BELOW)
            if h * f0i > c['fs'] / 5.0 + f0i: high.append(c['R64'][i, h - 1] < NOISY_BELOW)
    print('{}: flagged {:.1f} % below the cut-off, {:.1f} % above'.format(name, 100 * np.mean(low), 100 * np.mean(high)))
    assert np.mean(low) <= 0.10 and np.mean(high) >= 0.70


@pytest.mark.parametrize('fs,L,nb', [(8000, 512, 9), (8000, 512, 65), (32000, 4096, 129)])
def test_restated_band_compression_inverts_the_decompression(fs, L, nb):
    W = band_weights(nb, fs, L)
    A = W.T.dot(W)
    off = A - np.diag(np.diag(A)) - np.diag(np.diag(A, 1), 1) - np.diag(np.diag(A, -1), -1)
    assert (off == 0).all()
    assert np.linalg.cond(A) < 60, np.linalg.cond(A)
    np.testing.assert_allclose(W.sum(1), 1.0, rtol=0, atol=1e-14)
    y = np.random.RandomState(3).randn(5, nb) * 2 - 4
    got = compress_restated(y.dot(W.T), W, 'lsq', True, np.float64)
    assert np.abs(got - y).max() <= 1e-10
    got = compress_restated(np.exp(y.dot(W.T)), W, 'lsq', False, np.float64)
    assert np.abs(got - y).max() <= 1e-10


def test_band_axis_too_fine_is_refused():
    from percivaltts_amd import ops
    with pytest.raises(ValueError):
        band_weights(129, 16000, 512)
    with pytest.raises(ValueError):
        ops.fwbnd_compress_check(129, 16000, 512)
    for fs, L, nb in [(8000, 512, 9), (8000, 512, 65), (32000, 4096, 129), (16000, 4096, 129), (16000, 4096, 33)]:
        ops.fwbnd_compress_check(nb, fs, L)
    with pytest.raises(ValueError):
        ops.fwbnd_compress_check(1, 8000, 512)
    with pytest.raises(ValueError):
        ops.fwbnd_compress_check(9, 8000, 511)


# ---------------------------------------------------------------------------------------------------------------------------
# CPU: the host step and the public interface
# ---------------------------------------------------------------------------------------------------------------------------
def test_f0_track(capsys):
    from percivaltts_amd import ops
    fs, L = 8000, 512
    raw = [0, 0, 120, 0, 0, 180, 0, 500, 50, 0]
    got = ops.f0_track(raw, F0_MIN, F0_MAX, fs, SHIFT, L)
    assert got.dtype == np.float32 and got.shape == (10,)
    np.testing.assert_allclose(got, track_restated(raw, F0_MIN, F0_MAX), rtol=2.0 ** -23)
    np.testing.assert_array_equal(got[[0, 1, 2, 7, 8, 9]], [120, 120, 120, 400, 100, 100])
    assert capsys.readouterr().out == ''
    # a float32 never leaves [f0_min, f0_max], whichever way the bound rounds
    edge = ops.f0_track([1.0, 1e4], 100.1, 399.9, fs, SHIFT, L)
    assert float(edge[0]) >= 100.1 and float(edge[1]) <= 399.9
    # frames beyond the waveform: centre 40 i > 100 for i >= 3
    cropped = ops.f0_track(raw, F0_MIN, F0_MAX, fs, SHIFT, L, wavlen=100)
    np.testing.assert_array_equal(cropped, got[:3])
    assert 'cropped' in capsys.readouterr().out
    assert ops.f0_track(raw, F0_MIN, F0_MAX, fs, SHIFT, L, wavlen=360).shape == (10,)          # 40 * 9 = 360 is not beyond
    for bad in ([0, 0, -1], [], [100, float('nan')], [[100, 100]]):
        with pytest.raises(ValueError):
            ops.f0_track(bad, F0_MIN, F0_MAX, fs, SHIFT, L)
    with pytest.raises(ValueError):                             # f0_max above fs/6
        ops.f0_track(raw, F0_MIN, 1400.0, fs, SHIFT, L)
    with pytest.raises(ValueError):                             # 2 int(1.5 * 8000 / 40) + 1 = 601 samples do not fit 512
        ops.f0_track(raw, 40.0, F0_MAX, fs, SHIFT, L)
    with pytest.raises(ValueError):
        ops.f0_track(raw, 200.0, 100.0, fs, SHIFT, L)
    with pytest.raises(ValueError):
        ops.f0_track(raw, F0_MIN, F0_MAX, fs, SHIFT, 500)
    with pytest.raises(ValueError):
        ops.f0_track(raw, F0_MIN, F0_MAX, fs, 0.0, L)
    assert ops.analysis_check(L, fs, SHIFT, F0_MIN, F0_MAX) == hcap_of(fs, F0_MIN) == 38
    assert ops.analysis_check(4096, 32000, SHIFT, F0_MIN, F0_MAX) == 158
    assert abs(ops.ANALYSIS_NOISY_BELOW - NOISY_BELOW) < 1e-15


def test_wavread_inverts_wavwrite(tmp_path):
    import wave
    from percivaltts_amd import vocoders
    x = 0.7 * np.sin(np.arange(500) / 11.0) * np.linspace(0, 1, 500)
    path = str(tmp_path / 'a.wav')
    vocoders.wavwrite(path, x, 8000)
    got, fs = vocoders.wavread(path)
    assert fs == 8000 and got.dtype == np.float64 and got.shape == (500,)
    assert np.abs(got - x).max() <= 0.5 / 32767.0 + 1e-12
    vocoders.wavwrite(path, np.zeros(0), 16000)
    got, fs = vocoders.wavread(path)
    assert fs == 16000 and got.shape == (0,)
    for channels, width in ((2, 2), (1, 1), (1, 4)):
        with wave.open(path, 'wb') as f:
            f.setnchannels(channels); f.setsampwidth(width); f.setframerate(8000)
            f.writeframes(b'\0' * (channels * width * 10))
        with pytest.raises(ValueError):
            vocoders.wavread(path)
    with open(path, 'wb') as f:
        f.write(b'not a wave file')
    with pytest.raises(ValueError):
        vocoders.wavread(path)


def test_interface_and_argument_checks_without_a_device(tmp_path):
    import inspect
    from percivaltts_amd import ops, vocoders
    assert list(inspect.signature(vocoders.VocoderF0Spec.compress_spectrum).parameters) == ['self', 'SPEC', 'spec_type', 'spec_size']
    assert list(inspect.signature(vocoders.VocoderPML.analysisf_device).parameters)[:8] == [
        'self', 'fwav', 'f0_in', 'ff0', 'f0_min', 'f0_max', 'fspec', 'fnm']
    voc = vocoders.VocoderPML(8000, SHIFT, 9, 9, dftlen=512)
    for gone in (voc.analysisf, voc.analysisfid, voc.synthesis):
        with pytest.raises(NotImplementedError):
            gone(None)
    world = vocoders.VocoderWORLD(8000, SHIFT, 9, 4, dftlen=512)
    assert hasattr(world, 'compress_spectrum') and not hasattr(world, 'analysis_device')
    with pytest.raises(ValueError):                             # the SPTK fit is not built
        vocoders.VocoderPML(8000, SHIFT, 9, 9, dftlen=512, spec_type='mcep').compress_spectrum(np.ones((2, 257), np.float32))
    wav, f0 = np.zeros(400), np.full(10, 150.0)
    with pytest.raises(ValueError):
        voc.analysis_device(wav, f0, F0_MIN, 2000.0)
    with pytest.raises(ValueError):
        voc.analysis_device(wav, np.zeros(10), F0_MIN, F0_MAX)
    with pytest.raises(ValueError):
        voc.analysis_device(np.zeros((2, 200)), f0, F0_MIN, F0_MAX)
    with pytest.raises(ValueError):                             # 65 noise bands over 257 bins are fine, 129 are not
        vocoders.VocoderPML(8000, SHIFT, 9, 129, dftlen=512).analysis_device(wav, f0, F0_MIN, F0_MAX)
    path = str(tmp_path / 'a.wav')
    vocoders.wavwrite(path, wav, 16000)
    out = [str(tmp_path / n) for n in ('a.lf0', 'a.spec', 'a.nm')]
    with pytest.raises(ValueError):                             # another fs: resampling is not built
        voc.analysisf_device(path, f0, out[0], F0_MIN, F0_MAX, out[1], out[2])
    vocoders.wavwrite(path, wav, 8000)
    with pytest.raises(ValueError):
        voc.analysisf_device(path, f0, out[0], F0_MIN, F0_MAX, out[1], out[2], preproc_hp='auto')
    with pytest.raises(ValueError):
        voc.analysisf_device(path, f0, out[0], F0_MIN, F0_MAX, out[1], out[2], preproc_fs=8000)
    assert not any(os.path.exists(p) for p in out)
    x = torch.zeros(4, 257)
    with pytest.raises(ValueError):
        ops.fwbnd_compress(x, 8000, 9, mode='median')
    with pytest.raises(ValueError):
        ops.fwbnd_compress(x, 8000, 200)
    with pytest.raises(ValueError):
        ops.fwbnd_compress(torch.zeros(257), 8000, 9)
    with pytest.raises(ValueError):
        ops.frame_harmonics(torch.zeros(10), torch.zeros(3), SHIFT, 8000, 500, 38)
    with pytest.raises(ValueError):
        ops.frame_harmonics(torch.zeros(10), torch.zeros(3), SHIFT, 8000, 512, 0)
    with pytest.raises(ValueError):
        ops.phase_coherence(torch.zeros(3, 38, 3), torch.zeros(3), SHIFT, 8000, 512, 9)
    with pytest.raises(ValueError):
        ops.phase_coherence(torch.zeros(3, 38, 2), torch.zeros(4), SHIFT, 8000, 512, 9)


# ---------------------------------------------------------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------------------------------------------------------
def _dev(a, dtype=torch.float32):
    return torch.tensor(np.asarray(a), dtype=dtype).cuda().contiguous()


def _harmonics(c, wav=None, T=None):
    from percivaltts_amd import ops
    f0 = c['f0'] if T is None else c['f0'][:T]
    lspec, u = ops.frame_harmonics(_dev(c['wav'] if wav is None else wav), _dev(f0), SHIFT, c['fs'], c['L'], c['hcap'], log=True)
    assert lspec.dtype == u.dtype == torch.float32 and tuple(lspec.shape) == (len(f0), c['K']) and tuple(u.shape) == (len(f0), c['hcap'], 2)
    return lspec.cpu().numpy(), u.cpu().numpy()


@pytest.mark.gpu
@pytest.mark.parametrize('name', ['A', 'B'])
def test_frame_harmonics_against_restatement(name):
    from percivaltts_amd import ops
    c = case(name)
    lspec, u = _harmonics(c)
    check(lspec, c['lspec64'], c['lspec32'], 'frame_harmonics ln SPEC ' + name)
    check(u, c['u64'], c['u32'], 'frame_harmonics phasors ' + name)
    again = _harmonics(c)
    np.testing.assert_array_equal(lspec, again[0])              # same input, same bytes
    np.testing.assert_array_equal(u, again[1])
    spec, _ = ops.frame_harmonics(_dev(c['wav']), _dev(c['f0']), SHIFT, c['fs'], c['L'], c['hcap'])
    np.testing.assert_allclose(spec.cpu().numpy(), np.exp(c['lspec64']), rtol=1e-5)
    assert np.abs(np.hypot(u[..., 0], u[..., 1])[u.any(-1)] - 1).max() < 1e-6


@pytest.mark.gpu
@pytest.mark.parametrize('what', ['T1', 'T3', 'short'])
def test_frame_harmonics_short_inputs(what):
    c = case('A')
    T = 1 if what == 'T1' else 3
    wav = c['wav'][:60] if what == 'short' else c['wav']          # 60 samples: below the 2 * 52 + 1 of the shortest window
    assert 60 < 2 * int(1.5 * c['fs'] / float(c['f0'].max())) + 1
    want = [frames_restated(wav, c['f0'][:T], SHIFT, c['fs'], c['L'], c['hcap'], dt) for dt in (np.float64, np.float32)]
    lspec, u = _harmonics(c, wav=wav, T=T)
    check(lspec, want[0][0], want[1][0], 'frame_harmonics ln SPEC A ' + what)
    check(u, want[0][1], want[1][1], 'frame_harmonics phasors A ' + what)


@pytest.mark.gpu
def test_no_frames_no_launch():
    from percivaltts_amd import _hip, ops
    with _hip.KernelTimer() as kt:
        spec, u = ops.frame_harmonics(_dev(np.zeros(10)), _dev(np.zeros(0)), SHIFT, 8000, 512, 38)
        R, nm = ops.phase_coherence(u, _dev(np.zeros(0)), SHIFT, 8000, 512, 9)
        y = ops.fwbnd_compress(spec, 8000, 9)
    assert kt.records == []
    assert tuple(spec.shape) == (0, 257) and tuple(u.shape) == (0, 38, 2) and tuple(R.shape) == (0, 38)
    assert tuple(nm.shape) == (0, 9) and tuple(y.shape) == (0, 9)
    l = _hip.lib()
    assert l.ptts_frame_harmonics(None, 0, None, None, None, 1, 38, SHIFT, 8000.0, 768, 0, None) != 0
    assert l.ptts_frame_harmonics(None, 0, None, None, None, 0, 38, SHIFT, 8000.0, 512, 0, None) == 0
    assert l.ptts_fwbnd_compress(None, None, 0, 9, 512, 2, 0, None, 0, None, 0, None) != 0
    with pytest.raises(_hip.HipLibraryError):
        ops.frame_harmonics(torch.zeros(10), _dev(np.full(3, 150.0)), SHIFT, 8000, 512, 38)


@pytest.mark.gpu
@pytest.mark.parametrize('name', ['A', 'B'])
@pytest.mark.parametrize('nb', NBS)
def test_phase_coherence_against_restatement(name, nb):
    from percivaltts_amd import ops
    c = case(name)
    u = c['u64'].astype(np.float32)
    R, nm = ops.phase_coherence(_dev(u), _dev(c['f0']), SHIFT, c['fs'], c['L'], nb)
    R, nm = R.cpu().numpy(), nm.cpu().numpy()
    assert R.shape == (c['T'], c['hcap']) and nm.shape == (c['T'], nb)
    check(R, c['R64'], c['R32'], 'phase_coherence R {} nb={}'.format(name, nb))
    e32 = float(np.abs(c['R32'].astype(np.float64) - c['R64']).max())
    bound = 4.0 * e32 + 2.0 ** -23 * float(np.abs(c['R64']).max())
    clear = [i for i in range(c['T']) if (np.abs(c['R64'][i] - NOISY_BELOW) > bound).all()]
    print('phase_coherence NM {} nb={}: {} of {} frames compared (bound {:.3e})'.format(name, nb, len(clear), c['T'], bound))
    assert len(clear) >= 0.9 * c['T']
    want = noise_bands_restated(c['R64'], c['f0'], c['fs'], c['L'], band_weights(nb, c['fs'], c['L']), np.float64)
    assert 0.05 < want.mean() < 0.95 and want.min() >= 0 and want.max() <= 1 + 1e-12
    print('phase_coherence NM {} nb={}: worst {:.3e}'.format(name, nb, np.abs(nm[clear] - want[clear]).max()))
    assert np.abs(nm[clear] - want[clear]).max() <= 1e-6
    assert nm.min() >= 0 and nm.max() <= 1


@pytest.mark.gpu
@pytest.mark.parametrize('name', ['A', 'B'])
@pytest.mark.parametrize('nb', NBS)
def test_fwbnd_compress_against_restatement(name, nb):
    from percivaltts_amd import ops
    c = case(name)
    W = band_weights(nb, c['fs'], c['L'])
    x = _dev(c['spec'])
    for mode, log, inp in (('mean', False, c['spec']), ('lsq', False, c['spec']), ('lsq', True, c['lspec64'].astype(np.float32))):
        got = ops.fwbnd_compress(_dev(inp), c['fs'], nb, mode=mode, log=log)
        assert tuple(got.shape) == (c['T'], nb)
        want64 = compress_restated(inp, W, mode, log, np.float64)
        want32 = compress_restated(inp, W, mode, log, np.float32)
        check(got.cpu().numpy(), want64, want32, 'fwbnd_compress {} log={} {} nb={}'.format(mode, int(log), name, nb))
    got3 = ops.fwbnd_compress(x.view(2, c['T'] // 2, c['K']), c['fs'], nb)
    np.testing.assert_array_equal(got3.view(c['T'], nb).cpu().numpy(), ops.fwbnd_compress(x, c['fs'], nb).cpu().numpy())


@pytest.mark.gpu
@pytest.mark.parametrize('name', ['A', 'B'])
@pytest.mark.parametrize('nb', NBS)
def test_compress_spectrum_inverts_decompress_spectrum(name, nb):
    from percivaltts_amd import vocoders
    c = case(name)
    voc = vocoders.VocoderPML(c['fs'], SHIFT, nb, 9, dftlen=c['L'])
    y = (np.random.RandomState(7).randn(c['T'], nb) * 1.5 - 4.0).astype(np.float32)
    S = voc.decompress_spectrum(y)                              # numpy in, numpy out
    assert S.shape == (c['T'], c['K'])
    got = voc.compress_spectrum(S)
    assert isinstance(got, np.ndarray) and got.dtype == np.float32
    W = band_weights(nb, c['fs'], c['L'])
    want64 = compress_restated(S, W, 'lsq', False, np.float64)
    want32 = compress_restated(S, W, 'lsq', False, np.float32)
    check(got, want64, want32, 'compress_spectrum {} nb={}'.format(name, nb))
    e32 = float(np.abs(want32.astype(np.float64) - want64).max())
    bound = 4.0 * e32 + 2.0 ** -23 * float(np.abs(y).max())
    S2 = voc.decompress_spectrum(got)
    print('compress(decompress(y)) - y: worst {:.3e}, bound {:.3e}'.format(np.abs(got - y).max(), bound))
    assert np.abs(got.astype(np.float64) - y).max() <= bound    # the band values come back ...
    np.testing.assert_allclose(S2, S, rtol=2 * bound + 2.0 ** -22)        # ... and so does the envelope they stand for
    dev = voc.compress_spectrum(_dev(S), 'fwbnd', nb)
    assert torch.is_tensor(dev) and dev.is_cuda
    np.testing.assert_array_equal(dev.cpu().numpy(), got)


@pytest.mark.gpu
def test_round_trip_synthesis_then_analysis():
    """ops.pulse_synthesis on the known envelope of shape B, then ops.frame_harmonics: the envelope comes back as well as it does
    between the two float64 restatements (0.46 dB rms over the voiced band) -- at most 10 % worse, since both
    run the same definitions and float32 storage adds far less than the definition's own interpolation error."""
    from percivaltts_amd import ops
    c = case('B')
    cpu = envelope_rms_db(c['lspec64'], c)
    tab = ops.pulse_table(c['f0'], SHIFT, c['fs'], c['wavlen'], c['L'])
    wav = ops.pulse_synthesis(_dev(c['spec']), _dev(c['mask']), tab, _dev(c['g']), c['fs'], c['L'], c['wavlen'])
    lspec, _ = ops.frame_harmonics(wav, _dev(c['f0']), SHIFT, c['fs'], c['L'], c['hcap'], log=True)
    gpu = envelope_rms_db(lspec.cpu().numpy(), c)
    print('round trip B: {:.4f} dB rms on the device, {:.4f} dB between the float64 restatements'.format(gpu, cpu))
    assert gpu <= 1.1 * cpu


@pytest.mark.gpu
def test_analysis_device_and_files(tmp_path):
    from percivaltts_amd import ops, vocoders
    c = case('A')
    voc = vocoders.VocoderPML(c['fs'], SHIFT, 9, 9, dftlen=c['L'])
    f0 = c['f0'].copy()
    f0[5:8] = 0.0                                               # an unvoiced stretch
    CMP = voc.analysis_device(c['wav64'], f0, F0_MIN, F0_MAX)
    T = c['T']                                                  # the last centre is the sample behind the end: not beyond
    assert CMP.shape == (T, voc.featuressizeraw()) and CMP.dtype == np.float32 and np.isfinite(CMP).all()
    track = ops.f0_track(f0, F0_MIN, F0_MAX, c['fs'], SHIFT, c['L'])
    np.testing.assert_allclose(CMP[:, 0], np.log(track.astype(np.float64)), rtol=1e-6)
    # the chain of the public ops, byte for byte
    w, f = _dev(c['wav64']), _dev(track)
    lspec, u = ops.frame_harmonics(w, f, SHIFT, c['fs'], c['L'], c['hcap'], log=True)
    np.testing.assert_array_equal(CMP[:, 1:10], ops.fwbnd_compress(lspec, c['fs'], 9, log=True).cpu().numpy())
    np.testing.assert_array_equal(CMP[:, 10:], ops.phase_coherence(u, f, SHIFT, c['fs'], c['L'], 9)[1].cpu().numpy())
    assert CMP[:, 10:].min() >= 0 and CMP[:, 10:].max() <= 1 and CMP[2:-2, -1].mean() > 0.5 and CMP[2:-2, 10].mean() < 0.2
    # from file to files
    path = str(tmp_path / 'wav' / 'a.wav')
    os.makedirs(os.path.dirname(path))
    vocoders.wavwrite(path, c['wav64'], c['fs'])
    f0.astype(np.float32).tofile(str(tmp_path / 'a.f0'))
    outs = {'f0': str(tmp_path / 'lf0' / '*.lf0'), 'spec': str(tmp_path / 'spec' / '*.spec'), 'noise': str(tmp_path / 'nm' / '*.nm')}
    assert voc.analysisfid_device('a', str(tmp_path / 'wav' / '*.wav'), str(tmp_path / '*.f0'), F0_MIN, F0_MAX, outs) == T
    lf0 = np.fromfile(outs['f0'].replace('*', 'a'), dtype=np.float32)
    spec = np.fromfile(outs['spec'].replace('*', 'a'), dtype=np.float32)
    nm = np.fromfile(outs['noise'].replace('*', 'a'), dtype=np.float32)
    assert lf0.shape == (T,) and spec.shape == (T * 9,) and nm.shape == (T * 9,)
    np.testing.assert_array_equal(lf0, CMP[:, 0])
    back = voc.analysis_device(vocoders.wavread(path)[0], f0, F0_MIN, F0_MAX)      # the waveform went through 16 bits
    np.testing.assert_array_equal(np.concatenate([lf0[:, None], spec.reshape(T, 9), nm.reshape(T, 9)], axis=1), back)
    with pytest.raises(NotImplementedError):
        voc.analysisf(path, outs['f0'], F0_MIN, F0_MAX, outs['spec'], outs['noise'])


@pytest.mark.gpu
def test_features_extraction_on_a_synthetic_corpus(tmp_path, monkeypatch):
    """Three utterances from .wav and an F0 track to the composed outputs and the weights that training reads."""
    import importlib
    from percivaltts_amd import vocoders
    monkeypatch.setenv('PERCIVAL_CORPUS', str(tmp_path / 'corpus'))
    monkeypatch.chdir(tmp_path)
    import percivaltts_amd.run as run
    run = importlib.reload(run)
    run.cfg.id_valid_start = 2
    fs, voc = run.cfg.vocoder_fs, run.vocoder
    fids, lens = ['utt_a', 'utt_b', 'utt_c'], [31, 24, 40]
    os.makedirs(str(tmp_path / 'corpus' / 'wav'))
    os.makedirs(str(tmp_path / 'corpus' / 'f0'))
    rng = np.random.RandomState(11)
    for fid, T in zip(fids, lens):
        N = int(round(SHIFT * (T - 1) * fs))
        f0 = 150.0 + 40.0 * np.sin(np.arange(T) / 5.0 + rng.rand())
        phase = 2 * np.pi * np.cumsum(np.interp(np.arange(N) / float(fs), SHIFT * np.arange(T), f0)) / fs
        wav = 0.1 * sum(np.cos(h * phase) / h for h in range(1, 20)) + 0.01 * rng.randn(N)
        vocoders.wavwrite(str(tmp_path / 'corpus' / 'wav' / (fid + '.wav')), wav, fs)
        f0[:2] = 0.0
        f0.astype(np.float32).tofile(str(tmp_path / 'corpus' / 'f0' / (fid + '.f0')))
    with open(run.cfg.fileids, 'w') as f:
        f.write('\n'.join(fids) + '\n')
    run.features_extraction(str(tmp_path / 'corpus' / 'f0' / '*.f0'))
    nout = voc.featuressize()
    for fid, T in zip(fids, lens):
        cmp = np.fromfile(run.cfg.outpath.split(':')[0].replace('*', fid), dtype=np.float32)
        w = np.fromfile(run.cfg.wpath.split(':')[0].replace('*', fid), dtype=np.float32)
        assert cmp.shape == (T * nout,) and np.isfinite(cmp).all() and w.shape == (T,)
        lf0 = np.fromfile(str(tmp_path / 'corpus' / ('wav_PML_lf0/' + fid + '.lf0')), dtype=np.float32)
        assert lf0.shape == (T,) and (np.exp(lf0) > 100).all() and (np.exp(lf0) < 200).all()
    for stat in ('mean4norm.dat', 'std4norm.dat'):
        assert os.path.getsize(os.path.join(os.path.dirname(run.cfg.outpath), stat)) == 4 * nout
