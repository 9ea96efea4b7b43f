"""Waveform analysis for the WORLD parameters (csrc/worldanalysis.hip; ops.world_analysis_check / world_envelope /
world_aperiodicity, VocoderWORLDAnalysisDevice.analysis_device / analysisf_device / analysisfid_device / write_streams,
run.features_extraction with a WORLD vocoder).

The reference calls pyworld, which is not part of this build, so there is nothing of it to compare numbers with: the definition is
the build's own (the envelope after CheapTrick, the aperiodicity from two windows one period apart) and is
restated here in numpy, in a chosen dtype.  The transform of a frame is torch.fft.rfft, which keeps the dtype.  Integer decisions
(sample and bin indices, window lengths, which bins lie below f0) are taken in float64 from the float32 inputs in both dtypes, as
the kernels take them.

Tolerance of the device results: the rule of tests/test_pulsesynth.py (`check` in tests/test_worldsynth.py).  The yardstick is the
restatement in float64; the same restatement in float32 has a largest error e32 against it on the same input; every element of a
device result has to lie within 4 * e32 + 2^-23 * max|want64| of the float64 value.

The test signals are the float64 synthesis restatement of tests/test_worldsynth.py (synth_restated)."""
import inspect
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_analysis as ta                                      # noqa: E402  (band_weights, compress_restated)
import test_worldsynth as ws                                    # noqa: E402  (the synthesis restatement, `check`, the two shapes)

check, rnd = ws.check, ws.rnd
SHIFT, SHAPES = ws.SHIFT, ws.SHAPES
F0_MIN, F0_MAX = 100.0, 400.0
UNVOICED_RATE = 500.0
Q1 = -0.15
DB = 20.0 / math.log(10.0)
_weights = {}


# ---------------------------------------------------------------------------------------------------------------------------
# the definition, restated
# ---------------------------------------------------------------------------------------------------------------------------
def band_weights(nb, fs, L):
    key = (nb, fs, L)
    if key not in _weights:
        _weights[key] = ta.band_weights(nb, fs, L)
        _weights[key].setflags(write=False)
    return _weights[key]


def window_restated(hw, dtype):
    """w_j = 0.5 + 0.5 cos(pi j / (hw + 1)), j = -hw .. hw, scaled by 1 / sqrt(0.75 (hw + 1)): unit energy."""
    j = np.arange(-hw, hw + 1)
    return ((0.5 + 0.5 * np.cos(np.pi * j / (hw + 1.0))) / np.sqrt(0.75 * (hw + 1))).astype(dtype)


def frame_restated(wav, c, hw, L, dtype):
    """rfft of the windowed frame around sample c, zero-phase placement; samples outside the waveform count as 0."""
    j = np.arange(-hw, hw + 1)
    ok = (c + j >= 0) & (c + j < len(wav))
    x = np.zeros(L, dtype=dtype)
    x[j[ok] % L] = wav[c + j[ok]] * window_restated(hw, dtype)[ok]
    X = torch.fft.rfft(torch.from_numpy(x)).numpy()
    assert X.dtype == (np.complex128 if dtype == np.float64 else np.complex64)
    return X


def envelope_restated(wav, rate, shift, fs, L, dtype):
    """wav [N], rate [T] -> ln SPEC [T,K] in `dtype`."""
    dt = np.dtype(dtype).type
    ctype = torch.complex128 if dtype == np.float64 else torch.complex64
    wav = np.asarray(wav, dtype=dtype)
    T, M, K = len(rate), L // 2, L // 2 + 1
    ks = np.arange(K)
    q = np.minimum(np.arange(L), L - np.arange(L))
    lspec = np.zeros((T, K), dtype=dtype)
    for i in range(T):
        r = float(rate[i])
        X = frame_restated(wav, rnd(i * shift * fs), int(1.5 * fs / r), L, dtype)
        P0 = X.real ** 2 + X.imag ** 2
        # the DC correction: the uncorrected spectrum mirrored around kappa / 2
        kappa = r * L / fs
        low = ks[ks < kappa]
        y = kappa - low
        j = np.minimum(y.astype(np.int64), M - 1)
        P = P0.copy()
        P[low] += P0[j] + (y - j).astype(dtype) * (P0[j + 1] - P0[j])
        # the mean over [k - d, k + d] of the piecewise constant spectrum, mirrored at 0 and at M
        d = r * L / (3.0 * fs)
        lo, hi = ks - d, ks + d
        jlo, jhi = np.floor(lo + 0.5).astype(np.int64), np.floor(hi + 0.5).astype(np.int64)
        t = np.arange(int((jhi - jlo).max()) + 1)[None, :]
        idx = jlo[:, None] + t
        wts = np.where(idx <= jhi[:, None], 1.0, 0.0)
        wts[:, 0] = (jlo + 0.5) - lo
        last = (jhi - jlo)
        wts[ks, last] = np.where(last > 0, hi - (jhi - 0.5), hi - lo)
        m = np.abs(idx)
        m = np.where(m > M, 2 * M - m, m)
        S = (P[np.clip(m, 0, M)] * wts.astype(dtype)).sum(1) / dt(2.0 * d)
        la = np.log(np.maximum(np.sqrt(S * dt(fs) / dt(r)), dt(1e-10)))
        assert la.dtype == dtype
        # the lifter that undoes the smoothing at the harmonics
        cep = torch.fft.irfft(torch.from_numpy(la).to(ctype), n=L).numpy()
        x = (r * q / fs).astype(dtype)
        g = np.sinc(x) * (dt(1.0 - 2.0 * Q1) + dt(2.0 * Q1) * np.cos(dt(2.0 * np.pi) * x))
        lspec[i] = torch.fft.rfft(torch.from_numpy((cep * g).astype(dtype))).numpy().real
    return lspec


def aperiodicity_restated(wav, f0, voiced, shift, fs, L, nb, dtype):
    """wav [N], f0 [T], voiced [T] -> (rho [T,nb], the ratio before the clip, 1 in unvoiced frames; aper [T,nb] in dB) in `dtype`."""
    dt = np.dtype(dtype).type
    wav = np.asarray(wav, dtype=dtype)
    T, K = len(f0), L // 2 + 1
    ks = np.arange(K)
    W = band_weights(nb, fs, L)
    rho = np.ones((T, nb), dtype=dtype)
    for i in range(T):
        if not voiced[i]:
            continue
        f0i = float(f0[i])
        T0 = fs / f0i
        n0 = rnd(T0)
        delta = T0 - n0
        c1 = rnd(i * shift * fs) - (n0 >> 1)
        hw = int(1.5 * fs / f0i)
        X1 = frame_restated(wav, c1, hw, L, dtype)
        X2 = frame_restated(wav, c1 + n0, hw, L, dtype) * np.exp(2j * np.pi * ks * delta / L).astype(X1.dtype)
        D = (np.abs(X1 - X2) ** 2 / 2).astype(dtype)
        E = ((np.abs(X1) ** 2 + np.abs(X2) ** 2) / 2).astype(dtype)
        Wm = (W * (ks >= f0i * L / fs)[:, None]).astype(dtype)          # bins below f0 carry no weight
        num, den = Wm.T.dot(D), Wm.T.dot(E)
        for b in range(nb - 1, -1, -1):                         # a band without weight: the nearest band above that has some
            rho[i, b] = num[b] / den[b] if den[b] > 0 else (rho[i, b + 1] if b + 1 < nb else dt(1))     # none above: 0 dB
    assert rho.dtype == dtype
    return rho, (dt(10) * np.log10(np.clip(rho, dt(1e-6), dt(1)))).astype(dtype)


# ---------------------------------------------------------------------------------------------------------------------------
# signals with known parameters, computed once
# ---------------------------------------------------------------------------------------------------------------------------
_signals = {}


def signal(kind, fs=16000, L=2048, T=161, f0=200.0):
    """A waveform of the float64 synthesis restatement with a constant f0, a smooth envelope that does not move, and one row of
    aperiodicity bands: 'periodic' -200 dB, 'noise' 0 dB, 'mixed' -30 / -24 / -14 / -8 / -3 dB; 'unvoiced': every frame unvoiced,
    so that the synthesiser runs at its 500 Hz rate and the aperiodicity bands are not looked at."""
    key = (kind, fs, L, T, f0)
    if key not in _signals:
        bands = {'periodic': [-200.0] * 5, 'noise': [0.0] * 5, 'mixed': [-30.0, -24.0, -14.0, -8.0, -3.0],
                 'unvoiced': [-20.0] * 5}[kind]
        K = L // 2 + 1
        rng = np.random.RandomState(3)
        x = np.linspace(0, 1, K)
        la = sum(rng.randn() * np.cos(np.pi * j * x + rng.rand() * 6.28) / j for j in range(1, 6))
        la = -7.0 + 4.0 * (la - la.min()) / (la.max() - la.min())
        spec = np.tile(np.exp(la), (T, 1)).astype(np.float32)
        f0v = np.full(T, f0, dtype=np.float32)
        voiced = np.full(T, kind != 'unvoiced')
        aper_db = np.tile(np.array(bands, dtype=np.float32), (T, 1))
        aper = ws.aper_restated(aper_db, voiced.astype(np.float64), fs, L, np.float64).astype(np.float32)
        wavlen = ws.wavlen_of(T, fs)
        g = rng.randn(wavlen).astype(np.float32)
        rows = ws.table_restated(f0v, voiced, SHIFT, fs, wavlen, L)[1]
        wav = ws.synth_restated(spec, aper, g, rows, fs, L, wavlen, torch.float64)
        # interior frames: both windows of the aperiodicity (within 2 hw of the centre) lie where every pulse that reaches them
        # exists (a pulse's segment spans 50 ms; those before t = 0 and behind the end are not synthesised)
        hw, seg = int(1.5 * fs / f0), int(0.05 * fs)
        inner = [i for i in range(T) if rnd(i * SHIFT * fs) - 2 * hw >= seg and rnd(i * SHIFT * fs) + 2 * hw < wavlen - seg]
        c = dict(fs=fs, L=L, T=T, K=K, f0=f0v, voiced=voiced, spec=spec, aper_db=aper_db, wav=wav, inner=inner)
        for v in c.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _signals[key] = c
    return _signals[key]


def envelope_error_db(lspec, c, frames=None):
    """(rms, mean) over the given frames (the interior ones) and the bins at and above f0 of 20 log10(analysed / known)."""
    f = np.arange(c['K']) * float(c['fs']) / c['L']
    err = []
    for i in (c['inner'] if frames is None else frames):
        sel = f >= float(c['f0'][i])
        err.append(DB * (np.asarray(lspec[i], dtype=np.float64)[sel] - np.log(c['spec'][i].astype(np.float64))[sel]))
    err = np.concatenate(err)
    return float(np.sqrt(np.mean(err ** 2))), float(err.mean())


def analysed(kind):
    c = signal(kind)
    if 'lspec' not in c:
        c['lspec'] = envelope_restated(c['wav'], c['f0'], SHIFT, c['fs'], c['L'], np.float64)
        c['rho'], c['db'] = aperiodicity_restated(c['wav'], c['f0'], c['voiced'], SHIFT, c['fs'], c['L'], 5, np.float64)
    return c


# ---------------------------------------------------------------------------------------------------------------------------
# CPU: the restatement's properties
# ---------------------------------------------------------------------------------------------------------------------------
def test_restated_window_has_unit_energy():
    for hw in (1, 7, 60, 480):
        w = window_restated(hw, np.float64)
        assert len(w) == 2 * hw + 1 and abs(float((w ** 2).sum()) - 1.0) < 1e-12


def test_restated_periodic_input():
    """Aperiodicity -200 dB in every band, f0 = 200 Hz, fs 16 kHz, L 2048, the 134 interior frames.  Measured on this restatement:
    the envelope at and above f0 is off by 0.170 dB rms, -0.152 dB in the mean (the gain convention sqrt(S fs / f0) holds), and
    the largest rho is 1.2e-14: every band sits at the -60 dB floor.  The bounds are twice the rms figures; rho <= 1e-12."""
    c = analysed('periodic')
    rms, mean = envelope_error_db(c['lspec'], c)
    rho = c['rho'][c['inner']]
    print('periodic: envelope error above f0 {:.3f} dB rms, mean {:+.3f} dB; largest rho {:.3e}'.format(rms, mean, rho.max()))
    assert rms <= 2 * 0.170 and abs(mean) <= 2 * 0.152
    assert rho.max() <= 1e-12 and (c['db'][c['inner']] == -60.0).all()


def test_restated_noise_input():
    """Aperiodicity 0 dB in every band: noise alone.  Measured on this restatement: band medians 0 / 0 / 0 / -0.09 / -0.06 dB; the
    envelope at and above f0 is off by 4.14 dB rms, -1.43 dB in the mean, which is the variance of a single frame's periodogram
    (ln of a chi-square with few degrees of freedom), not bias in the definition.  The bounds: twice the rms, 2 dB below the lowest
    median."""
    c = analysed('noise')
    rms, mean = envelope_error_db(c['lspec'], c)
    med = np.median(c['db'][c['inner']], axis=0)
    print('noise: envelope error above f0 {:.3f} dB rms, mean {:+.3f} dB; band medians {}'.format(rms, mean, np.round(med, 2)))
    assert rms <= 2 * 4.144
    assert (med <= 0).all() and (med >= -0.09 - 2.0).all()


MIXED_MEDIANS = (-27.29, -22.30, -13.51, -3.81, -3.74)


def test_restated_mixed_input():
    """Bands at -30 / -24 / -14 / -8 / -3 dB.  Measured on this restatement: medians -27.29 / -22.30 / -13.51 / -3.81 / -3.74 dB,
    interquartile ranges 4.3 / 1.7 / 1.3 / 2.1 / 2.8 dB: monotone above the first band (which lies at 0 Hz, below f0, hence the
    rule that bins below f0 carry no weight) and within 4.2 dB of what went in.  It is a power-weighted estimate over a band's
    bins, not an exact inverse of the synthesiser's interpolation between the bands.  The medians have to stay within 2 dB of the
    measured ones."""
    c = analysed('mixed')
    db = c['db'][c['inner']]
    med = np.median(db, axis=0)
    iqr = np.percentile(db, 75, axis=0) - np.percentile(db, 25, axis=0)
    print('mixed: band medians {}, interquartile ranges {}'.format(np.round(med, 2), np.round(iqr, 2)))
    assert (np.diff(med[1:]) > 0).all()                        # monotone above the first band, which lies at 0 Hz, below f0
    assert (np.abs(med - np.array(MIXED_MEDIANS)) <= 2.0).all()


def test_restated_all_unvoiced_track():
    """Every frame unvoiced: the aperiodicity rows are exactly 0 dB whatever f0 says, and the envelope is the one of the 500 Hz
    rate (another rate gives another window, hence another envelope).  The signal is the synthesiser's own unvoiced output, noise
    in 2-ms pieces: analysed at 500 Hz its known envelope comes back within 3.78 dB rms, -1.04 dB in the mean, as measured on this
    restatement (the periodogram's variance again; the gain fs / rate holds for the unvoiced rate too); the bound is twice the rms.
    Analysed at a voiced signal's 200 Hz instead, the mean would be off by 10 log10(200 / 500) = -4 dB."""
    c = signal('unvoiced', T=41)
    T, wav, f0 = c['T'], c['wav'], c['f0']
    assert not c['voiced'].any()
    rho, db = aperiodicity_restated(wav, f0, c['voiced'], SHIFT, c['fs'], c['L'], 5, np.float64)
    assert (db == 0.0).all() and (rho == 1.0).all()
    rate = np.full(T, UNVOICED_RATE, dtype=np.float32)
    a = envelope_restated(wav, rate, SHIFT, c['fs'], c['L'], np.float64)
    assert np.isfinite(a).all()
    hw = int(1.5 * c['fs'] / UNVOICED_RATE)
    X = frame_restated(wav, rnd(5 * SHIFT * c['fs']), hw, c['L'], np.float64)
    assert hw == 48 and np.abs(X).max() > 0
    b = envelope_restated(wav, f0, SHIFT, c['fs'], c['L'], np.float64)
    assert np.abs(a[2:-2] - b[2:-2]).max() > 0.1
    # the synthesiser's noise in 2-ms pieces comes back under the gain of the 500 Hz rate
    rms, mean = envelope_error_db(a, dict(c, f0=rate))
    print('all unvoiced: envelope error above 500 Hz {:.3f} dB rms, mean {:+.3f} dB'.format(rms, mean))
    assert rms <= 2 * 3.779


def test_world_analysis_check():
    from percivaltts_amd import ops
    ops.world_analysis_check(512, 8000, SHIFT, F0_MIN, F0_MAX)
    ops.world_analysis_check(8192, 32000, SHIFT, 60.0, 400.0)
    for dftlen in (500, 768, 128, 16384):                      # not a power of two, out of range
        with pytest.raises(ValueError):
            ops.world_analysis_check(dftlen, 8000, SHIFT, F0_MIN, F0_MAX)
    with pytest.raises(ValueError):                             # f0_max above fs / 6
        ops.world_analysis_check(512, 8000, SHIFT, F0_MIN, 1400.0)
    with pytest.raises(ValueError):                             # 2 int(1.5 * 8000 / 40) + 1 = 601 samples do not fit 512
        ops.world_analysis_check(512, 8000, SHIFT, 40.0, F0_MAX)
    with pytest.raises(ValueError):                             # the window at 500 Hz: 2 int(1.5 * 48000 / 500) + 1 = 289 > 256
        ops.world_analysis_check(256, 48000, SHIFT, 600.0, 800.0)
    ops.world_analysis_check(512, 48000, SHIFT, 600.0, 800.0)
    with pytest.raises(ValueError):
        ops.world_analysis_check(512, 8000, 0.0, F0_MIN, F0_MAX)
    with pytest.raises(ValueError):
        ops.world_analysis_check(512, 8000, SHIFT, 300.0, 200.0)


def test_interface_without_a_device():
    from percivaltts_amd import ops, ops_offline, vocoders
    assert list(inspect.signature(ops.world_analysis_check).parameters) == ['dftlen', 'fs', 'shift', 'f0_min', 'f0_max']
    assert list(inspect.signature(ops.world_envelope).parameters) == ['wav', 'rate', 'shift', 'fs', 'dftlen', 'log']
    assert inspect.signature(ops.world_envelope).parameters['log'].default is False
    assert list(inspect.signature(ops.world_aperiodicity).parameters) == ['wav', 'f0', 'voiced', 'shift', 'fs', 'dftlen', 'nb']
    for name in ('world_analysis_check', 'world_envelope', 'world_aperiodicity'):
        assert getattr(ops, name) is getattr(ops_offline, name) and name in ops_offline.__all__
    cls = vocoders.VocoderWORLDAnalysisDevice
    assert issubclass(cls, vocoders.VocoderWORLDDevice)
    assert list(inspect.signature(cls.analysis_device).parameters) == ['self', 'wav', 'f0', 'f0_min', 'f0_max']
    assert list(inspect.signature(cls.write_streams).parameters) == ['self', 'CMP', 'ff0', 'fspec', 'faper', 'fvuv']
    assert list(inspect.signature(cls.analysisf_device).parameters) == [
        'self', 'fwav', 'f0_in', 'ff0', 'f0_min', 'f0_max', 'fspec', 'faper', 'fvuv', 'kwargs']
    assert list(inspect.signature(cls.analysisfid_device).parameters) == [
        'self', 'fid', 'wav_path', 'f0in_path', 'f0_min', 'f0_max', 'outputpathdicts', 'kwargs']
    voc = cls(8000, SHIFT, 9, 4, dftlen=512)
    assert isinstance(voc, vocoders.VocoderWORLD) and voc.name() == 'WORLD' and voc.featuressizeraw() == 1 + 9 + 4 + 1
    assert cls.synthesis_device is vocoders.VocoderWORLDDevice.synthesis_device
    assert not hasattr(vocoders.VocoderWORLDDevice(8000, SHIFT, 9, 4, dftlen=512), 'analysis_device')
    assert not hasattr(vocoders.VocoderWORLD(8000, SHIFT, 9, 4, dftlen=512), 'analysis_device')
    for gone in (voc.analysisf, voc.analysisfid, voc.synthesis):
        with pytest.raises(NotImplementedError):
            gone(None)
    wav, f0 = np.zeros(400), np.full(10, 150.0)
    with pytest.raises(ValueError):
        voc.analysis_device(wav, f0, F0_MIN, 2000.0)
    with pytest.raises(ValueError):
        voc.analysis_device(wav, np.zeros(10), F0_MIN, F0_MAX)
    with pytest.raises(ValueError):
        voc.analysis_device(np.zeros((2, 200)), f0, F0_MIN, F0_MAX)
    x = torch.zeros(10)
    with pytest.raises(ValueError):
        ops.world_envelope(x, torch.zeros(3), SHIFT, 8000, 500)
    with pytest.raises(ValueError):
        ops.world_envelope(torch.zeros(2, 5), torch.zeros(3), SHIFT, 8000, 512)
    with pytest.raises(ValueError):
        ops.world_envelope(x, torch.zeros(3, 1), SHIFT, 8000, 512)
    with pytest.raises(ValueError):
        ops.world_envelope(x, torch.zeros(3, requires_grad=True), SHIFT, 8000, 512)
    with pytest.raises(ValueError):
        ops.world_aperiodicity(x, torch.zeros(3), torch.zeros(4), SHIFT, 8000, 512, 5)
    with pytest.raises(ValueError):
        ops.world_aperiodicity(x, torch.zeros(3), torch.zeros(3), 0.0, 8000, 512, 5)


def test_write_streams(tmp_path):
    from percivaltts_amd import vocoders
    voc = vocoders.VocoderWORLDAnalysisDevice(8000, SHIFT, 9, 4, dftlen=512)
    T = 7
    CMP = np.random.RandomState(0).randn(T, voc.featuressizeraw())
    CMP[:, -1] = np.arange(T) % 2
    paths = [str(tmp_path / d / ('a.' + d)) for d in ('lf0', 'spec', 'aper', 'vuv')]
    assert voc.write_streams(CMP, *paths) == T
    got = [np.fromfile(p, dtype=np.float32) for p in paths]
    assert [os.path.getsize(p) for p in paths] == [4 * T, 4 * T * 9, 4 * T * 4, 4 * T]
    back = np.concatenate([got[0][:, None], got[1].reshape(T, 9), got[2].reshape(T, 4), got[3][:, None]], axis=1)
    np.testing.assert_array_equal(back, CMP.astype(np.float32))
    assert voc.write_streams(back, *paths) == T                 # the directories exist now
    np.testing.assert_array_equal(np.fromfile(paths[2], dtype=np.float32), got[2])


def test_features_extraction_default_world_paths(tmp_path, monkeypatch):
    import importlib
    from percivaltts_amd import vocoders
    monkeypatch.setenv('PERCIVAL_CORPUS', str(tmp_path / 'corpus'))
    monkeypatch.chdir(tmp_path)
    import percivaltts_amd.run as run
    run = importlib.reload(run)
    fs = run.cfg.vocoder_fs
    os.makedirs(str(tmp_path / 'corpus' / 'wav'))
    vocoders.wavwrite(str(tmp_path / 'corpus' / 'wav' / 'a.wav'), np.zeros(100), fs)
    calls = []
    monkeypatch.setattr(run, 'features_compose', lambda rawpaths, fids=None, win_convention='mlpg': calls.append(('compose', list(rawpaths), fids)))
    base = str(tmp_path / 'corpus') + '/wav'
    # a PML vocoder: nothing changes
    monkeypatch.setattr(run.vocoder, 'analysisfid_device', lambda *a, **k: calls.append(('pml', a, k)), raising=False)
    run.features_extraction(fids=['a'])
    assert calls[0][0] == 'pml' and calls[0][1][5] == {'f0': base + '_PML_lf0/*.lf0', 'spec': base + '_PML_fwlspec129/*.fwlspec',
                                                       'noise': base + '_PML_fwnm33/*.fwnm'}
    assert calls[1] == ('compose', [base + '_PML_lf0/*.lf0', base + '_PML_fwlspec129/*.fwlspec', base + '_PML_fwnm33/*.fwnm'], ['a'])
    # a WORLD vocoder without an analysis is refused as before
    run.vocoder = vocoders.VocoderWORLDDevice(fs, SHIFT, 65, 17)
    with pytest.raises(ValueError):
        run.features_extraction(fids=['a'])
    # the WORLD vocoder with one: the reference's places, four streams
    del calls[:]
    run.vocoder = vocoders.VocoderWORLDAnalysisDevice(fs, SHIFT, 65, 17)
    monkeypatch.setattr(run.vocoder, 'analysisfid_device', lambda *a, **k: calls.append(('world', a, k)), raising=False)
    run.features_extraction('f0/*.f0', fids=['a'], f0_min=80, f0_max=500)
    want = [base + '_WORLD_lf0/*.lf0', base + '_WORLD_fwlspec65/*.fwlspec', base + '_WORLD_fwdbap17/*.fwdbap', base + '_WORLD_vuv1/*.vuv']
    assert calls[0] == ('world', ('a', base + '/*.wav', 'f0/*.f0', 80, 500, dict(zip(('f0', 'spec', 'noise', 'vuv'), want))), {})
    assert calls[1] == ('compose', want, ['a'])
    # a caller's paths
    del calls[:]
    mine = ['x/*.lf0', 'y/*.spec', 'z/*.ap', 'v/*.vuv']
    run.features_extraction(None, rawpaths=mine, fids=['a'])
    assert calls[0][1][5] == dict(zip(('f0', 'spec', 'noise', 'vuv'), mine)) and calls[1][1] == mine
    importlib.reload(run)


# ---------------------------------------------------------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------------------------------------------------------
_cases = {}


def _dev(a, dtype=torch.float32):
    return torch.tensor(np.asarray(a), dtype=dtype).cuda().contiguous()


def references(wav, f0, voiced, fs, L, nb):
    """The restatement in both dtypes on the float32 values a kernel is given."""
    wav, f0 = np.asarray(wav, dtype=np.float32), np.asarray(f0, dtype=np.float32)
    rate = np.where(voiced, f0, np.float32(UNVOICED_RATE)).astype(np.float32)
    c = dict(wav=wav, f0=f0, voiced=np.asarray(voiced, dtype=bool), rate=rate, fs=fs, L=L, nb=nb, T=len(f0), K=L // 2 + 1)
    for tag, dtype in (('64', np.float64), ('32', np.float32)):
        c['lspec' + tag] = envelope_restated(wav, rate, SHIFT, fs, L, dtype)
        c['rho' + tag], c['db' + tag] = aperiodicity_restated(wav, f0, c['voiced'], SHIFT, fs, L, nb, dtype)
    for v in c.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return c


def case(name):
    """The waveform of test_worldsynth's shape, its f0 track and voicing, nb = 5 bands."""
    if name not in _cases:
        s = ws.case(name)
        _cases[name] = references(s['wav64'], s['f0'], s['voiced'], s['fs'], s['L'], 5)
    return _cases[name]


def _envelope(c, log=True):
    from percivaltts_amd import ops
    out = ops.world_envelope(_dev(c['wav']), _dev(c['rate']), SHIFT, c['fs'], c['L'], log=log)
    assert out.dtype == torch.float32 and out.is_cuda and tuple(out.shape) == (c['T'], c['K'])
    return out.cpu().numpy()


def _aperiodicity(c):
    from percivaltts_amd import ops
    out = ops.world_aperiodicity(_dev(c['wav']), _dev(c['f0']), _dev(c['voiced'].astype(np.float32)), SHIFT, c['fs'], c['L'], c['nb'])
    assert out.dtype == torch.float32 and out.is_cuda and tuple(out.shape) == (c['T'], c['nb'])
    return out.cpu().numpy()


def _check_both(c, what):
    lspec = _envelope(c)
    check(lspec, c['lspec64'], c['lspec32'], 'world_envelope ln SPEC ' + what)
    check(_envelope(c, log=False), np.exp(c['lspec64']), np.exp(c['lspec32'].astype(np.float32)), 'world_envelope SPEC ' + what)
    db = _aperiodicity(c)
    check(db, c['db64'], c['db32'], 'world_aperiodicity dB ' + what)
    assert db.min() >= -60.0 and db.max() <= 0.0 and (db[~c['voiced']] == 0.0).all()
    return lspec, db


@pytest.mark.gpu
@pytest.mark.parametrize('name', ['A', 'B'])
def test_kernels_against_restatement(name):
    """Both kernels on the waveform of test_worldsynth's shapes.  The aperiodicity is compared in dB: on these signals rho lies
    far above the 1e-6 floor in most bands, and e32 is printed by `check`."""
    c = case(name)
    assert (~c['voiced']).any() and c['voiced'].any() and (c['db64'][c['voiced']] < -1.0).any()
    lspec, db = _check_both(c, name)
    np.testing.assert_array_equal(lspec, _envelope(c))          # same input, same bytes
    np.testing.assert_array_equal(db, _aperiodicity(c))


@pytest.mark.gpu
@pytest.mark.parametrize('what', ['T1', 'T3', 'short', 'f0_min', 'f0_max', 'nb2', 'nb33', 'L256', 'L8192'])
def test_edge_shapes(what):
    from percivaltts_amd import ops
    s = ws.case('A')
    fs, L, nb = s['fs'], s['L'], 5
    wav, f0, voiced = s['wav64'], s['f0'][8:26], s['voiced'][8:26]          # eighteen voiced frames (the waveform's own start is noise)
    if what in ('T1', 'T3'):
        f0, voiced = f0[:int(what[1])], voiced[:int(what[1])]
    elif what == 'short':
        wav, f0, voiced = wav[:60], f0[:3], voiced[:3]          # shorter than the 2 * 52 + 1 samples of the shortest window
        assert 60 < 2 * int(1.5 * fs / float(f0.max())) + 1
    elif what == 'f0_min':
        f0 = np.full(6, F0_MIN, dtype=np.float32)               # 2 * 120 + 1 = 241 samples
    elif what == 'f0_max':
        f0 = np.full(6, F0_MAX, dtype=np.float32)               # 2 * 30 + 1 = 61 samples, n0 = 20
    elif what == 'nb2':
        nb = 2
    elif what == 'nb33':
        nb = 33
    elif what == 'L256':
        L, f0 = 256, np.full(6, 250.0, dtype=np.float32)        # 2 * 48 + 1 = 97 samples
    elif what == 'L8192':                                       # the largest dftlen the check admits: 112 and 144 KiB of LDS
        L, f0 = 8192, np.array([3.0, 140.0, 120.0, 101.0, 250.0], dtype=np.float32)    # 3 Hz: 2 * 4000 + 1 <= 8192, d = 1.02 bins
        voiced = np.array([True, True, False, True, True])
    if len(voiced) != len(f0):
        voiced = np.ones(len(f0), dtype=bool)
    ops.world_analysis_check(L, fs, SHIFT, float(f0.min()), float(f0.max()))
    _check_both(references(wav, f0, voiced, fs, L, nb), what)


@pytest.mark.gpu
def test_no_frames_no_launch():
    from percivaltts_amd import _hip, ops
    with _hip.KernelTimer() as kt:
        spec = ops.world_envelope(_dev(np.zeros(10)), _dev(np.zeros(0)), SHIFT, 8000, 512)
        aper = ops.world_aperiodicity(_dev(np.zeros(10)), _dev(np.zeros(0)), _dev(np.zeros(0)), SHIFT, 8000, 512, 5)
    assert kt.records == []
    assert tuple(spec.shape) == (0, 257) and tuple(aper.shape) == (0, 5)
    l = _hip.lib()
    assert l.ptts_world_envelope(None, 0, None, None, 0, SHIFT, 8000.0, 512, 0, None) == 0
    assert l.ptts_world_envelope(None, 0, None, None, 1, SHIFT, 8000.0, 768, 0, None) != 0
    assert l.ptts_world_envelope(None, 0, None, None, 1, SHIFT, 8000.0, 16384, 0, None) != 0
    assert l.ptts_world_aperiodicity(None, 0, None, None, None, 0, 5, SHIFT, 8000.0, 512, None, 0, None) == 0
    assert l.ptts_world_aperiodicity(None, 0, None, None, None, 1, 5, SHIFT, 8000.0, 768, None, 0, None) != 0
    assert l.ptts_world_aperiodicity(None, 0, None, None, None, 1, 1, SHIFT, 8000.0, 512, None, 0, None) != 0
    with pytest.raises(_hip.HipLibraryError):
        ops.world_envelope(torch.zeros(10), _dev(np.full(3, 150.0)), SHIFT, 8000, 512)
    with pytest.raises(_hip.HipLibraryError):
        ops.world_aperiodicity(_dev(np.zeros(10)), _dev(np.full(3, 150.0)).double(), _dev(np.ones(3)), SHIFT, 8000, 512, 5)


@pytest.mark.gpu
def test_unvoiced_frames_inside_a_voiced_track():
    """The rows of unvoiced frames are 0 dB exactly; a frame's row depends on that frame alone: turning other frames unvoiced, or
    analysing a frame on its own grid position with the others unvoiced, leaves it byte for byte."""
    from percivaltts_amd import ops
    c = case('A')
    base = _aperiodicity(c)
    assert (base[~c['voiced']] == 0.0).all() and (base[c['voiced']] < 0.0).any()
    voiced = c['voiced'].copy()
    off = np.flatnonzero(voiced)[::3]
    voiced[off] = False
    got = ops.world_aperiodicity(_dev(c['wav']), _dev(c['f0']), _dev(voiced), SHIFT, c['fs'], c['L'], c['nb']).cpu().numpy()    # a bool tensor
    assert (got[~voiced] == 0.0).all()
    np.testing.assert_array_equal(got[voiced], base[voiced])
    # the envelope: a frame follows its own rate alone
    env = _envelope(c)
    rate = c['rate'].copy()
    rate[off] = UNVOICED_RATE
    got = ops.world_envelope(_dev(c['wav']), _dev(rate), SHIFT, c['fs'], c['L'], log=True).cpu().numpy()
    keep = np.ones(c['T'], dtype=bool)
    keep[off] = False
    np.testing.assert_array_equal(got[keep], env[keep])
    assert np.abs(got[off] - env[off]).max() > 0


def _round_trip_errors(CMP_in, bands, aper, voc, frames):
    """(rms in dB of the spectral bands, mean over the bands of |the median over the frames of the aperiodicity error|)."""
    s1 = 1 + voc.spec_size
    e = DB * (np.asarray(bands, dtype=np.float64)[frames] - CMP_in[frames, 1:s1].astype(np.float64))
    a = np.median(np.asarray(aper, dtype=np.float64)[frames] - CMP_in[frames, s1:s1 + voc.aper_size].astype(np.float64), axis=0)
    return float(np.sqrt(np.mean(e ** 2))), float(np.abs(a).mean())


@pytest.mark.gpu
def test_round_trip_synthesis_then_analysis():
    """synthesis_device with a fixed noise, then analysis_device with the true f0, against the parameters that went in: the
    device's errors stay within 10 % of those of the float64 restatement's analysis of the same waveform, since both run the same
    definition (the rule of test_analysis.py::test_round_trip_synthesis_then_analysis).  f0 moves slowly, as the estimator asks."""
    from percivaltts_amd import vocoders
    fs, L, T, ns, na = 16000, 2048, 81, 17, 5
    voc = vocoders.VocoderWORLDAnalysisDevice(fs, SHIFT, ns, na, dftlen=L)
    rng = np.random.RandomState(9)
    f0 = (170.0 + 30.0 * np.sin(np.arange(T) / 40.0)).astype(np.float32)
    spec = -5.0 + np.cumsum(rng.randn(1, ns) * 0.4, axis=1) + 0.1 * np.sin(np.arange(T) / 25.0)[:, None]
    aper = np.tile(np.array([-30.0, -24.0, -14.0, -8.0, -3.0]), (T, 1))
    CMP = np.concatenate([np.log(f0.astype(np.float64))[:, None], spec, aper, np.ones((T, 1))], axis=1).astype(np.float32)
    wavlen = ws.wavlen_of(T, fs)
    wav = voc.synthesis_device(CMP, noise=_dev(rng.randn(wavlen)))
    assert wav.shape == (wavlen,) and np.abs(wav).max() > 1e-4
    got = voc.analysis_device(wav, f0, F0_MIN, F0_MAX)
    assert got.shape == CMP.shape and got.dtype == np.float32 and (got[:, -1] == 1).all()
    np.testing.assert_allclose(got[:, 0], CMP[:, 0], rtol=1e-6)
    frames = np.arange(6, T - 6)
    gpu = _round_trip_errors(CMP, got[:, 1:1 + ns], got[:, 1 + ns:1 + ns + na], voc, frames)
    lspec = envelope_restated(wav, f0, SHIFT, fs, L, np.float64)
    bands = ta.compress_restated(lspec, band_weights(ns, fs, L), 'lsq', True, np.float64)
    _, db = aperiodicity_restated(wav, f0, np.ones(T, dtype=bool), SHIFT, fs, L, na, np.float64)
    cpu = _round_trip_errors(CMP, bands, db, voc, frames)
    print('round trip: spectral bands {:.4f} dB rms on the device, {:.4f} dB by the float64 restatement; '
          'aperiodicity band medians off by {:.4f} dB on the device, {:.4f} dB by the restatement'.format(gpu[0], cpu[0], gpu[1], cpu[1]))
    assert gpu[0] <= 1.1 * cpu[0] and gpu[1] <= 1.1 * cpu[1]


@pytest.mark.gpu
def test_analysis_device_and_files(tmp_path):
    from percivaltts_amd import ops, vocoders
    s = ws.case('A')
    fs, L, T = s['fs'], s['L'], s['T']
    voc = vocoders.VocoderWORLDAnalysisDevice(fs, SHIFT, 9, 4, dftlen=L)
    f0 = np.where(s['voiced'], s['f0'], 0.0).astype(np.float32)
    CMP = voc.analysis_device(s['wav64'], f0, F0_MIN, F0_MAX)
    assert CMP.shape == (T, voc.featuressizeraw()) and CMP.dtype == np.float32 and np.isfinite(CMP).all()
    np.testing.assert_array_equal(CMP[:, -1], s['voiced'].astype(np.float32))
    track = ops.f0_track(f0, F0_MIN, F0_MAX, fs, SHIFT, L)
    np.testing.assert_allclose(CMP[:, 0], np.log(track.astype(np.float64)), rtol=1e-6)
    # the chain of the public ops, byte for byte
    w = _dev(s['wav64'])
    rate = np.where(s['voiced'], track, np.float32(UNVOICED_RATE)).astype(np.float32)
    lspec = ops.world_envelope(w, _dev(rate), SHIFT, fs, L, log=True)
    np.testing.assert_array_equal(CMP[:, 1:10], ops.fwbnd_compress(lspec, fs, 9, log=True).cpu().numpy())
    aper = ops.world_aperiodicity(w, _dev(track), _dev(s['voiced'].astype(np.float32)), SHIFT, fs, L, 4).cpu().numpy()
    np.testing.assert_array_equal(CMP[:, 10:14], aper)
    assert (aper[~s['voiced']] == 0).all() and aper.min() >= -60 and aper.max() <= 0
    # from file to files
    path = str(tmp_path / 'wav' / 'a.wav')
    os.makedirs(os.path.dirname(path))
    vocoders.wavwrite(path, s['wav64'], fs)
    f0.tofile(str(tmp_path / 'a.f0'))
    outs = {'f0': str(tmp_path / 'lf0' / '*.lf0'), 'spec': str(tmp_path / 'spec' / '*.spec'), 'noise': str(tmp_path / 'ap' / '*.ap'),
            'vuv': str(tmp_path / 'vuv' / '*.vuv')}
    assert voc.analysisfid_device('a', str(tmp_path / 'wav' / '*.wav'), str(tmp_path / '*.f0'), F0_MIN, F0_MAX, outs) == T
    got = {k: np.fromfile(p.replace('*', 'a'), dtype=np.float32) for k, p in outs.items()}
    assert got['f0'].shape == (T,) and got['spec'].shape == (T * 9,) and got['noise'].shape == (T * 4,) and got['vuv'].shape == (T,)
    assert set(got['vuv']) == {0.0, 1.0} and np.isfinite(got['f0']).all()
    np.testing.assert_array_equal(got['f0'], CMP[:, 0])
    back = voc.analysis_device(vocoders.wavread(path)[0], f0, F0_MIN, F0_MAX)       # the waveform went through 16 bits
    np.testing.assert_array_equal(
        np.concatenate([got['f0'][:, None], got['spec'].reshape(T, 9), got['noise'].reshape(T, 4), got['vuv'][:, None]], axis=1), back)
    # the build's own F0 estimate
    est = voc.analysisf_device(path, None, str(tmp_path / 'est.lf0'), F0_MIN, F0_MAX, str(tmp_path / 'est.spec'),
                               str(tmp_path / 'est.ap'), str(tmp_path / 'est.vuv'))
    vuv = np.fromfile(str(tmp_path / 'est.vuv'), dtype=np.float32)
    assert est == len(vuv) and set(vuv) <= {0.0, 1.0} and np.isfinite(np.fromfile(str(tmp_path / 'est.lf0'), dtype=np.float32)).all()
    # refusals
    args = (f0, str(tmp_path / 'no.lf0'), F0_MIN, F0_MAX, str(tmp_path / 'no.spec'), str(tmp_path / 'no.ap'), str(tmp_path / 'no.vuv'))
    with pytest.raises(ValueError):
        voc.analysisf_device(path, *args, preproc_hp=60)
    with pytest.raises(ValueError):
        voc.analysisf_device(path, *args, preproc_fs=8000)
    other = str(tmp_path / 'other.wav')
    vocoders.wavwrite(other, s['wav64'], 16000)
    with pytest.raises(ValueError):
        voc.analysisf_device(other, *args)
    assert not os.path.exists(str(tmp_path / 'no.lf0'))
    with pytest.raises(NotImplementedError):
        voc.analysisf(path, outs['f0'], F0_MIN, F0_MAX, outs['spec'], outs['noise'], outs['vuv'])


@pytest.mark.gpu
@pytest.mark.parametrize('how', ['own_f0', 'highpass'])
def test_features_extraction_on_a_synthetic_world_corpus(how, tmp_path, monkeypatch):
    """Three utterances from .wav to the composed outputs and the weights that training reads, with a WORLD vocoder: once with the
    build's own F0 estimate, once through preprocwav with a high-pass filter."""
    import importlib
    from percivaltts_amd import vocoders
    monkeypatch.setenv('PERCIVAL_CORPUS', str(tmp_path / 'corpus'))
    monkeypatch.chdir(tmp_path)
    import percivaltts_amd.run as run
    run = importlib.reload(run)
    try:
        run.cfg.id_valid_start = 2
        fs = run.cfg.vocoder_fs
        voc = run.vocoder = vocoders.VocoderWORLDAnalysisDevice(fs, SHIFT, 33, 9, dftlen=2048)
        nout = voc.featuressize()
        run.cfg.outpath = str(tmp_path / 'corpus' / 'wav_WORLD_cmp') + '/*.cmp:(-1,' + str(nout) + ')'
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
        if how == 'own_f0':
            run.features_extraction(None, f0_min=100, f0_max=400)
        else:
            run.features_extraction(str(tmp_path / 'corpus' / 'f0' / '*.f0'), f0_min=100, f0_max=400, preproc_hp=60)
        for fid, T in zip(fids, lens):
            cmp = np.fromfile(run.cfg.outpath.split(':')[0].replace('*', fid), dtype=np.float32)
            w = np.fromfile(run.cfg.wpath.split(':')[0].replace('*', fid), dtype=np.float32)
            assert cmp.size % nout == 0 and np.isfinite(cmp).all() and w.shape == (cmp.size // nout,)
            vuv = np.fromfile(str(tmp_path / 'corpus' / ('wav_WORLD_vuv1/' + fid + '.vuv')), dtype=np.float32)
            ap = np.fromfile(str(tmp_path / 'corpus' / ('wav_WORLD_fwdbap9/' + fid + '.fwdbap')), dtype=np.float32)
            assert set(vuv) <= {0.0, 1.0} and len(vuv) == cmp.size // nout and ap.shape == (9 * len(vuv),)
            if how == 'highpass':
                assert len(vuv) == T and (vuv[:2] == 0).all() and (vuv[2:] == 1).all()
            else:
                assert abs(len(vuv) - T) <= 1 and vuv.mean() > 0.5
        for stat in ('mean4norm.dat', 'std4norm.dat'):
            assert os.path.getsize(os.path.join(os.path.dirname(run.cfg.outpath), stat)) == 4 * nout
    finally:
        importlib.reload(run)
