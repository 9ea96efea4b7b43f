"""Pulse-and-noise waveform synthesis (csrc/pulsesynth.hip; ops.pulse_table / noise_mask / pulse_synthesis,
VocoderPML.synthesis_device, vocoders.wavwrite, ModelTTS.generate_params(wavdir=...)).

The reference delegates synthesis to a submodule that is absent from its checkout and draws noise from numpy's global generator,
so there is nothing to compare samples with: the definition is the build's own and is restated here with
torch.fft on the CPU, in a chosen dtype.

Tolerance of the device results, a rule and not a tuned number (the rule of tests/test_spectrum.py, for a waveform): the yardstick
is the restatement in float64.  The same restatement with every array and intermediate in float32 has a largest absolute error
e32 against float64 ON THE SAME INPUT.  Every element of a device result has to lie within 4 * e32 + 2^-23 * max|want64| of the
float64 value.  The factor 4 covers another summation order and the device's exp / log / cos; it is a margin, not a measurement.
`check` prints e32 and the kernel's worst error before it asserts."""
import inspect
import math
import os
import wave

import numpy as np
import pytest
import torch


# ---------------------------------------------------------------------------------------------------------------------------
# the definition, restated
# ---------------------------------------------------------------------------------------------------------------------------
def rnd(x):
    return int(math.floor(x + 0.5))


def table_restated(f0, shift, fs, wavlen, dftlen):
    """The pulse table as a plain-Python loop: (t [P], rows), rows = dicts of start, winlen, lb, rb, fr, delay, f0."""
    f0 = np.asarray(f0, dtype=np.float64)
    T = len(f0)
    times = shift * np.arange(T)
    f0_at = lambda t: max(float(np.interp(t, times, f0)), 50.0)
    t = [0.0]
    while t[-1] < wavlen / float(fs):
        t.append(t[-1] + 1.0 / f0_at(t[-1]))
    rows = []
    P = len(t)
    for n in range(P):
        f0n = f0_at(t[n])
        winlen = 2 * int(max(0.050 * fs, 4.0 * fs / f0n) / 2) + 1
        if winlen > dftlen:
            raise ValueError('winlen')
        pos = int(winlen / 4)
        c = rnd(fs * t[n])
        lb = rnd(fs * (t[n - 1] + t[n]) / 2) if n > 0 else rnd(fs * (t[n] - 0.5 / f0n))
        rb = rnd(fs * (t[n] + t[n + 1]) / 2) if n < P - 1 else rnd(fs * (t[n] + 0.5 / f0n))
        rows.append(dict(start=c - pos, winlen=winlen, lb=min(max(lb, 0), wavlen), rb=min(max(rb, 0), wavlen),
                         fr=min(max(rnd(t[n] / shift), 0), T - 1), delay=pos + (fs * t[n] - c), f0=f0n))
    return np.array(t), rows


def band_centres(nb, fs):
    melmax = 1127.0 * np.log(1.0 + 0.5 * fs / 700.0)
    return 700.0 * (np.exp(np.arange(nb) * melmax / ((nb - 1) * 1127.0)) - 1.0)


def smooth_taps():
    w = np.hanning(9)
    w = w / w.sum()
    return w, np.convolve(w, w)


def mask_restated(nmb, f0, fs, L, dtype):
    """[T,nb] -> [T,K] in `dtype` (the band axis itself is float64 in both: it is a table, not data)."""
    nmb = np.asarray(nmb, dtype=dtype)
    T, nb = nmb.shape
    K = L // 2 + 1
    fb = band_centres(nb, fs)
    f = np.arange(K) * float(fs) / L
    b = np.clip(np.searchsorted(fb, f, side='right') - 1, 0, nb - 2)
    frac = np.clip((f - fb[b]) / (fb[b + 1] - fb[b]), 0.0, 1.0).astype(dtype)
    v = nmb[:, b] + frac[None, :] * (nmb[:, b + 1] - nmb[:, b])
    kcut = np.array([int(2.0 * float(x) * L / fs) for x in np.asarray(f0, dtype=np.float64)])
    x = ((v > 0.5) & (np.arange(K)[None, :] >= kcut[:, None])).astype(dtype)
    h = smooth_taps()[1].astype(dtype)
    left = 2 * x[:, :1] - x[:, 8:0:-1]
    right = 2 * x[:, -1:] - x[:, -2:-10:-1]
    xe = np.concatenate([left, x, right], axis=1)
    out = np.zeros_like(x)
    for i in range(17):
        out += h[i] * xe[:, i:i + K]
    return np.clip(out, 0, 1)


def minphase_restated(la, L):
    """Log-amplitudes la [K] (torch, real) -> the minimum-phase spectrum E [K] with |E| = exp(la)."""
    ctype = torch.complex128 if la.dtype == torch.float64 else torch.complex64
    c = torch.fft.irfft(la.to(ctype), n=L)
    c[1:L // 2] *= 2
    c[L // 2 + 1:] = 0
    return torch.exp(torch.fft.rfft(c))


def segments_restated(spec, mask, g, rows, fs, L, dtype):
    """The list of segments, each irfft(S)[:winlen], computed in `dtype` (torch.float64 or torch.float32)."""
    ctype = torch.complex128 if dtype == torch.float64 else torch.complex64
    spec = torch.tensor(np.asarray(spec), dtype=dtype)
    mask = torch.tensor(np.asarray(mask), dtype=dtype)
    g = torch.tensor(np.asarray(g), dtype=dtype)
    K = L // 2 + 1
    k = torch.arange(K, dtype=dtype)
    d = rnd(0.001 * fs)
    hann = torch.as_tensor(np.hanning(2 * d + 1)[:d + 1], dtype=dtype)
    segs = []
    for r in rows:
        hp = torch.zeros(K, dtype=dtype)
        tc = torch.tan(torch.tensor(math.pi * 0.5 * r['f0'] / fs, dtype=dtype))
        hp[1:] = (1.0 + (tc / torch.tan(math.pi * k[1:] / L)) ** 8) ** -0.5
        la = torch.log(torch.clamp(spec[r['fr']] * hp, min=1e-10))
        E = minphase_restated(la, L)
        D = torch.exp((-2j * math.pi * r['delay'] / L) * k.to(ctype))
        x = torch.zeros(L, dtype=dtype)
        n = r['rb'] - r['lb']
        if n > 0:
            s = g[r['lb']:r['rb']].clone()
            if n >= 2 * (d + 1):
                s[:d + 1] *= hann
                s[n - d - 1:] *= torch.flip(hann, [0])
            x[r['lb'] - r['start']:r['rb'] - r['start']] = s
        N = torch.fft.rfft(x)
        p = N.real ** 2 + N.imag ** 2
        e = (p[0] + p[-1] + 2 * p[1:-1].sum()) / L
        if float(e) > 0:
            N = N / torch.sqrt(e)
        m = mask[r['fr']]
        S = E * ((1 - m) * D + m * N)
        S[0] = S[0].real + 0j           # irfft reads the real part of bins 0 and L/2 only; said here, not left to the library
        S[-1] = S[-1].real + 0j
        segs.append(torch.fft.irfft(S, n=L)[:r['winlen']])
    return segs


def overlap_add_restated(segs, rows, wavlen, dtype):
    wav = torch.zeros(wavlen, dtype=dtype)
    for s, r in zip(segs, rows):
        a, b = max(r['start'], 0), min(r['start'] + r['winlen'], wavlen)
        if b > a:
            wav[a:b] += s[a - r['start']:b - r['start']]
    return wav.numpy()


def synth_restated(spec, mask, g, rows, fs, L, wavlen, dtype):
    return overlap_add_restated(segments_restated(spec, mask, g, rows, fs, L, dtype), rows, wavlen, dtype)


def check(got, want64, want32, what):
    """|got - want64| <= 4 e32 + 2^-23 max|want64|, every element."""
    got = np.asarray(got, dtype=np.float64)
    want64 = np.asarray(want64, dtype=np.float64)
    assert got.shape == want64.shape, (what, got.shape, want64.shape)
    e32 = float(np.abs(np.asarray(want32, dtype=np.float64) - want64).max()) if want64.size else 0.0
    bound = 4.0 * e32 + 2.0 ** -23 * (float(np.abs(want64).max()) if want64.size else 0.0)
    err = np.abs(got - want64)
    worst = float(err.max()) if err.size else 0.0
    print('{}: e32 = {:.3e}, kernel worst {:.3e}, bound {:.3e}, max|want| = {:.3e}'.format(
        what, e32, worst, bound, float(np.abs(want64).max()) if want64.size else 0.0))
    assert np.isfinite(got).all() and (err <= bound).all(), (what, e32, worst, bound)


# ---------------------------------------------------------------------------------------------------------------------------
# the two shapes; their references are computed once
# ---------------------------------------------------------------------------------------------------------------------------
SHIFT = 0.005
SHAPES = {'A': dict(fs=8000, L=512, T=40), 'B': dict(fs=32000, L=4096, T=24)}
NB = 9
_cases = {}


def wavlen_of(T, fs):
    return int(round(SHIFT * (T - 1) * fs))


def make_inputs(name, T=None, seed=None):
    """f0 [T], SPEC [T,K] (smooth, about 8 nepers of range), binary masks with a random cut-off, band values away from 0.5, g."""
    sh = SHAPES[name]
    fs, L = sh['fs'], sh['L']
    T = sh['T'] if T is None else T
    K = L // 2 + 1
    rng = np.random.RandomState((17 if name == 'A' else 29) if seed is None else seed)
    f0 = (170.0 + 60.0 * np.sin(np.arange(T) / 7.0)).astype(np.float32)
    x = np.linspace(0, 1, K)
    la = np.zeros((T, K))
    for j in range(1, 6):
        la += rng.randn(T, 1) * np.cos(np.pi * j * x + rng.rand(T, 1) * 6.28) / j
    la = la - la.min()
    la = -9.0 + 8.0 * la / la.max()
    spec = np.exp(la).astype(np.float32)
    cut = rng.randint(K // 8, K, size=T)
    mask = (np.arange(K)[None, :] >= cut[:, None]).astype(np.float32)
    nmb = rng.uniform(0, 0.45, size=(T, NB))
    hi = rng.rand(T, NB) < 0.5
    nmb[hi] = 1.0 - nmb[hi]                                     # [0, 0.45] U [0.55, 1]
    wavlen = wavlen_of(T, fs)
    g = rng.randn(max(wavlen, 1))[:wavlen].astype(np.float32)
    return dict(fs=fs, L=L, T=T, K=K, f0=f0, spec=spec, mask=mask, nmb=nmb.astype(np.float32), g=g, wavlen=wavlen)


def case(name):
    if name not in _cases:
        c = make_inputs(name)
        c['t'], c['rows'] = table_restated(c['f0'], SHIFT, c['fs'], c['wavlen'], c['L'])
        c['wav64'] = synth_restated(c['spec'], c['mask'], c['g'], c['rows'], c['fs'], c['L'], c['wavlen'], torch.float64)
        c['wav32'] = synth_restated(c['spec'], c['mask'], c['g'], c['rows'], c['fs'], c['L'], c['wavlen'], torch.float32)
        for v in c.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _cases[name] = c
    return _cases[name]


# ---------------------------------------------------------------------------------------------------------------------------
# CPU: the pulse table
# ---------------------------------------------------------------------------------------------------------------------------
INT_ROWS = ('start', 'winlen', 'lb', 'rb', 'fr')


@pytest.mark.parametrize('name', ['A', 'B'])
def test_pulse_table_matches_the_plain_loop(name):
    from percivaltts_amd import ops
    c = case(name)
    tab = ops.pulse_table(c['f0'], SHIFT, c['fs'], c['wavlen'], c['L'])
    t, rows = c['t'], c['rows']
    P = len(rows)
    assert tab['t'].shape == (P,) and (np.diff(tab['t']) > 0).all() and tab['t'][-1] >= c['wavlen'] / float(c['fs'])
    np.testing.assert_array_equal(tab['t'], t)
    for key in INT_ROWS:
        assert tab[key].dtype == np.int32 and tab[key].shape == (P,)
        np.testing.assert_array_equal(tab[key], [r[key] for r in rows], err_msg=key)
    for key in ('delay', 'f0'):
        assert tab[key].dtype == np.float64
        np.testing.assert_array_equal(tab[key], [r[key] for r in rows], err_msg=key)
    assert (np.diff(tab['start']) >= 0).all()
    assert (tab['lb'] <= tab['rb']).all() and (tab['rb'][:-1] <= tab['lb'][1:]).all()          # disjoint and ascending
    assert (tab['rb'][:-1] == tab['lb'][1:]).all() and tab['lb'][0] == 0 and tab['rb'][-1] == c['wavlen']      # and they tile
    assert (tab['winlen'] <= c['L']).all() and (tab['winlen'] % 2 == 1).all()
    d = rnd(0.001 * c['fs'])
    inner = (tab['rb'] - tab['lb'])[1:-1]
    assert inner.min() >= 2 * (d + 1), inner.min()


def test_pulse_table_shape_a_is_cropped_at_both_ends():
    c = case('A')
    starts = np.array([r['start'] for r in c['rows']])
    ends = starts + np.array([r['winlen'] for r in c['rows']])
    assert (starts < 0).any() and (ends > c['wavlen']).any()


def test_pulse_table_constant_f0():
    from percivaltts_amd import ops
    fs, T = 16000, 61
    wavlen = wavlen_of(T, fs)
    tab = ops.pulse_table(np.full(T, 100.0), SHIFT, fs, wavlen, 1024)
    n = np.arange(len(tab['t']))
    assert len(n) == int(np.ceil(wavlen / fs * 100.0 - 1e-9)) + 1
    np.testing.assert_allclose(tab['t'], n / 100.0, rtol=0, atol=1e-12)
    np.testing.assert_array_equal(tab['f0'], 100.0)
    np.testing.assert_array_equal(tab['winlen'], 2 * int(0.05 * fs / 2) + 1)
    # below the floor: 30 Hz is synthesised at 50 Hz
    low = ops.pulse_table(np.full(T, 30.0), SHIFT, fs, wavlen, 2048)
    np.testing.assert_array_equal(low['f0'], 50.0)
    np.testing.assert_allclose(np.diff(low['t']), 1 / 50.0, rtol=0, atol=1e-12)


def test_pulse_table_refuses_what_it_cannot_build():
    from percivaltts_amd import ops
    fs, T = 16000, 21
    wavlen = wavlen_of(T, fs)
    with pytest.raises(ValueError):                             # 0.05 * fs = 800 samples do not fit 512
        ops.pulse_table(np.full(T, 100.0), SHIFT, fs, wavlen, 512)
    with pytest.raises(ValueError):
        ops.pulse_table(np.full(T, 100.0), SHIFT, fs, wavlen, 1000)       # not a power of two
    with pytest.raises(ValueError):
        ops.pulse_table(np.full(T, 100.0), SHIFT, fs, wavlen + 1, 1024)   # not this utterance's length
    with pytest.raises(ValueError):
        ops.pulse_table(np.array([100.0, -1.0, 100.0]), SHIFT, fs, wavlen_of(3, fs), 1024)
    empty = ops.pulse_table(np.array([100.0]), SHIFT, fs, 0, 1024)
    assert empty['start'].shape == (1,) and empty['rb'][0] == 0             # the pulse at t = 0, with nothing to fill


# ---------------------------------------------------------------------------------------------------------------------------
# CPU: the restatement itself
# ---------------------------------------------------------------------------------------------------------------------------
def test_restated_minimum_phase_is_causal_and_keeps_the_amplitude():
    c = case('A')
    L, K, fs = c['L'], c['K'], c['fs']
    r = dict(c['rows'][5])
    # a smooth envelope: the response is causal
    la = torch.log(torch.as_tensor(c['spec'][r['fr']].astype(np.float64)))
    E = minphase_restated(la, L)
    e = torch.fft.irfft(E, n=L).numpy()
    assert (e[L // 2:] ** 2).sum() < 1e-6 * (e ** 2).sum()
    np.testing.assert_allclose(np.abs(E.numpy()), c['spec'][r['fr']].astype(np.float64), rtol=1e-12)
    # the whole segment without noise and without delay: the envelope times the high-pass
    zeros = np.zeros((c['T'], K))
    impulse_row = dict(r, delay=0.0, lb=0, rb=0, winlen=L)
    seg = segments_restated(c['spec'], zeros, np.zeros(c['wavlen']), [impulse_row], fs, L, torch.float64)[0].numpy()
    k = np.arange(K)
    hp = np.zeros(K)
    hp[1:] = (1 + (np.tan(np.pi * 0.5 * r['f0'] / fs) / np.tan(np.pi * k[1:] / L)) ** 8) ** -0.5
    want = np.maximum(c['spec'][r['fr']].astype(np.float64) * hp, 1e-10)
    np.testing.assert_allclose(np.abs(np.fft.rfft(seg)), want, rtol=1e-12, atol=1e-14 * want.max())       # fp64 rounding of the FFTs


def test_restated_pulse_train_is_periodic():
    fs, L, T = 8000, 512, 60
    wavlen = wavlen_of(T, fs)
    f0 = np.full(T, 200.0)                                      # 40 samples a period, exactly
    _, rows = table_restated(f0, SHIFT, fs, wavlen, L)
    spec = np.tile(make_inputs('A')['spec'][:1], (T, 1))
    wav = synth_restated(spec, np.zeros_like(spec), np.zeros(wavlen), rows, fs, L, wavlen, torch.float64)
    mid = wav[L:wavlen - L]
    assert np.abs(mid).max() > 1e-4
    np.testing.assert_allclose(mid[40:], mid[:-40], rtol=0, atol=1e-12 * np.abs(mid).max())


def test_restated_mask_equals_filtfilt():
    import scipy.signal
    c = case('A')
    got = mask_restated(c['nmb'], c['f0'], c['fs'], c['L'], np.float64)
    K, L, fs = c['K'], c['L'], c['fs']
    fb = band_centres(NB, fs)
    w = smooth_taps()[0]
    for t in range(c['T']):
        v = np.interp(np.arange(K) * float(fs) / L, fb, c['nmb'][t].astype(np.float64))
        v[:int(2.0 * float(c['f0'][t]) * L / fs)] = 0.0
        x = (v > 0.5).astype(np.float64)
        want = np.clip(scipy.signal.filtfilt(w, [1.0], x), 0, 1)
        np.testing.assert_allclose(got[t], want, rtol=0, atol=1e-12)
    assert 0.0 < got.mean() < 1.0 and ((got > 0) & (got < 1)).any()


# ---------------------------------------------------------------------------------------------------------------------------
# CPU: the public interface
# ---------------------------------------------------------------------------------------------------------------------------
def test_interface():
    from percivaltts_amd import modeltts, vocoders
    names = list(inspect.signature(modeltts.ModelTTS.generate_params).parameters)
    assert names[-1] == 'wavdir'
    assert inspect.signature(modeltts.ModelTTS.generate_params).parameters['wavdir'].default is None
    voc = vocoders.VocoderPML(8000, SHIFT, 12, NB, dftlen=512)
    with pytest.raises(NotImplementedError):
        voc.synthesis(None)
    with pytest.raises(ValueError):
        voc.synthesis_device(np.zeros((4, voc.featuressizeraw()), dtype=np.float32), pp_f0_smooth=0.1)
    with pytest.raises(ValueError):
        voc.synthesis_device(np.zeros((4, voc.featuressizeraw() + 1), dtype=np.float32))
    assert not hasattr(vocoders.VocoderWORLD(8000, SHIFT, 12, 4), 'synthesis_device')


def test_wavwrite_round_trip(tmp_path, capsys):
    from percivaltts_amd import vocoders
    x = (0.5 * np.sin(np.arange(400) / 9.0)).astype(np.float32)
    path = str(tmp_path / 'a.wav')
    vocoders.wavwrite(path, x, 8000)
    assert capsys.readouterr().out == ''
    with wave.open(path, 'rb') as f:
        assert (f.getnchannels(), f.getsampwidth(), f.getframerate(), f.getnframes()) == (1, 2, 8000, 400)
        pcm = np.frombuffer(f.readframes(400), dtype='<i2')
    assert np.abs(pcm / 32767.0 - x).max() <= 0.5 / 32767.0 + 1e-7
    vocoders.wavwrite(path, 4.0 * x, 8000)                      # above full scale: divided by its peak, and said so
    assert 'peak' in capsys.readouterr().out
    with wave.open(path, 'rb') as f:
        loud = np.frombuffer(f.readframes(400), dtype='<i2')
    assert np.abs(loud).max() == 32767
    vocoders.wavwrite(path, np.zeros(0, dtype=np.float32), 8000)
    with wave.open(path, 'rb') as f:
        assert f.getnframes() == 0


# ---------------------------------------------------------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------------------------------------------------------
def _dev(a, dtype=torch.float32):
    return torch.tensor(np.asarray(a), dtype=dtype).cuda().contiguous()


def _synth(c, mask=None, g=None, tab=None):
    from percivaltts_amd import ops
    tab = ops.pulse_table(c['f0'], SHIFT, c['fs'], c['wavlen'], c['L']) if tab is None else tab
    wav = ops.pulse_synthesis(_dev(c['spec']), _dev(c['mask'] if mask is None else mask), tab, _dev(c['g'] if g is None else g),
                              c['fs'], c['L'], c['wavlen'])
    assert wav.dtype == torch.float32 and wav.is_cuda and tuple(wav.shape) == (c['wavlen'],)
    return wav.cpu().numpy()


@pytest.mark.gpu
@pytest.mark.parametrize('name', ['A', 'B'])
def test_noise_mask_against_restatement(name):
    from percivaltts_amd import ops
    c = case(name)
    got = ops.noise_mask(_dev(c['nmb']), _dev(c['f0']), c['fs'], c['L'])
    assert tuple(got.shape) == (c['T'], c['K'])
    want64 = mask_restated(c['nmb'], c['f0'], c['fs'], c['L'], np.float64)
    want32 = mask_restated(c['nmb'], c['f0'], c['fs'], c['L'], np.float32)
    check(got.cpu().numpy(), want64, want32, 'noise_mask ' + name)
    assert 0.0 < want64.mean() < 1.0


@pytest.mark.gpu
@pytest.mark.parametrize('name', ['A', 'B'])
def test_pulse_synthesis_against_restatement(name):
    c = case(name)
    got = _synth(c)
    assert np.abs(c['wav64']).max() > 1e-3
    check(got, c['wav64'], c['wav32'], 'pulse_synthesis ' + name)
    np.testing.assert_array_equal(got, _synth(c))               # same input, same bytes


@pytest.mark.gpu
def test_pulse_synthesis_smoothed_mask_of_the_kernel():
    """The two kernels chained: a mask with values strictly between 0 and 1, as ops.noise_mask makes them."""
    from percivaltts_amd import ops
    c = case('A')
    mask = ops.noise_mask(_dev(c['nmb']), _dev(c['f0']), c['fs'], c['L']).cpu().numpy()
    want64 = synth_restated(c['spec'], mask, c['g'], c['rows'], c['fs'], c['L'], c['wavlen'], torch.float64)
    want32 = synth_restated(c['spec'], mask, c['g'], c['rows'], c['fs'], c['L'], c['wavlen'], torch.float32)
    check(_synth(c, mask=mask), want64, want32, 'pulse_synthesis A, smoothed mask')


@pytest.mark.gpu
@pytest.mark.parametrize('fill', [0.0, 1.0])
def test_pulse_synthesis_constant_masks(fill):
    c = case('A')
    mask = np.full_like(c['mask'], fill)
    want64 = synth_restated(c['spec'], mask, c['g'], c['rows'], c['fs'], c['L'], c['wavlen'], torch.float64)
    want32 = synth_restated(c['spec'], mask, c['g'], c['rows'], c['fs'], c['L'], c['wavlen'], torch.float32)
    got = _synth(c, mask=mask)
    check(got, want64, want32, 'pulse_synthesis A, mask = {}'.format(fill))
    other = _synth(c, mask=mask, g=np.random.RandomState(3).randn(c['wavlen']).astype(np.float32))
    if fill == 0.0:
        np.testing.assert_array_equal(got, other)               # no noise gets through
    else:
        assert np.abs(got - other).max() > 1e-4


@pytest.mark.gpu
def test_pulse_synthesis_short_utterances():
    from percivaltts_amd import _hip, ops
    one = make_inputs('A', T=1)
    assert one['wavlen'] == 0
    with _hip.KernelTimer() as kt:
        tab = ops.pulse_table(one['f0'], SHIFT, one['fs'], 0, one['L'])
        wav = ops.pulse_synthesis(_dev(one['spec']), _dev(one['mask']), tab, _dev(one['g']), one['fs'], one['L'], 0)
    assert tuple(wav.shape) == (0,) and kt.records == []
    c = make_inputs('A', T=3)
    t, rows = table_restated(c['f0'], SHIFT, c['fs'], c['wavlen'], c['L'])
    assert len(rows) == 3 and t[1] < c['wavlen'] / float(c['fs']) <= t[2]      # the first, one interior and the end pulse
    want64 = synth_restated(c['spec'], c['mask'], c['g'], rows, c['fs'], c['L'], c['wavlen'], torch.float64)
    want32 = synth_restated(c['spec'], c['mask'], c['g'], rows, c['fs'], c['L'], c['wavlen'], torch.float32)
    check(_synth(c), want64, want32, 'pulse_synthesis A, T = 3')


@pytest.mark.gpu
def test_ops_argument_checks_on_device():
    from percivaltts_amd import _hip, ops
    c = case('A')
    tab = ops.pulse_table(c['f0'], SHIFT, c['fs'], c['wavlen'], c['L'])
    spec, mask, g = _dev(c['spec']), _dev(c['mask']), _dev(c['g'])
    with pytest.raises(_hip.HipLibraryError):
        ops.pulse_synthesis(spec.cpu(), mask, tab, g, c['fs'], c['L'], c['wavlen'])
    with pytest.raises(_hip.HipLibraryError):
        ops.pulse_synthesis(spec.double(), mask, tab, g, c['fs'], c['L'], c['wavlen'])
    with pytest.raises(ValueError):
        ops.pulse_synthesis(spec, mask[:, :-1].contiguous(), tab, g, c['fs'], c['L'], c['wavlen'])
    with pytest.raises(ValueError):
        ops.pulse_synthesis(spec, mask, tab, g[:-1].contiguous(), c['fs'], c['L'], c['wavlen'])
    with pytest.raises(ValueError):
        ops.pulse_synthesis(spec.clone().requires_grad_(True), mask, tab, g, c['fs'], c['L'], c['wavlen'])
    with pytest.raises(ValueError):                             # a table built for another transform length
        ops.pulse_synthesis(spec, mask, dict(tab, winlen=tab['winlen'] + 2 * c['L']), g, c['fs'], c['L'], c['wavlen'])
    with pytest.raises(ValueError):
        ops.noise_mask(_dev(c['nmb']), _dev(c['f0'][:-1]), c['fs'], c['L'])
    with pytest.raises(ValueError):
        ops.noise_mask(_dev(c['nmb']), _dev(c['f0']), c['fs'], 500)
    # the C ABI refuses a transform length it has no kernel for, without a launch
    l = _hip.lib()
    assert l.ptts_pulse_segments(None, None, None, None, None, 1, 1, 768, 8000.0, 10, None, 64, None) != 0
    assert l.ptts_pulse_segments(None, None, None, None, None, 0, 1, 512, 8000.0, 10, None, 64, None) == 0
    assert l.ptts_noise_mask(None, None, None, 0, NB, 8000.0, 512, None, 0, None) == 0


def _cmp_of(c, voc):
    """[T, 1 + spec_size + nb] PML parameters whose decompressed envelope is moderate."""
    rng = np.random.RandomState(5)
    spec = -4.0 + np.cumsum(rng.randn(c['T'], voc.spec_size) * 0.3, axis=1)
    return np.concatenate([np.log(c['f0'].astype(np.float64))[:, None], spec, c['nmb']], axis=1).astype(np.float32)


@pytest.mark.gpu
def test_synthesis_device_is_the_chain_and_follows_the_seed():
    from percivaltts_amd import ops, vocoders
    c = case('A')
    voc = vocoders.VocoderPML(c['fs'], SHIFT, 12, NB, dftlen=c['L'])
    CMP = _cmp_of(c, voc)
    # a caller's noise: the chain of the public ops, byte for byte
    got = voc.synthesis_device(CMP, noise=_dev(c['g']))
    assert got.dtype == np.float32 and got.shape == (c['wavlen'],)
    d = _dev(CMP)
    f0 = torch.exp(d[:, 0]).contiguous()
    spec = voc.decompress_spectrum(d[:, 1:13].contiguous())
    mask = ops.noise_mask(d[:, 13:].contiguous(), f0, c['fs'], c['L'])
    tab = ops.pulse_table(f0.cpu().numpy(), SHIFT, c['fs'], c['wavlen'], c['L'])
    want = ops.pulse_synthesis(spec, mask, tab, _dev(c['g']), c['fs'], c['L'], c['wavlen']).cpu().numpy()
    np.testing.assert_array_equal(got, want)
    np.testing.assert_array_equal(voc.synthesis_device(d, noise=_dev(c['g'])), got)          # device tensor in
    assert np.isfinite(got).all() and np.abs(got).max() > 0
    # the library's generator
    ops.rng_seed(1234)
    a = voc.synthesis_device(CMP)
    ops.rng_seed(1234)
    b = voc.synthesis_device(CMP)
    np.testing.assert_array_equal(a, b)
    ops.rng_seed(1235)
    assert np.abs(voc.synthesis_device(CMP) - a).max() > 0
    assert float(mask.max()) > 0


def _small_cfg():
    import percivaltts_amd
    cfg = percivaltts_amd.configuration()
    cfg.arch_hiddenwidth = 8; cfg.train_batch_size = 2
    cfg.arch_ctx_nbcnnlayers = 1; cfg.arch_ctx_winlen = 5
    cfg.arch_gen_nbcnnlayers = 2; cfg.arch_gen_nbfilters = 2; cfg.arch_gen_winlen = 3; cfg.arch_spec_freqlen = 3
    return cfg


@pytest.mark.gpu
@pytest.mark.parametrize('wins', [None, [[-0.5, 0.0, 0.5], [1.0, -2.0, 1.0]]])
def test_generate_params_writes_waveforms(wins, tmp_path):
    from percivaltts_amd import modeltts_common, vocoders
    ctx, fs, L = 19, 8000, 512
    voc = vocoders.VocoderPML(fs, SHIFT, 12, 4, dftlen=L, mlpg_wins=wins)
    mod = modeltts_common.Generic(ctx, voc, layertypes=['FC', 'BLSTM'], cfgarch=_small_cfg())
    rng = np.random.RandomState(0)
    nout = voc.featuressize()
    lens = [41, 23, 9]
    (tmp_path / 'lab').mkdir(); (tmp_path / 'cmp').mkdir()
    fids = ['utt_{:02d}'.format(i) for i in range(len(lens))]
    for fid, n in zip(fids, lens):
        (rng.rand(n, ctx) * 2 - 1).astype(np.float32).tofile(str(tmp_path / 'lab' / (fid + '.lab')))
    mean = (rng.randn(nout) * 0.3).astype(np.float32)
    mean[0] = np.log(170.0)                                     # log f0: keeps winlen within dftlen
    std = np.full(nout, 0.1, dtype=np.float32)
    mean.tofile(str(tmp_path / 'cmp' / 'mean4norm.dat')); std.tofile(str(tmp_path / 'cmp' / 'std4norm.dat'))
    inpath = str(tmp_path / 'lab') + '/*.lab:(-1,{})'.format(ctx)
    outpath = str(tmp_path / 'cmp') + '/*.cmp:(-1,{})'.format(nout)

    mod.generate_params(inpath, outpath, fids, str(tmp_path / 'gen'), do_objmeas=False, batch_size=2,
                        specdir=str(tmp_path / 'spec'), wavdir=str(tmp_path / 'wav'))
    mod.generate_params(inpath, outpath, fids, str(tmp_path / 'gen0'), do_objmeas=False, batch_size=2,
                        specdir=str(tmp_path / 'spec0'))
    assert not os.path.exists(str(tmp_path / 'wav0'))
    for fid, n in zip(fids, lens):
        with wave.open(str(tmp_path / 'wav' / (fid + '.wav')), 'rb') as f:
            assert (f.getnchannels(), f.getsampwidth(), f.getframerate()) == (1, 2, fs)
            assert f.getnframes() == wavlen_of(n, fs)
            pcm = np.frombuffer(f.readframes(f.getnframes()), dtype='<i2')
        assert np.abs(pcm).max() > 0
        for sub, ext in (('gen', '.cmp'), ('spec', '.spec')):
            a = np.fromfile(str(tmp_path / sub / (fid + ext)), dtype=np.float32)
            b = np.fromfile(str(tmp_path / (sub + '0') / (fid + ext)), dtype=np.float32)
            np.testing.assert_array_equal(a, b)

    world = vocoders.VocoderWORLD(fs, SHIFT, 12, 4, dftlen=L)
    mw = modeltts_common.Generic(ctx, world, layertypes=['FC'], cfgarch=_small_cfg())
    with pytest.raises(ValueError):
        mw.generate_params(inpath, outpath, fids, str(tmp_path / 'genw'), do_objmeas=False, wavdir=str(tmp_path / 'wavw'))
