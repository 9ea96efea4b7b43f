"""Periodic-plus-aperiodic waveform synthesis for the WORLD parameters (csrc/worldsynth.hip; ops.world_pulse_table / aper_rows /
world_synthesis, VocoderWORLDDevice.synthesis_device, ModelTTS.generate_params(wavdir=...) over it).

The reference calls pyworld, which is not part of this build, and draws its noise from a global generator, so there is nothing to
compare samples with: the definition is the build's own, modelled on the published WORLD synthesis, and is
restated here with torch.fft on the CPU, in a chosen dtype.

Tolerance of the device results: the rule of tests/test_pulsesynth.py, not a tuned number.  The yardstick is the restatement in
float64.  The same restatement with every array and intermediate in float32 has a largest absolute error e32 against float64 ON
THE SAME INPUT.  Every element of a device result has to lie within 4 * e32 + 2^-23 * max|want64| of the float64 value.  `check`
prints e32 and the kernel's worst error before it asserts."""
import inspect
import math
import wave

import numpy as np
import pytest
import torch


# ---------------------------------------------------------------------------------------------------------------------------
# the definition, restated
# ---------------------------------------------------------------------------------------------------------------------------
def rnd(x):
    return int(math.floor(x + 0.5))


def table_restated(f0, voiced, shift, fs, wavlen, dftlen):
    """The pulse table as a plain-Python loop: (t [P], rows), rows = dicts of start, winlen, lb, rb, fr, i0, i1, v, delay, f0, w."""
    f0 = np.asarray(f0, dtype=np.float64)
    T = len(f0)
    times = shift * np.arange(T)

    def rate(t):
        if not voiced[min(max(rnd(t / shift), 0), T - 1)]:
            return 500.0
        return max(float(np.interp(t, times, f0)), 50.0)

    t = [0.0]
    while t[-1] < wavlen / float(fs):
        t.append(t[-1] + 1.0 / rate(t[-1]))
    rows = []
    P = len(t)
    pos = int((2 * int(0.050 * fs / 2) + 1) / 4)
    for n in range(P):
        f0n = rate(t[n])
        winlen = 2 * int(max(0.050 * fs, 4.0 * fs / f0n) / 2) + 1
        if winlen > dftlen:
            raise ValueError('winlen')
        c = rnd(fs * t[n])
        lb = rnd(fs * (t[n - 1] + t[n]) / 2) if n > 0 else rnd(fs * (t[n] - 0.5 / f0n))
        rb = rnd(fs * (t[n] + t[n + 1]) / 2) if n < P - 1 else rnd(fs * (t[n] + 0.5 / f0n))
        fr = min(max(rnd(t[n] / shift), 0), T - 1)
        i0 = min(int(t[n] / shift), T - 1)
        rows.append(dict(start=c - pos, winlen=winlen, lb=min(max(lb, 0), wavlen), rb=min(max(rb, 0), wavlen), fr=fr,
                         i0=i0, i1=min(i0 + 1, T - 1), v=int(bool(voiced[fr])), delay=pos + (fs * t[n] - c), f0=f0n,
                         w=(t[n] / shift - i0) if i0 < T - 1 else 0.0))
    return np.array(t), rows


def band_centres(nb, fs):
    melmax = 1127.0 * np.log(1.0 + 0.5 * fs / 700.0)
    return 700.0 * (np.exp(np.arange(nb) * melmax / ((nb - 1) * 1127.0)) - 1.0)


def aper_restated(aper_db, vuv, fs, L, dtype):
    """[T,A] dB -> [T,K] in `dtype` (the band axis itself is float64 in both: it is a table, not data)."""
    x = np.asarray(aper_db, dtype=dtype)
    T, nb = x.shape
    K = L // 2 + 1
    amp = np.power(dtype(10.0), x / dtype(20.0))
    fb = band_centres(nb, fs)
    f = np.arange(K) * float(fs) / L
    b = np.clip(np.searchsorted(fb, f, side='right') - 1, 0, nb - 2)
    frac = np.clip((f - fb[b]) / (fb[b + 1] - fb[b]), 0.0, 1.0).astype(dtype)
    v = np.clip(amp[:, b] + frac[None, :] * (amp[:, b + 1] - amp[:, b]), 0, 1)
    v[np.asarray(vuv, dtype=np.float64) < 0.5] = 1
    return v.astype(dtype)


def minphase_restated(la, L):
    """Log-amplitudes la [K] (torch, real) -> the minimum-phase spectrum E [K] with |E| = exp(la)."""
    ctype = torch.complex128 if la.dtype == torch.float64 else torch.complex64
    c = torch.fft.irfft(la.to(ctype), n=L)
    c[1:L // 2] *= 2
    c[L // 2 + 1:] = 0
    return torch.exp(torch.fft.rfft(c))


def segments_restated(spec, aper, g, rows, fs, L, dtype):
    """The list of segments, each irfft(E_p D + E_a N)[:winlen], computed in `dtype` (torch.float64 or torch.float32)."""
    ctype = torch.complex128 if dtype == torch.float64 else torch.complex64
    spec = torch.tensor(np.asarray(spec), dtype=dtype)
    aper = torch.tensor(np.asarray(aper), dtype=dtype)
    g = torch.tensor(np.asarray(g), dtype=dtype)
    K = L // 2 + 1
    k = torch.arange(K, dtype=dtype)
    d = rnd(0.001 * fs)
    hann = torch.as_tensor(np.hanning(2 * d + 1)[:d + 1], dtype=dtype)
    segs = []
    for r in rows:
        w = torch.tensor(r['w'], dtype=dtype)
        s = (1 - w) * spec[r['i0']] + w * spec[r['i1']]
        a = (1 - w) * aper[r['i0']] + w * aper[r['i1']]
        x = torch.zeros(L, dtype=dtype)
        n = r['rb'] - r['lb']
        if n > 0:
            q = g[r['lb']:r['rb']].clone()
            if n >= 2 * (d + 1):
                q[:d + 1] *= hann
                q[n - d - 1:] *= torch.flip(hann, [0])
            x[r['lb'] - r['start']:r['rb'] - r['start']] = q
        N = torch.fft.rfft(x)
        p = N.real ** 2 + N.imag ** 2
        e = (p[0] + p[-1] + 2 * p[1:-1].sum()) / L
        if float(e) > 0:
            N = N / torch.sqrt(e)
        S = minphase_restated(torch.log(torch.clamp(s * a, min=1e-10)), L) * N
        if r['v']:
            hp = torch.zeros(K, dtype=dtype)
            tc = torch.tan(torch.tensor(math.pi * 0.5 * r['f0'] / fs, dtype=dtype))
            hp[1:] = (1.0 + (tc / torch.tan(math.pi * k[1:] / L)) ** 8) ** -0.5
            Ep = minphase_restated(torch.log(torch.clamp(s * torch.sqrt(1 - a * a) * hp, min=1e-10)), L)
            S = S + Ep * torch.exp((-2j * math.pi * r['delay'] / L) * k.to(ctype))
        S[0] = S[0].real + 0j           # irfft reads the real part of bins 0 and L/2 only; said here, not left to the library
        S[-1] = S[-1].real + 0j
        segs.append(torch.fft.irfft(S, n=L)[:r['winlen']])
    return segs


def synth_restated(spec, aper, g, rows, fs, L, wavlen, dtype):
    wav = torch.zeros(wavlen, dtype=dtype)
    for s, r in zip(segments_restated(spec, aper, g, rows, fs, L, dtype), rows):
        a, b = max(r['start'], 0), min(r['start'] + r['winlen'], wavlen)
        if b > a:
            wav[a:b] += s[a - r['start']:b - r['start']]
    return wav.numpy()


def bound_of(want64, want32):
    want64 = np.asarray(want64, dtype=np.float64)
    e32 = float(np.abs(np.asarray(want32, dtype=np.float64) - want64).max()) if want64.size else 0.0
    return e32, 4.0 * e32 + 2.0 ** -23 * (float(np.abs(want64).max()) if want64.size else 0.0)


def check(got, want64, want32, what):
    """|got - want64| <= 4 e32 + 2^-23 max|want64|, every element."""
    got = np.asarray(got, dtype=np.float64)
    want64 = np.asarray(want64, dtype=np.float64)
    assert got.shape == want64.shape, (what, got.shape, want64.shape)
    e32, bound = bound_of(want64, want32)
    err = np.abs(got - want64)
    worst = float(err.max()) if err.size else 0.0
    print('{}: e32 = {:.3e}, kernel worst {:.3e}, bound {:.3e}, max|want| = {:.3e}'.format(
        what, e32, worst, bound, float(np.abs(want64).max()) if want64.size else 0.0))
    assert np.isfinite(got).all() and (err <= bound).all(), (what, e32, worst, bound)


# ---------------------------------------------------------------------------------------------------------------------------
# the two shapes; their references are computed once
# ---------------------------------------------------------------------------------------------------------------------------
SHIFT = 0.005
NS, NA = 9, 4
SHAPES = {'A': dict(fs=8000, L=512, T=40, unvoiced=[(0, 8), (26, 32)]),         # unvoiced start, both transitions, voiced end
          'B': dict(fs=32000, L=4096, T=24, unvoiced=[(10, 16)])}               # 72 KiB of LDS: two workgroups per CU
_cases = {}


def wavlen_of(T, fs):
    return int(round(SHIFT * (T - 1) * fs))


def make_inputs(name, T=None, voiced=None, seed=None):
    """f0 [T] (finite in unvoiced frames too), voiced [T], SPEC [T,K] (smooth, about 8 nepers of range, another one in every
    frame), aperiodicity bands [T,NA] in [-40, 0] dB with a few above 0 and one at -200, vuv [T] away from 0.5, g."""
    sh = SHAPES[name]
    fs, L = sh['fs'], sh['L']
    if voiced is None:
        voiced = np.ones(sh['T'] if T is None else T, dtype=bool)
        if T is None:
            for a, b in sh['unvoiced']:
                voiced[a:b] = False
    voiced = np.asarray(voiced, dtype=bool)
    T = len(voiced)
    K = L // 2 + 1
    rng = np.random.RandomState((41 if name == 'A' else 43) if seed is None else seed)
    f0 = (170.0 + 60.0 * np.sin(np.arange(T) / 7.0)).astype(np.float32)
    x = np.linspace(0, 1, K)
    la = np.zeros((T, K))
    for j in range(1, 6):
        la += rng.randn(T, 1) * np.cos(np.pi * j * x + rng.rand(T, 1) * 6.28) / j
    la = la - la.min()
    la = -9.0 + 8.0 * la / la.max()
    spec = np.exp(la).astype(np.float32)
    aper_db = rng.uniform(-40.0, 0.0, size=(T, NA))
    aper_db[rng.rand(T, NA) < 0.1] = 3.0                        # above 0 dB: clipped to 1
    vi = np.flatnonzero(voiced)
    aper_db[vi[len(vi) // 2] if len(vi) else T // 2, 1] = -200.0      # in a voiced frame where there is one
    aper_db = aper_db.astype(np.float32)
    vuv = np.where(voiced, 0.9, 0.1).astype(np.float32)
    wavlen = wavlen_of(T, fs)
    g = rng.randn(max(wavlen, 1))[:wavlen].astype(np.float32)
    aper = aper_restated(aper_db, vuv, fs, L, np.float64).astype(np.float32)     # what the segment kernel is given
    return dict(fs=fs, L=L, T=T, K=K, f0=f0, voiced=voiced, vuv=vuv, spec=spec, aper_db=aper_db, aper=aper, g=g, wavlen=wavlen)


def with_references(c):
    c['t'], c['rows'] = table_restated(c['f0'], c['voiced'], SHIFT, c['fs'], c['wavlen'], c['L'])
    c['wav64'] = synth_restated(c['spec'], c['aper'], c['g'], c['rows'], c['fs'], c['L'], c['wavlen'], torch.float64)
    c['wav32'] = synth_restated(c['spec'], c['aper'], c['g'], c['rows'], c['fs'], c['L'], c['wavlen'], torch.float32)
    for v in c.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return c


def case(name):
    if name not in _cases:
        _cases[name] = with_references(make_inputs(name))
    return _cases[name]


def flat_case():
    """All frames voiced, every frame's row the same: what the cross-check against the PML kernel needs."""
    if 'flat' not in _cases:
        c = make_inputs('A', voiced=np.ones(SHAPES['A']['T'], dtype=bool))
        c['spec'] = np.tile(c['spec'][:1], (c['T'], 1))
        c['aper'] = np.zeros_like(c['aper'])
        _cases['flat'] = with_references(c)
    return _cases['flat']


# ---------------------------------------------------------------------------------------------------------------------------
# CPU: the pulse table
# ---------------------------------------------------------------------------------------------------------------------------
INT_ROWS = ('start', 'winlen', 'lb', 'rb', 'fr', 'i0', 'i1', 'v')
DBL_ROWS = ('delay', 'f0', 'w')


@pytest.mark.parametrize('name', ['A', 'B'])
def test_world_pulse_table_matches_the_plain_loop(name):
    from percivaltts_amd import ops
    c = case(name)
    tab = ops.world_pulse_table(c['f0'], c['voiced'], SHIFT, c['fs'], c['wavlen'], c['L'])
    t, rows = c['t'], c['rows']
    P = len(rows)
    assert tab['t'].shape == (P,) and (np.diff(tab['t']) > 0).all() and tab['t'][-1] >= c['wavlen'] / float(c['fs'])
    np.testing.assert_array_equal(tab['t'], t)
    for key in INT_ROWS:
        assert tab[key].dtype == np.int32 and tab[key].shape == (P,)
        np.testing.assert_array_equal(tab[key], [r[key] for r in rows], err_msg=key)
    for key in DBL_ROWS:
        assert tab[key].dtype == np.float64
        np.testing.assert_array_equal(tab[key], [r[key] for r in rows], err_msg=key)
    assert (tab['winlen'] <= c['L']).all() and (tab['winlen'] % 2 == 1).all()        # f0 = 170 + 60 sin(i/7) fits shape A's 512
    assert (tab['rb'][:-1] == tab['lb'][1:]).all() and tab['lb'][0] == 0 and tab['rb'][-1] == c['wavlen']      # the noise tiles
    assert (tab['w'] >= 0).all() and (tab['w'] < 1).all() and (tab['w'] > 0).any()
    assert set(tab['v']) == {0, 1}
    np.testing.assert_array_equal(tab['f0'][tab['v'] == 0], 500.0)                   # noise in 2-ms pieces
    np.testing.assert_array_equal(tab['v'], c['voiced'][tab['fr']].astype(np.int32))


def low_onset():
    """Unvoiced frames, then voiced frames at 65 Hz: winlen grows from 401 to 493 samples at the onset."""
    fs, L, T = 8000, 1024, 30
    voiced = np.arange(T) >= 12
    return fs, L, T, np.full(T, 65.0), voiced, wavlen_of(T, fs)


def test_world_pulse_table_start_ascends():
    from percivaltts_amd import ops
    for name in ('A', 'B'):
        c = case(name)
        assert (np.diff([r['start'] for r in c['rows']]) >= 0).all()
    fs, L, T, f0, voiced, wavlen = low_onset()
    tab = ops.world_pulse_table(f0, voiced, SHIFT, fs, wavlen, L)
    assert (np.diff(tab['start']) >= 0).all() and tab['winlen'].max() == 493 and tab['winlen'].min() == 401
    # the PML table's lead, int(winlen / 4), would step backwards at the onset
    pml_start = tab['start'] + int(401 / 4) - (tab['winlen'] // 4)
    assert (np.diff(pml_start) < 0).any()


def test_world_pulse_table_all_voiced_equals_the_pml_table():
    from percivaltts_amd import ops
    c = case('A')
    assert c['f0'].min() >= 80.0
    tab = ops.world_pulse_table(c['f0'], np.ones(c['T'], dtype=bool), SHIFT, c['fs'], c['wavlen'], c['L'])
    pml = ops.pulse_table(c['f0'], SHIFT, c['fs'], c['wavlen'], c['L'])
    for key in ('t', 'start', 'winlen', 'lb', 'rb', 'fr', 'delay', 'f0'):
        assert tab[key].dtype == pml[key].dtype
        np.testing.assert_array_equal(tab[key], pml[key], err_msg=key)
    np.testing.assert_array_equal(tab['v'], 1)


def test_world_pulse_table_refuses_what_it_cannot_build():
    from percivaltts_amd import ops
    fs, T = 16000, 21
    wavlen = wavlen_of(T, fs)
    v = np.ones(T, dtype=bool)
    with pytest.raises(ValueError):                             # 0.05 * fs = 800 samples do not fit 512
        ops.world_pulse_table(np.full(T, 100.0), v, SHIFT, fs, wavlen, 512)
    with pytest.raises(ValueError):                             # 4 fs / 55 = 1163 samples do not fit 1024
        ops.world_pulse_table(np.full(T, 55.0), v, SHIFT, fs, wavlen, 1024)
    ops.world_pulse_table(np.full(T, 55.0), ~v, SHIFT, fs, wavlen, 1024)       # unvoiced: f0 is not looked at
    with pytest.raises(ValueError):                             # T < 1
        ops.world_pulse_table(np.zeros(0), np.zeros(0, dtype=bool), SHIFT, fs, 0, 1024)
    with pytest.raises(ValueError):
        ops.world_pulse_table(np.full(T, 100.0), v[:-1], SHIFT, fs, wavlen, 1024)
    with pytest.raises(ValueError):
        ops.world_pulse_table(np.full(T, 100.0), v, SHIFT, fs, wavlen + 1, 1024)
    with pytest.raises(ValueError):
        ops.world_pulse_table(np.full(T, 100.0), v, SHIFT, fs, wavlen, 1000)
    one = ops.world_pulse_table(np.array([100.0]), np.array([True]), SHIFT, fs, 0, 1024)
    assert one['start'].shape == (1,) and one['rb'][0] == 0 and one['w'][0] == 0.0 and one['i1'][0] == 0


# ---------------------------------------------------------------------------------------------------------------------------
# CPU: the restatement itself, the public interface
# ---------------------------------------------------------------------------------------------------------------------------
def test_restated_aper_rows_equal_interp():
    for name in ('A', 'B'):
        c = case(name)
        got = aper_restated(c['aper_db'], c['vuv'], c['fs'], c['L'], np.float64)
        fb = band_centres(NA, c['fs'])
        f = np.arange(c['K']) * float(c['fs']) / c['L']
        for t in range(c['T']):
            want = np.clip(np.interp(f, fb, 10.0 ** (c['aper_db'][t].astype(np.float64) / 20.0)), 0, 1) if c['voiced'][t] else np.ones(c['K'])
            np.testing.assert_allclose(got[t], want, rtol=0, atol=1e-12)
        assert got.min() >= 0 and got.max() == 1 and (got[~c['voiced']] == 1).all() and (got[c['voiced']] < 1).any()
        assert (c['aper_db'][c['voiced']] > 0).any() and (c['aper_db'][c['voiced']] == -200).any()


def test_restated_unvoiced_pulse_is_noise_only():
    c = case('A')
    r = next(r for r in c['rows'] if not r['v'] and r['rb'] - r['lb'] > 4)
    seg = segments_restated(c['spec'], c['aper'], np.zeros(c['wavlen']), [r], c['fs'], c['L'], torch.float64)[0].numpy()
    np.testing.assert_array_equal(seg, 0.0)
    r = next(r for r in c['rows'] if r['v'])
    seg = segments_restated(c['spec'], c['aper'], np.zeros(c['wavlen']), [r], c['fs'], c['L'], torch.float64)[0].numpy()
    assert np.abs(seg).max() > 1e-5


def test_interface():
    from percivaltts_amd import ops, ops_offline, vocoders
    assert list(inspect.signature(ops.world_pulse_table).parameters) == ['f0', 'voiced', 'shift', 'fs', 'wavlen', 'dftlen']
    assert list(inspect.signature(ops.aper_rows).parameters) == ['aper_db', 'vuv', 'fs', 'dftlen']
    assert inspect.signature(ops.aper_rows).parameters['dftlen'].default == 4096
    assert list(inspect.signature(ops.world_synthesis).parameters) == ['spec', 'aper', 'table', 'noise', 'fs', 'dftlen', 'wavlen']
    for name in ('world_pulse_table', 'aper_rows', 'world_synthesis'):
        assert getattr(ops, name) is getattr(ops_offline, name) and name in ops_offline.__all__
    voc = vocoders.VocoderWORLDDevice(8000, SHIFT, 12, NA, dftlen=512)
    assert isinstance(voc, vocoders.VocoderWORLD) and voc.featuressizeraw() == 1 + 12 + NA + 1 and voc.name() == 'WORLD'
    assert list(inspect.signature(voc.synthesis_device).parameters) == ['CMP', 'pp_mcep', 'pp_f0_smooth', 'noise']
    assert not hasattr(vocoders.VocoderWORLD(8000, SHIFT, 12, NA), 'synthesis_device')
    assert not hasattr(voc, 'analysis_device')
    with pytest.raises(NotImplementedError):
        voc.synthesis(None)
    with pytest.raises(ValueError):
        voc.synthesis_device(np.zeros((4, voc.featuressizeraw()), dtype=np.float32), pp_f0_smooth=0.1)
    with pytest.raises(ValueError):
        voc.synthesis_device(np.zeros((4, voc.featuressizeraw() + 1), dtype=np.float32))


# ---------------------------------------------------------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------------------------------------------------------
def _dev(a, dtype=torch.float32):
    return torch.tensor(np.asarray(a), dtype=dtype).cuda().contiguous()


def _table(c):
    from percivaltts_amd import ops
    return ops.world_pulse_table(c['f0'], c['voiced'], SHIFT, c['fs'], c['wavlen'], c['L'])


def _synth(c, aper=None, g=None, tab=None):
    from percivaltts_amd import ops
    wav = ops.world_synthesis(_dev(c['spec']), _dev(c['aper']) if aper is None else aper, _table(c) if tab is None else tab,
                              _dev(c['g'] if g is None else g), c['fs'], c['L'], c['wavlen'])
    assert wav.dtype == torch.float32 and wav.is_cuda and tuple(wav.shape) == (c['wavlen'],)
    return wav.cpu().numpy()


@pytest.mark.gpu
@pytest.mark.parametrize('name', ['A', 'B'])
def test_aper_rows_against_restatement(name):
    from percivaltts_amd import ops
    c = case(name)
    got = ops.aper_rows(_dev(c['aper_db']), _dev(c['vuv']), c['fs'], c['L'])
    assert tuple(got.shape) == (c['T'], c['K']) and got.dtype == torch.float32
    want64 = aper_restated(c['aper_db'], c['vuv'], c['fs'], c['L'], np.float64)
    want32 = aper_restated(c['aper_db'], c['vuv'], c['fs'], c['L'], np.float32)
    got = got.cpu().numpy()
    check(got, want64, want32, 'aper_rows ' + name)
    assert (got[~c['voiced']] == 1).all() and got.min() >= 0 and got.max() <= 1


@pytest.mark.gpu
@pytest.mark.parametrize('name', ['A', 'B'])
def test_world_synthesis_against_restatement(name):
    c = case(name)
    got = _synth(c)
    assert np.abs(c['wav64']).max() > 1e-3
    check(got, c['wav64'], c['wav32'], 'world_synthesis ' + name)
    np.testing.assert_array_equal(got, _synth(c))               # same input, same bytes


@pytest.mark.gpu
def test_world_synthesis_short_utterances():
    from percivaltts_amd import _hip, ops
    one = make_inputs('A', voiced=[True])
    assert one['wavlen'] == 0
    with _hip.KernelTimer() as kt:
        wav = ops.world_synthesis(_dev(one['spec']), _dev(one['aper']), _table(one), _dev(one['g']), one['fs'], one['L'], 0)
    assert tuple(wav.shape) == (0,) and kt.records == []
    for voiced in ([False, True], [True, False, True]):
        c = with_references(make_inputs('A', voiced=voiced))
        assert len(c['rows']) >= 3
        check(_synth(c), c['wav64'], c['wav32'], 'world_synthesis A, T = {}'.format(len(voiced)))


@pytest.mark.gpu
def test_world_synthesis_unvoiced_means_no_pulse():
    """With every frame unvoiced the aperiodicity columns are not looked at: two different inputs, the same bytes, and the
    waveform follows the noise alone."""
    from percivaltts_amd import ops
    c = make_inputs('A', voiced=np.zeros(SHAPES['A']['T'], dtype=bool))
    tab = _table(c)
    assert (tab['v'] == 0).all()
    other_db = np.random.RandomState(7).uniform(-60, -10, size=c['aper_db'].shape).astype(np.float32)
    a = ops.aper_rows(_dev(c['aper_db']), _dev(c['vuv']), c['fs'], c['L'])
    b = ops.aper_rows(_dev(other_db), _dev(c['vuv']), c['fs'], c['L'])
    wa, wb = _synth(c, aper=a, tab=tab), _synth(c, aper=b, tab=tab)
    np.testing.assert_array_equal(wa, wb)
    assert np.abs(wa).max() > 1e-4
    np.testing.assert_array_equal(_synth(c, aper=a, tab=tab, g=np.zeros(c['wavlen'], dtype=np.float32)), 0.0)


@pytest.mark.gpu
def test_world_synthesis_agrees_with_the_pml_kernel():
    """All frames voiced and alike, aperiodicity exactly 0 here, mask exactly 0 there, the same table rows and noise: both
    kernels compute irfft(E D), and this one adds the aperiodic branch at its floor.  That floor is 1e-10 |N| with N at unit mean
    energy: at most 1e-10 * 2K / L per segment sample, and at most about ten segments cover one sample, hence 1e-9."""
    from percivaltts_amd import ops
    c = flat_case()
    tab = _table(c)
    zeros = torch.zeros((c['T'], c['K']), dtype=torch.float32, device='cuda')
    got = _synth(c, aper=zeros, tab=tab)
    pml = ops.pulse_synthesis(_dev(c['spec']), zeros, tab, _dev(c['g']), c['fs'], c['L'], c['wavlen']).cpu().numpy()
    e32, bound = bound_of(c['wav64'], c['wav32'])
    diff = float(np.abs(got.astype(np.float64) - pml.astype(np.float64)).max())
    print('world vs pml: e32 = {:.3e}, largest difference {:.3e}, bound {:.3e} + 1e-9'.format(e32, diff, bound))
    assert np.abs(pml).max() > 1e-3 and diff <= bound + 1e-9
    check(got, c['wav64'], c['wav32'], 'world_synthesis, flat')


@pytest.mark.gpu
def test_ops_argument_checks_on_device():
    from percivaltts_amd import _hip, ops
    c = case('A')
    tab = _table(c)
    spec, aper, g = _dev(c['spec']), _dev(c['aper']), _dev(c['g'])
    args = (c['fs'], c['L'], c['wavlen'])
    with pytest.raises(_hip.HipLibraryError):
        ops.world_synthesis(spec.cpu(), aper, tab, g, *args)
    with pytest.raises(_hip.HipLibraryError):
        ops.world_synthesis(spec, aper.double(), tab, g, *args)
    with pytest.raises(_hip.HipLibraryError):
        ops.world_synthesis(spec, aper.t().contiguous().t(), tab, g, *args)
    with pytest.raises(ValueError):
        ops.world_synthesis(spec, aper[:, :-1].contiguous(), tab, g, *args)
    with pytest.raises(ValueError):
        ops.world_synthesis(spec, aper, tab, g[:-1].contiguous(), *args)
    with pytest.raises(ValueError):
        ops.world_synthesis(spec.clone().requires_grad_(True), aper, tab, g, *args)
    with pytest.raises(ValueError):                             # a table built for another transform length
        ops.world_synthesis(spec, aper, dict(tab, winlen=tab['winlen'] + 2 * c['L']), g, *args)
    with pytest.raises(ValueError):                             # descending start samples
        ops.world_synthesis(spec, aper, dict(tab, start=tab['start'][::-1].copy()), g, *args)
    with pytest.raises(ValueError):                             # a frame outside the rows given
        ops.world_synthesis(spec, aper, dict(tab, i1=tab['i1'] + 1), g, *args)
    with pytest.raises(ValueError):                             # the PML table has no i0 / i1 / w / v
        ops.world_synthesis(spec, aper, ops.pulse_table(c['f0'], SHIFT, c['fs'], c['wavlen'], c['L']), g, *args)
    db, vuv = _dev(c['aper_db']), _dev(c['vuv'])
    with pytest.raises(_hip.HipLibraryError):
        ops.aper_rows(db.cpu(), vuv, c['fs'], c['L'])
    with pytest.raises(_hip.HipLibraryError):
        ops.aper_rows(db, vuv.double(), c['fs'], c['L'])
    with pytest.raises(_hip.HipLibraryError):
        ops.aper_rows(db.t().contiguous().t(), vuv, c['fs'], c['L'])
    with pytest.raises(ValueError):
        ops.aper_rows(db, vuv[:-1].contiguous(), c['fs'], c['L'])
    with pytest.raises(ValueError):
        ops.aper_rows(db, vuv, c['fs'], 500)
    with pytest.raises(ValueError):
        ops.aper_rows(db.clone().requires_grad_(True), vuv, c['fs'], c['L'])
    # the C ABI refuses a transform length it has no kernel for, without a launch
    l = _hip.lib()
    assert l.ptts_world_segments(None, None, None, None, None, 1, 1, 768, 8000.0, 10, None, 64, None) != 0
    assert l.ptts_world_segments(None, None, None, None, None, 0, 1, 512, 8000.0, 10, None, 64, None) == 0
    assert l.ptts_world_segments(None, None, None, None, None, 1, 0, 512, 8000.0, 10, None, 64, None) == 0
    assert l.ptts_aper_rows(None, None, None, 0, NA, 8000.0, 512, None, 0, None) == 0
    assert l.ptts_aper_rows(None, None, None, 1, NA, 8000.0, 768, None, 0, None) != 0


def _cmp_of(c, voc):
    """[T, 1 + spec_size + NA + 1] WORLD parameters whose decompressed envelope is moderate."""
    rng = np.random.RandomState(5)
    spec = -4.0 + np.cumsum(rng.randn(c['T'], voc.spec_size) * 0.3, axis=1)
    return np.concatenate([np.log(c['f0'].astype(np.float64))[:, None], spec, c['aper_db'], c['vuv'][:, None]], axis=1).astype(np.float32)


@pytest.mark.gpu
def test_synthesis_device_is_the_chain_and_follows_the_seed():
    from percivaltts_amd import ops, vocoders
    c = case('A')
    voc = vocoders.VocoderWORLDDevice(c['fs'], SHIFT, NS, NA, dftlen=c['L'])
    CMP = _cmp_of(c, voc)
    assert CMP.shape == (c['T'], 1 + NS + NA + 1)
    # a caller's noise: the chain of the public ops, byte for byte
    got = voc.synthesis_device(CMP, noise=_dev(c['g']))
    assert got.dtype == np.float32 and got.shape == (c['wavlen'],)
    d = _dev(CMP)
    f0 = torch.exp(d[:, 0]).cpu().numpy()
    spec = voc.decompress_spectrum(d[:, 1:1 + NS].contiguous())
    aper = ops.aper_rows(d[:, 1 + NS:1 + NS + NA].contiguous(), d[:, -1].contiguous(), c['fs'], c['L'])
    tab = ops.world_pulse_table(f0, c['voiced'], SHIFT, c['fs'], c['wavlen'], c['L'])
    want = ops.world_synthesis(spec, aper, tab, _dev(c['g']), c['fs'], c['L'], c['wavlen']).cpu().numpy()
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
    from percivaltts_amd import modeltts_common, ops, vocoders
    ctx, fs, L = 19, 8000, 512
    voc = vocoders.VocoderWORLDDevice(fs, SHIFT, 12, NA, dftlen=L, mlpg_wins=wins)
    mod = modeltts_common.Generic(ctx, voc, layertypes=['FC', 'BLSTM'], cfgarch=_small_cfg())
    rng = np.random.RandomState(0)
    nout, nraw = voc.featuressize(), voc.featuressizeraw()
    lens = [41, 23, 9]
    (tmp_path / 'lab').mkdir(); (tmp_path / 'cmp').mkdir()
    fids = ['utt_{:02d}'.format(i) for i in range(len(lens))]
    for fid, n in zip(fids, lens):
        (rng.rand(n, ctx) * 2 - 1).astype(np.float32).tofile(str(tmp_path / 'lab' / (fid + '.lab')))
    mean = (rng.randn(nout) * 0.3).astype(np.float32)
    mean[0] = np.log(170.0)                                     # log f0: keeps winlen within dftlen
    mean[13:13 + NA] = -15.0                                    # aperiodicity in dB
    mean[nraw - 1] = 0.45                                       # the vuv head is a sigmoid: 0.45 + 0.1 * (0 .. 1)
    std = np.full(nout, 0.1, dtype=np.float32)
    mean.tofile(str(tmp_path / 'cmp' / 'mean4norm.dat')); std.tofile(str(tmp_path / 'cmp' / 'std4norm.dat'))
    inpath = str(tmp_path / 'lab') + '/*.lab:(-1,{})'.format(ctx)
    outpath = str(tmp_path / 'cmp') + '/*.cmp:(-1,{})'.format(nout)
    # the parameters alone first: the vuv mean is then moved so that the first utterance's median frame sits on the threshold
    # (the de-normalisation and MLPG are linear in the mean), which gives that utterance voiced and unvoiced frames
    mod.generate_params(inpath, outpath, fids[:1], str(tmp_path / 'gen0'), do_objmeas=False)
    assert not (tmp_path / 'wav').exists()
    vuv0 = np.fromfile(str(tmp_path / 'gen0' / (fids[0] + '.cmp')), dtype=np.float32).reshape(lens[0], nraw)[:, -1]
    mean[nraw - 1] += 0.5 - float(np.median(vuv0))
    mean.tofile(str(tmp_path / 'cmp' / 'mean4norm.dat'))

    for sub in ('wav', 'wav2'):
        ops.rng_seed(77)
        mod.generate_params(inpath, outpath, fids, str(tmp_path / 'gen'), do_objmeas=False, batch_size=2, wavdir=str(tmp_path / sub))
    for fid, n in zip(fids, lens):
        with wave.open(str(tmp_path / 'wav' / (fid + '.wav')), 'rb') as f:
            assert (f.getnchannels(), f.getsampwidth(), f.getframerate()) == (1, 2, fs)
            assert f.getnframes() == wavlen_of(n, fs)
            pcm = np.frombuffer(f.readframes(f.getnframes()), dtype='<i2')
        assert np.abs(pcm).max() > 0
        with open(str(tmp_path / 'wav' / (fid + '.wav')), 'rb') as f1, open(str(tmp_path / 'wav2' / (fid + '.wav')), 'rb') as f2:
            assert f1.read() == f2.read()                       # the same seed, the same files
        gen = np.fromfile(str(tmp_path / 'gen' / (fid + '.cmp')), dtype=np.float32).reshape(n, nraw)
        print('{}: {} of {} frames voiced'.format(fid, int((gen[:, -1] >= 0.5).sum()), n))
        if fid == fids[0]:
            assert 0 < int((gen[:, -1] >= 0.5).sum()) < n
