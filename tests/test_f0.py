"""F0 estimation (csrc/f0.hip; ops.f0_check / f0_window_table / f0_candidates / f0_viterbi / f0_estimate,
VocoderF0Spec.f0_estimate_device, the f0=None paths of VocoderPML.analysis_device / analysisf_device / analysisfid_device and of
run.features_extraction).

The reference runs an external pitch tracker that is absent from its checkout, so there is nothing of it to compare with: the
estimator is the build's own (after Boersma 1993: the autocorrelation method with a path finder) and is restated
here in plain numpy loops, in a chosen dtype, with torch.fft.rfft / irfft for the transforms (they keep the dtype).  Integer decisions
(sample indices, the window length, the lag range) are taken in float64 in both dtypes; the two tables (the window's own
autocorrelation and the low-pass weight) are float64 tables rounded to the dtype, not data.

Tolerance of the device results: the rule of tests/test_pulsesynth.py (`check` there): within 4 * e32 + 2^-23 * max|want64| of the
float64 restatement, e32 being the error of the float32 restatement on the same input.  Lags, counts and paths are compared exactly:
test_float32_and_float64_restatements_decide_alike shows that the two restatements take the same decisions on these signals.

The test signals are the float64 synthesis restatement of tests/test_pulsesynth.py: a pulse train below fs/5 and noise above, a
stretch of noise only (unvoiced) in the middle and silence at the end."""
import inspect
import itertools
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_pulsesynth as ps                                    # noqa: E402  (the synthesis restatement, `check`, the two shapes)

check, rnd = ps.check, ps.rnd
SHIFT, SHAPES = ps.SHIFT, ps.SHAPES
F0_MIN, F0_MAX = 100.0, 400.0
NCAND = 8
VOICING_THRESHOLD, SILENCE_THRESHOLD = 0.45, 0.03
OCTAVE_COST, OCTAVE_JUMP_COST, VOICED_UNVOICED_COST = 0.01, 0.35, 0.14
MAX_FRAMES = 32768
GROSS = 0.2                                                     # gross pitch error: |f^ / f - 1| > 0.2


# ---------------------------------------------------------------------------------------------------------------------------
# the definition, restated
# ---------------------------------------------------------------------------------------------------------------------------
def geometry(fs, f0_min, f0_max):
    """(hw, W, lmin, lmax)"""
    hw = int(1.5 * fs / f0_min)
    return hw, 2 * hw + 1, int(math.ceil(fs / f0_max)), int(math.floor(fs / f0_min))


def window_restated(W):
    return np.array([0.5 - 0.5 * math.cos(2.0 * math.pi * (j + 1) / (W + 1)) for j in range(W)])


def window_autocorrelation(w, lmax):
    e = float(np.dot(w, w))
    return np.array([float(np.dot(w[:len(w) - k], w[k:])) / e for k in range(lmax + 2)])


def lowpass_restated(fs, L, f0_max):
    flp = 2.5 * f0_max
    G = np.zeros(L // 2 + 1)
    for k in range(L // 2 + 1):
        f = k * float(fs) / L
        if f <= flp: G[k] = 1.0
        elif f < 1.5 * flp: G[k] = math.cos(math.pi * (f - flp) / flp) ** 2
    return G


def frames_restated(wav, T, shift, fs, L, f0_min, f0_max, dtype):
    """wav [N] -> (r [T, lmax+2], lpeak [T]) in `dtype`."""
    hw, W, lmin, lmax = geometry(fs, f0_min, f0_max)
    assert W + lmax + 1 <= L
    wav = np.asarray(wav, dtype=dtype)
    N = len(wav)
    w64 = window_restated(W)
    w, rw, G = w64.astype(dtype), window_autocorrelation(w64, lmax).astype(dtype), lowpass_restated(fs, L, f0_max).astype(dtype)
    r, lpeak = np.zeros((T, lmax + 2), dtype=dtype), np.zeros(T, dtype=dtype)
    for i in range(T):
        c = rnd(i * shift * fs)
        j0, j1 = max(0, hw - c), min(W, N - c + hw)
        a = np.zeros(W, dtype=dtype)
        if j1 > j0:
            seg = wav[c - hw + j0:c - hw + j1]
            a[j0:j1] = seg - seg.mean(dtype=dtype)
        lpeak[i] = np.abs(a).max()
        x = np.zeros(L, dtype=dtype)
        x[:W] = a * w
        X = torch.fft.rfft(torch.from_numpy(x))
        P = torch.from_numpy(G) * (X.real ** 2 + X.imag ** 2)
        rho = torch.fft.irfft(torch.complex(P, torch.zeros_like(P)), n=L).numpy()
        assert rho.dtype == dtype
        if rho[0] > 0:
            r[i] = (rho[:lmax + 2] / rho[0]) / rw
    return r, lpeak


def candidates_restated(r, lpeak, gpeak, fs, f0_min, f0_max, ncand, dtype, voicing_threshold=VOICING_THRESHOLD,
                        silence_threshold=SILENCE_THRESHOLD, octave_cost=OCTAVE_COST):
    """r [T, lmax+2], lpeak [T] -> freq, strength [T, ncand] in `dtype`, n [T], lag [T, ncand]."""
    dt = np.dtype(dtype).type
    _, _, lmin, lmax = geometry(fs, f0_min, f0_max)
    T = r.shape[0]
    freq, strength = np.zeros((T, ncand), dtype=dtype), np.zeros((T, ncand), dtype=dtype)
    n, lag = np.zeros(T, dtype=np.int32), np.zeros((T, ncand), dtype=np.int32)
    vt = dt(voicing_threshold)
    for i in range(T):
        if gpeak == 0:
            strength[i, 0] = vt + dt(2)
        else:
            strength[i, 0] = vt + max(dt(0), dt(2) - (lpeak[i] / dt(gpeak)) / (dt(silence_threshold) / (dt(1) + vt)))
        found = []
        for k in range(max(lmin, 1), lmax + 1):
            a, b, c = r[i, k - 1], r[i, k], r[i, k + 1]
            if not (b > a and b >= c and b > dt(0.5) * vt):
                continue
            d = a - dt(2) * b + c
            delta = dt(0.5) * (a - c) / d if d < 0 else dt(0)
            peak = b - dt(0.25) * (a - c) * delta
            tau = (dt(k) + delta) / dt(fs)
            F = dt(1) / tau
            if not dt(f0_min) <= F <= dt(f0_max):
                continue
            found.append((-(min(peak, dt(1)) - dt(octave_cost) * np.log2(dt(f0_min) * tau)), k, F))
        found.sort(key=lambda e: (e[0], e[1]))
        found = found[:ncand - 1]
        n[i] = len(found)
        for s, (negS, k, F) in enumerate(found):
            freq[i, 1 + s], strength[i, 1 + s], lag[i, 1 + s] = F, -negS, k
    return freq, strength, n, lag


def transition(lf, p, j, ojc, vuc, dt):
    """The cost of going from slot p of one frame to slot j of the next; lf: the two frames' log2 F rows."""
    if p == 0 and j == 0: return dt(0)
    if p == 0 or j == 0: return dt(vuc)
    return dt(ojc) * abs(lf[0][p] - lf[1][j])


def log2_rows(freq, n, dtype):
    lf = np.zeros(freq.shape, dtype=dtype)
    for i in range(freq.shape[0]):
        lf[i, 1:1 + n[i]] = np.log2(freq[i, 1:1 + n[i]].astype(dtype))
    return lf


def viterbi_restated(freq, strength, n, shift, dtype, octave_jump_cost=OCTAVE_JUMP_COST, voiced_unvoiced_cost=VOICED_UNVOICED_COST):
    """-> (path [T] of slots, f0 [T] in the dtype of freq, the path's cost)."""
    dt = np.dtype(dtype).type
    T = freq.shape[0]
    S, lf, corr = strength.astype(dtype), log2_rows(freq, n, dtype), dt(0.01 / shift)
    cost = [-S[0, j] for j in range(n[0] + 1)]
    back = []
    for i in range(1, T):
        new, bp = [], []
        for j in range(n[i] + 1):
            best, arg = None, 0
            for p in range(n[i - 1] + 1):
                v = cost[p] + corr * transition((lf[i - 1], lf[i]), p, j, octave_jump_cost, voiced_unvoiced_cost, dt)
                if best is None or v < best:
                    best, arg = v, p
            new.append(best - S[i, j])
            bp.append(arg)
        cost = new
        back.append(bp)
    j = int(np.argmin(np.array(cost)))                          # the first of equal minima
    total = cost[j]
    path = [j]
    for bp in reversed(back):
        j = bp[j]
        path.append(j)
    path = np.array(path[::-1], dtype=np.int64)
    return path, freq[np.arange(T), path], float(total)


def path_cost(path, freq, strength, n, shift, octave_jump_cost=OCTAVE_JUMP_COST, voiced_unvoiced_cost=VOICED_UNVOICED_COST):
    """The float64 cost of a given path; None when it uses a slot behind a frame's count."""
    if any(not 0 <= path[i] <= n[i] for i in range(len(path))):
        return None
    S, lf, corr = strength.astype(np.float64), log2_rows(freq, n, np.float64), 0.01 / shift
    total = -S[0, path[0]]
    for i in range(1, len(path)):
        total = total + corr * transition((lf[i - 1], lf[i]), path[i - 1], path[i], octave_jump_cost, voiced_unvoiced_cost, np.float64)
        total = total - S[i, path[i]]
    return float(total)


def global_peak(wav32):
    x = np.asarray(wav32, dtype=np.float64)
    return float(np.abs(x - x.mean()).max()) if x.size else 0.0


def estimate_restated(wav, T, shift, fs, L, f0_min, f0_max, ncand, dtype):
    """The whole chain in `dtype` on the float32 samples a kernel would be given.  The path finder reads the float32 tables."""
    wav32 = np.asarray(wav, dtype=np.float32)
    r, lpeak = frames_restated(wav32, T, shift, fs, L, f0_min, f0_max, dtype)
    freq, strength, n, lag = candidates_restated(r, lpeak, global_peak(wav32), fs, f0_min, f0_max, ncand, dtype)
    path, f0, cost = viterbi_restated(freq.astype(np.float32), strength.astype(np.float32), n, shift, dtype)
    return dict(r=r, lpeak=lpeak, freq=freq, strength=strength, n=n, lag=lag, path=path, f0=f0, cost=cost)


# ---------------------------------------------------------------------------------------------------------------------------
# the two test signals; they and their references are computed once
# ---------------------------------------------------------------------------------------------------------------------------
SIGNALS = {'A': dict(T=120, noise=(50, 70), silence=100), 'B': dict(T=60, noise=(25, 35), silence=50)}
_cases = {}


def case(name):
    if name not in _cases:
        sg = SIGNALS[name]
        T = sg['T']
        c = dict(ps.make_inputs(name, T))
        K, fs, L = c['K'], c['fs'], c['L']
        la, x = np.log(c['spec'][[0, -1]].astype(np.float64)), np.linspace(0, 1, T)[:, None]
        spec = np.exp((1 - x) * la[0] + x * la[1]).astype(np.float32)
        mask = np.tile((np.arange(K) * float(fs) / L >= fs / 5.0).astype(np.float32), (T, 1))
        mask[sg['noise'][0]:sg['noise'][1]] = 1.0
        rows = ps.table_restated(c['f0'], SHIFT, fs, c['wavlen'], L)[1]
        wav = ps.synth_restated(spec, mask, c['g'], rows, fs, L, c['wavlen'], torch.float64).copy()
        wav[rnd(sg['silence'] * SHIFT * fs):] = 0.0
        c['wav'] = wav.astype(np.float32)
        c['truth'] = np.array([not sg['noise'][0] <= i < sg['noise'][1] and i < sg['silence'] for i in range(T)])
        c['bounds'] = sg['noise'] + (sg['silence'],)               # the first frame of every stretch after the first
        c['gpeak'] = global_peak(c['wav'])
        assert rnd((T - 1) * SHIFT * fs) <= len(c['wav']) < rnd(T * SHIFT * fs)         # T frames by the cropping rule
        for tag, dtype in (('64', np.float64), ('32', np.float32)):
            c[tag] = estimate_restated(c['wav'], T, SHIFT, fs, L, F0_MIN, F0_MAX, NCAND, dtype)
        for v in list(c.values()) + list(c['64'].values()) + list(c['32'].values()):
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _cases[name] = c
    return _cases[name]


def near(c, m):
    """The m frames on either side of every voicing boundary."""
    return np.array([any(b - m <= i < b + m for b in c['bounds']) for i in range(c['T'])])


def excluded(c):
    """The frames left out of the voicing comparison: the two on either side of every voicing boundary, or only the one on either
    side where two would be more than a tenth of the frames (signal B, three boundaries in 60 frames)."""
    return near(c, 2) if near(c, 2).sum() <= 0.1 * c['T'] else near(c, 1)


# ---------------------------------------------------------------------------------------------------------------------------
# CPU: the restatement
# ---------------------------------------------------------------------------------------------------------------------------
def test_restated_pure_harmonic_sum():
    fs, L, T = 8000, 512, 40
    n = np.arange(rnd((T - 1) * SHIFT * fs) + 1)
    wav = sum(np.cos(2 * np.pi * 150.0 * h * n / fs) / h for h in range(1, 6))
    e = estimate_restated(wav, T, SHIFT, fs, L, F0_MIN, F0_MAX, NCAND, np.float64)
    hw = geometry(fs, F0_MIN, F0_MAX)[0]
    inside = [i for i in range(T) if rnd(i * SHIFT * fs) - hw >= 0 and rnd(i * SHIFT * fs) + hw < len(n)]
    assert len(inside) >= 30
    print('harmonic sum: best candidate {:.4f} .. {:.4f} Hz, strength >= {:.4f}'.format(
        e['freq'][inside, 1].min(), e['freq'][inside, 1].max(), e['strength'][inside, 1].min()))
    assert (e['n'][inside] >= 1).all()
    assert np.abs(e['freq'][inside, 1] - 150.0).max() <= 0.1
    assert e['strength'][inside, 1].min() >= 1.0
    assert (e['f0'][inside] == e['freq'][inside, 1].astype(np.float32)).all()


@pytest.mark.parametrize('name', ['A', 'B'])
def test_restated_voicing_follows_the_signal(name):
    c = case(name)
    out = excluded(c)
    assert out.sum() <= 0.1 * c['T'] and out.sum() == (12 if name == 'A' else 6)
    voiced = c['64']['f0'] > 0
    wrong = [i for i in range(c['T']) if voiced[i] != c['truth'][i]]
    print('{}: voicing differs from the truth at frames {}; {} frames excluded'.format(name, wrong, int(out.sum())))
    assert not [i for i in wrong if not out[i]]
    assert 0.5 < c['truth'].mean() < 0.9 and (c['64']['lpeak'][-5:] == 0).all()


@pytest.mark.parametrize('name', ['A', 'B'])
def test_restated_has_no_gross_pitch_error(name):
    c = case(name)
    both = (c['64']['f0'] > 0) & c['truth']
    rel = np.abs(c['64']['f0'][both].astype(np.float64) / c['f0'][both].astype(np.float64) - 1.0)
    print('{}: relative F0 error over {} frames: mean {:.4f}, largest {:.4f}'.format(name, int(both.sum()), rel.mean(), rel.max()))
    assert both.sum() >= 0.5 * c['T'] and rel.max() <= GROSS


@pytest.mark.parametrize('name', ['A', 'B'])
def test_float32_and_float64_restatements_decide_alike(name):
    c = case(name)
    a, b = c['64'], c['32']
    np.testing.assert_array_equal(a['n'], b['n'])
    np.testing.assert_array_equal(a['lag'], b['lag'])
    np.testing.assert_array_equal(a['path'], b['path'])
    gaps = [np.diff(-a['strength'][i, 1:1 + a['n'][i]]).min() for i in range(c['T']) if a['n'][i] > 1]
    e32 = np.abs(b['r'].astype(np.float64) - a['r']).max()
    print('{}: e32 of r {:.3e}, smallest gap between ranked strengths {:.3e}, at most {} candidates'.format(
        name, e32, min(gaps), a['n'].max()))
    assert min(gaps) > 100 * e32 and a['n'].max() >= 3


def random_table(T, ncand, seed):
    rng = np.random.RandomState(seed)
    n = rng.randint(0, ncand, size=T).astype(np.int32)
    freq = rng.uniform(100.0, 400.0, size=(T, ncand)).astype(np.float32)
    strength = rng.uniform(0.0, 1.2, size=(T, ncand)).astype(np.float32)
    for i in range(T):
        freq[i, 0] = 0.0
        freq[i, 1 + n[i]:] = 0.0
        strength[i, 1 + n[i]:] = 0.0
    return freq, strength, n


def test_restated_viterbi_against_brute_force():
    for seed in range(5):
        freq, strength, n = random_table(6, 3, seed)
        path, f0, cost = viterbi_restated(freq, strength, n, SHIFT, np.float64)
        costs = {p: path_cost(p, freq, strength, n, SHIFT) for p in itertools.product(range(3), repeat=6)}
        valid = {p: v for p, v in costs.items() if v is not None}
        assert len(valid) == int(np.prod(n + 1))
        best = min(valid.values())
        assert abs(cost - best) <= 1e-12 * abs(best) and abs(valid[tuple(path)] - best) <= 1e-12 * abs(best)
        np.testing.assert_array_equal(f0, freq[np.arange(6), path])


# ---------------------------------------------------------------------------------------------------------------------------
# CPU: the host side and the public interface
# ---------------------------------------------------------------------------------------------------------------------------
def test_f0_check_frame_count_and_window_table():
    from percivaltts_amd import ops
    assert ops.f0_check(512, 8000, SHIFT, F0_MIN, F0_MAX) == (120, 20, 80)
    assert ops.f0_check(4096, 32000, SHIFT, F0_MIN, F0_MAX) == (480, 80, 320)
    assert ops.f0_check(4096, 16000, SHIFT, 70, 600) == (342, 27, 228)
    ops.analysis_check(512, 8000, SHIFT, 60.0, F0_MAX)          # the analysis window at 60 Hz fits 512 ...
    with pytest.raises(ValueError, match='longest lag'):        # ... 401 samples and a lag of 133 do not
        ops.f0_check(512, 8000, SHIFT, 60.0, F0_MAX)
    for bad in ((500, 8000, SHIFT, F0_MIN, F0_MAX), (512, 8000, 0.0, F0_MIN, F0_MAX), (512, 8000, SHIFT, 200.0, 100.0),
                (512, 8000, SHIFT, F0_MIN, 2000.0)):
        with pytest.raises(ValueError):
            ops.f0_check(*bad)
    for N, fs in ((0, 8000), (39, 8000), (40, 8000), (4760, 8000), (4761, 8000), (12345, 44100), (100000, 32000)):
        T = ops.f0_frame_count(N, SHIFT, fs)
        assert rnd((T - 1) * SHIFT * fs) <= N < rnd(T * SHIFT * fs), (N, fs, T)
    assert ops.f0_frame_count(0, SHIFT, 8000) == 1 and ops.f0_frame_count(40, SHIFT, 8000) == 2
    with pytest.raises(ValueError):
        ops.f0_frame_count(-1, SHIFT, 8000)
    rw = ops.f0_window_table(8000, F0_MIN, F0_MAX)
    want = window_autocorrelation(window_restated(241), 80)
    assert rw.dtype == np.float64 and rw.shape == (82,) and rw[0] == 1.0 and (np.diff(rw) < 0).all() and rw[-1] > 0.4
    np.testing.assert_allclose(rw, want, rtol=1e-14)
    assert ops.f0_window_table(8000, F0_MIN, 300.0) is rw       # kept: the table does not depend on f0_max
    with pytest.raises(ValueError):
        ops.f0_window_table(8000, 0.0, F0_MAX)
    assert ops.F0_CONSTANTS == dict(voicing_threshold=VOICING_THRESHOLD, silence_threshold=SILENCE_THRESHOLD, octave_cost=OCTAVE_COST,
                                    octave_jump_cost=OCTAVE_JUMP_COST, voiced_unvoiced_cost=VOICED_UNVOICED_COST)
    assert (ops.F0_MIN_NCAND, ops.F0_MAX_NCAND, ops.F0_MAX_FRAMES) == (2, 16, MAX_FRAMES)


def test_argument_checks_without_a_device():
    from percivaltts_amd import ops, vocoders
    wav = torch.zeros(400)
    geo = (SHIFT, 8000, 512, F0_MIN, F0_MAX)
    for kw in (dict(ncand=1), dict(ncand=17), dict(ncand=2.5), dict(voicing_threshold=0.0), dict(silence_threshold=-1.0),
               dict(octave_cost=float('nan'))):
        with pytest.raises(ValueError):
            ops.f0_candidates(wav, 3, *geo, 1.0, **kw)
    for args in ((torch.zeros(2, 200), 3) + geo + (1.0,), (wav, -1) + geo + (1.0,), (wav, 3) + geo + (-1.0,),
                 (wav, 3) + geo + (float('inf'),), (wav, 3, SHIFT, 8000, 512, 60.0, F0_MAX, 1.0), (wav, 3, SHIFT, 8000, 768, F0_MIN, F0_MAX, 1.0),
                 (torch.zeros(400, requires_grad=True), 3) + geo + (1.0,), (np.zeros(400), 3) + geo + (1.0,)):
        with pytest.raises(ValueError):
            ops.f0_candidates(*args)
    z = lambda *shape, **kw: torch.zeros(*shape, **kw)
    n3 = torch.zeros(3, dtype=torch.int32)
    for args in ((z(3, 1), z(3, 1), n3), (z(3, 17), z(3, 17), n3), (z(3), z(3), n3), (z(3, 8), z(3, 7), n3), (z(3, 8), z(3, 8), n3[:2]),
                 (z(3, 8, requires_grad=True), z(3, 8), n3), (z(3, 8), z(3, 8, requires_grad=True), n3),
                 (z(MAX_FRAMES + 1, 8), z(MAX_FRAMES + 1, 8), torch.zeros(MAX_FRAMES + 1, dtype=torch.int32)),
                 (z(MAX_FRAMES // 2 + 1, 9), z(MAX_FRAMES // 2 + 1, 9), torch.zeros(MAX_FRAMES // 2 + 1, dtype=torch.int32))):
        with pytest.raises(ValueError):
            ops.f0_viterbi(*args, SHIFT)
    with pytest.raises(ValueError):
        ops.f0_viterbi(z(3, 8), z(3, 8), n3, 0.0)
    with pytest.raises(ValueError):
        ops.f0_viterbi(z(3, 8), z(3, 8), n3, SHIFT, octave_jump_cost=-1.0)
    long = np.zeros(rnd(MAX_FRAMES * SHIFT * 8000))             # MAX_FRAMES + 1 frames
    for args, kw in (((long,) + geo, {}), ((np.zeros(400), SHIFT, 8000, 512, 60.0, F0_MAX), {}), ((np.zeros((2, 200)),) + geo, {}),
                     ((np.full(400, np.nan),) + geo, {}), ((np.zeros(400),) + geo, dict(ncand=1)), ((np.zeros(400),) + geo, dict(cost=1.0)),
                     ((torch.zeros(400, requires_grad=True),) + geo, {})):
        with pytest.raises(ValueError):
            ops.f0_estimate(*args, **kw)
    # the f0 = None paths of the vocoder
    voc = vocoders.VocoderPML(8000, SHIFT, 9, 9, dftlen=512)
    with pytest.raises(ValueError, match='longest lag'):
        voc.analysis_device(np.zeros(400), None, 60.0, F0_MAX)
    with pytest.raises(ValueError, match='longest lag'):
        voc.f0_estimate_device(np.zeros(400), 60.0, F0_MAX)
    with pytest.raises(ValueError, match='at most {}'.format(MAX_FRAMES)):
        voc.analysis_device(long, None, F0_MIN, F0_MAX)
    with pytest.raises(ValueError):
        voc.analysis_device(np.zeros((2, 200)), None, F0_MIN, F0_MAX)


def test_interface(tmp_path, monkeypatch):
    import importlib
    from percivaltts_amd import ops, ops_offline, vocoders
    names = lambda f: list(inspect.signature(f).parameters)
    assert names(ops.f0_check) == ['dftlen', 'fs', 'shift', 'f0_min', 'f0_max']
    assert names(ops.f0_candidates) == ['wav', 'T', 'shift', 'fs', 'dftlen', 'f0_min', 'f0_max', 'gpeak', 'ncand', 'voicing_threshold',
                                        'silence_threshold', 'octave_cost', 'want_r']
    assert names(ops.f0_viterbi)[:6] == ['freq', 'strength', 'n', 'shift', 'octave_jump_cost', 'voiced_unvoiced_cost']
    assert names(ops.f0_estimate)[:6] == ['wav', 'shift', 'fs', 'dftlen', 'f0_min', 'f0_max']
    defaults = {k: v.default for k, v in inspect.signature(ops.f0_candidates).parameters.items()}
    assert defaults['ncand'] == NCAND and defaults['voicing_threshold'] == VOICING_THRESHOLD and defaults['want_r'] is False
    for name in ('f0_check', 'f0_window_table', 'f0_candidates', 'f0_viterbi', 'f0_estimate'):
        assert getattr(ops, name) is getattr(ops_offline, name) and name in ops_offline.__all__
    assert names(vocoders.VocoderF0Spec.f0_estimate_device) == ['self', 'wav', 'f0_min', 'f0_max']
    assert names(vocoders.VocoderPML.analysis_device) == ['self', 'wav', 'f0', 'f0_min', 'f0_max']
    assert names(vocoders.VocoderPML.analysisfid_device)[:7] == ['self', 'fid', 'wav_path', 'f0in_path', 'f0_min', 'f0_max', 'outputpathdicts']
    world = vocoders.VocoderWORLD(8000, SHIFT, 9, 4, dftlen=512)
    assert hasattr(world, 'f0_estimate_device') and not hasattr(world, 'analysis_device')
    monkeypatch.setenv('PERCIVAL_CORPUS', str(tmp_path / 'corpus'))
    monkeypatch.chdir(tmp_path)
    import percivaltts_amd.run as run
    run = importlib.reload(run)
    sig = inspect.signature(run.features_extraction)
    assert list(sig.parameters)[:3] == ['f0in_path', 'wav_path', 'rawpaths'] and sig.parameters['f0in_path'].default is None
    assert 'no F0 tracker' not in run.features_extraction.__doc__


# ---------------------------------------------------------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------------------------------------------------------
def _dev(a, dtype=torch.float32):
    return torch.tensor(np.asarray(a), dtype=dtype).cuda().contiguous()


_device_results = {}


def device_candidates(name, ncand=NCAND):
    """(freq, strength, n, lag, r) of the device on a test signal, as numpy; computed once."""
    if (name, ncand) not in _device_results:
        from percivaltts_amd import ops
        c = case(name)
        out = ops.f0_candidates(_dev(c['wav']), c['T'], SHIFT, c['fs'], c['L'], F0_MIN, F0_MAX, c['gpeak'], ncand=ncand, want_r=True)
        assert [t.dtype for t in out] == [torch.float32, torch.float32, torch.int32, torch.int32, torch.float32]
        lmax = geometry(c['fs'], F0_MIN, F0_MAX)[3]
        assert [tuple(t.shape) for t in out] == [(c['T'], ncand), (c['T'], ncand), (c['T'],), (c['T'], ncand), (c['T'], lmax + 2)]
        _device_results[(name, ncand)] = tuple(t.cpu().numpy() for t in out)
    return _device_results[(name, ncand)]


@pytest.mark.gpu
@pytest.mark.parametrize('name', ['A', 'B'])
def test_autocorrelation_against_restatement(name):
    c = case(name)
    r = device_candidates(name)[4]
    check(r, c['64']['r'], c['32']['r'], 'f0_candidates r ' + name)
    assert (r[:, 0] == (c['64']['lpeak'] > 0)).all()            # r[0] is 1 wherever the frame holds anything


@pytest.mark.gpu
@pytest.mark.parametrize('name', ['A', 'B'])
def test_candidates_against_restatement(name):
    from percivaltts_amd import ops
    c = case(name)
    freq, strength, n, lag, _ = device_candidates(name)
    np.testing.assert_array_equal(n, c['64']['n'])
    np.testing.assert_array_equal(lag, c['64']['lag'])
    check(freq, c['64']['freq'], c['32']['freq'], 'f0_candidates freq ' + name)
    check(strength, c['64']['strength'], c['32']['strength'], 'f0_candidates strength ' + name)
    again = ops.f0_candidates(_dev(c['wav']), c['T'], SHIFT, c['fs'], c['L'], F0_MIN, F0_MAX, c['gpeak'])
    assert len(again) == 4
    for got, first in zip(again, (freq, strength, n, lag)):     # same input, same bytes, with or without r
        np.testing.assert_array_equal(got.cpu().numpy(), first)


@pytest.mark.gpu
def test_candidates_truncated_to_three_slots():
    c = case('A')
    want = {tag: candidates_restated(c[tag]['r'], c[tag]['lpeak'], c['gpeak'], c['fs'], F0_MIN, F0_MAX, 3, dt)
            for tag, dt in (('64', np.float64), ('32', np.float32))}
    assert (c['64']['n'] > 2).any() and want['64'][2].max() == 2
    freq, strength, n, lag, _ = device_candidates('A', ncand=3)
    np.testing.assert_array_equal(n, want['64'][2])
    np.testing.assert_array_equal(lag, want['64'][3])
    np.testing.assert_array_equal(lag, c['64']['lag'][:, :3])   # the strongest two of the eight-slot table
    check(freq, want['64'][0], want['32'][0], 'f0_candidates freq A ncand=3')
    check(strength, want['64'][1], want['32'][1], 'f0_candidates strength A ncand=3')


@pytest.mark.gpu
@pytest.mark.parametrize('name', ['A', 'B'])
def test_silent_frames(name):
    c = case(name)
    freq, strength, n, lag, r = device_candidates(name)
    silent = c['64']['lpeak'] == 0
    assert silent.sum() >= 5 and (~silent).sum() >= 5
    assert (n[silent] == 0).all() and (r[silent] == 0).all() and (freq[silent] == 0).all() and (lag[silent] == 0).all()
    assert (strength[silent, 1:] == 0).all()
    assert ((strength[:, 0] == np.float32(VOICING_THRESHOLD + 2.0)) == silent).all()
    assert (strength[~silent, 0] < np.float32(VOICING_THRESHOLD + 2.0)).all() and (strength[:, 0] >= np.float32(VOICING_THRESHOLD)).all()


def _viterbi(freq, strength, n, **kw):
    from percivaltts_amd import ops
    f0, path = ops.f0_viterbi(_dev(freq), _dev(strength), _dev(n, torch.int32), SHIFT, want_path=True, **kw)
    assert f0.dtype == torch.float32 and path.dtype == torch.int32 and tuple(f0.shape) == tuple(path.shape) == (len(n),)
    return f0.cpu().numpy(), path.cpu().numpy()


@pytest.mark.gpu
@pytest.mark.parametrize('name', ['A', 'B'])
def test_viterbi_on_the_restated_tables(name):
    c = case(name)
    freq, strength = c['64']['freq'].astype(np.float32), c['64']['strength'].astype(np.float32)
    f0, path = _viterbi(freq, strength, c['64']['n'])
    np.testing.assert_array_equal(path, c['64']['path'])
    np.testing.assert_array_equal(f0, freq[np.arange(c['T']), c['64']['path']])
    assert ((f0 > 0) == (path > 0)).all()


@pytest.mark.gpu
@pytest.mark.parametrize('ncand', [8, 16, 2, 5, 11])
def test_viterbi_on_a_random_table(ncand):
    """Near-ties are possible here, so the criterion is the cost: the device path, re-evaluated in float64, costs within
    1e-9 |optimum| of the optimum (float64 rounding of about 4 T operations) and uses only valid slots."""
    T = 257
    freq, strength, n = random_table(T, ncand, 100 + ncand)
    _, _, best = viterbi_restated(freq, strength, n, SHIFT, np.float64)
    f0, path = _viterbi(freq, strength, n)
    cost = path_cost(path, freq, strength, n, SHIFT)
    assert cost is not None, 'the path uses a slot behind a frame\'s count'
    print('ncand={}: device path costs {:.12f}, the optimum {:.12f}'.format(ncand, cost, best))
    assert abs(cost - best) <= 1e-9 * abs(best)
    np.testing.assert_array_equal(f0, freq[np.arange(T), path])
    other = _viterbi(freq, strength, n, octave_jump_cost=0.0, voiced_unvoiced_cost=0.0)[1]      # free transitions: every frame's best
    np.testing.assert_array_equal(other, [int(np.argmax(strength[i, :n[i] + 1])) for i in range(T)])


@pytest.mark.gpu
@pytest.mark.parametrize('what', ['T1', 'T2', 'short'])
def test_edge_lengths(what):
    from percivaltts_amd import ops
    c = case('A')
    wav = c['wav'][:60] if what == 'short' else c['wav']        # 60 samples: a quarter of the 241 of the window
    T = {'T1': 1, 'T2': 2, 'short': ops.f0_frame_count(60, SHIFT, c['fs'])}[what]
    assert T == (2 if what != 'T1' else 1)
    want = {tag: estimate_restated(wav, T, SHIFT, c['fs'], c['L'], F0_MIN, F0_MAX, NCAND, dt) for tag, dt in (('64', np.float64), ('32', np.float32))}
    out = ops.f0_candidates(_dev(wav), T, SHIFT, c['fs'], c['L'], F0_MIN, F0_MAX, global_peak(wav), want_r=True)
    freq, strength, n, lag, r = (t.cpu().numpy() for t in out)
    check(r, want['64']['r'], want['32']['r'], 'f0_candidates r A ' + what)
    np.testing.assert_array_equal(n, want['64']['n'])
    np.testing.assert_array_equal(lag, want['64']['lag'])
    check(freq, want['64']['freq'], want['32']['freq'], 'f0_candidates freq A ' + what)
    check(strength, want['64']['strength'], want['32']['strength'], 'f0_candidates strength A ' + what)
    f0, path = _viterbi(want['64']['freq'].astype(np.float32), want['64']['strength'].astype(np.float32), n)
    np.testing.assert_array_equal(path, want['64']['path'])
    np.testing.assert_array_equal(f0, want['64']['freq'].astype(np.float32)[np.arange(T), path])
    if what == 'short':                                         # the whole chain on a waveform of two frames
        got = ops.f0_estimate(wav, SHIFT, c['fs'], c['L'], F0_MIN, F0_MAX)
        assert got.shape == (T,) and ((got > 0) == (want['64']['path'] > 0)).all()


@pytest.mark.gpu
def test_no_frames_no_launch():
    from percivaltts_amd import _hip, ops
    with _hip.KernelTimer() as kt:
        out = ops.f0_candidates(_dev(np.zeros(10)), 0, SHIFT, 8000, 512, F0_MIN, F0_MAX, 0.0, want_r=True)
        f0, path = ops.f0_viterbi(out[0], out[1], out[2], SHIFT, want_path=True)
    assert kt.records == []
    assert [tuple(t.shape) for t in out] == [(0, 8), (0, 8), (0,), (0, 8), (0, 82)] and tuple(f0.shape) == tuple(path.shape) == (0,)
    l = _hip.lib()
    geo = (SHIFT, 8000.0, 512, F0_MIN, F0_MAX, 0.0, VOICING_THRESHOLD, SILENCE_THRESHOLD, OCTAVE_COST, None)
    assert l.ptts_f0_candidates(None, 0, None, 0, None, None, None, None, None, 0, 8, *geo) == 0
    assert l.ptts_f0_candidates(None, 0, None, 0, None, None, None, None, None, 0, 17, *geo) != 0
    assert l.ptts_f0_candidates(None, 0, None, 0, None, None, None, None, None, 1, 8, SHIFT, 8000.0, 768, *geo[3:]) != 0
    assert l.ptts_f0_candidates(None, 0, None, 0, None, None, None, None, None, 0, 8, SHIFT, 8000.0, 512, 60.0, *geo[4:]) != 0
    assert l.ptts_f0_viterbi(None, None, None, None, None, 0, 8, SHIFT, OCTAVE_JUMP_COST, VOICED_UNVOICED_COST, None) == 0
    assert l.ptts_f0_viterbi(None, None, None, None, None, MAX_FRAMES + 1, 8, SHIFT, OCTAVE_JUMP_COST, VOICED_UNVOICED_COST, None) != 0
    assert l.ptts_f0_viterbi(None, None, None, None, None, MAX_FRAMES // 2 + 1, 9, SHIFT, OCTAVE_JUMP_COST, VOICED_UNVOICED_COST, None) != 0
    assert l.ptts_f0_viterbi(None, None, None, None, None, 0, 1, SHIFT, OCTAVE_JUMP_COST, VOICED_UNVOICED_COST, None) != 0
    assert (l.ptts_f0_viterbi_max_frames(8), l.ptts_f0_viterbi_max_frames(9), l.ptts_f0_viterbi_max_frames(17)) == (MAX_FRAMES, MAX_FRAMES // 2, 0)
    with pytest.raises(_hip.HipLibraryError):
        ops.f0_candidates(torch.zeros(400), 3, SHIFT, 8000, 512, F0_MIN, F0_MAX, 1.0)


@pytest.mark.gpu
def test_estimate_and_analysis_end_to_end():
    from percivaltts_amd import ops, vocoders
    c = case('A')
    f0 = ops.f0_estimate(c['wav'], SHIFT, c['fs'], c['L'], F0_MIN, F0_MAX)
    assert isinstance(f0, np.ndarray) and f0.dtype == np.float32 and f0.shape == (c['T'],)
    np.testing.assert_array_equal(f0 > 0, c['64']['path'] > 0)
    sel = np.arange(c['T'])
    check(f0, c['64']['freq'][sel, c['64']['path']], c['32']['freq'][sel, c['32']['path']], 'f0_estimate A')
    voc = vocoders.VocoderPML(c['fs'], SHIFT, 9, 9, dftlen=c['L'])
    np.testing.assert_array_equal(voc.f0_estimate_device(c['wav'], F0_MIN, F0_MAX), f0)
    np.testing.assert_array_equal(ops.f0_estimate(_dev(c['wav']), SHIFT, c['fs'], c['L'], F0_MIN, F0_MAX), f0)
    own = voc.analysis_device(c['wav'], None, F0_MIN, F0_MAX)
    given = voc.analysis_device(c['wav'], f0, F0_MIN, F0_MAX)
    assert own.shape == (c['T'], voc.featuressizeraw()) and own.dtype == np.float32 and np.isfinite(own).all()
    np.testing.assert_array_equal(own, given)
    # an explicit track goes the way it went: ops.f0_track, then the chain of the public ops
    track = ops.f0_track(f0, F0_MIN, F0_MAX, c['fs'], SHIFT, c['L'])
    np.testing.assert_array_equal(given[:, 0], np.log(track.astype(np.float64)).astype(np.float32))
    hcap = ops.analysis_check(c['L'], c['fs'], SHIFT, F0_MIN, F0_MAX)
    lspec, _ = ops.frame_harmonics(_dev(c['wav']), _dev(track), SHIFT, c['fs'], c['L'], hcap, log=True)
    np.testing.assert_array_equal(given[:, 1:10], ops.fwbnd_compress(lspec, c['fs'], 9, log=True).cpu().numpy())
    other = voc.analysis_device(c['wav'], c['f0'], F0_MIN, F0_MAX)
    np.testing.assert_array_equal(other[:, 0], np.log(c['f0'].astype(np.float64)).astype(np.float32))


@pytest.mark.gpu
def test_features_extraction_estimates_the_track(tmp_path, monkeypatch):
    """Two utterances from .wav alone to the raw streams and the composed outputs."""
    import importlib
    from percivaltts_amd import vocoders
    monkeypatch.setenv('PERCIVAL_CORPUS', str(tmp_path / 'corpus'))
    monkeypatch.chdir(tmp_path)
    import percivaltts_amd.run as run
    run = importlib.reload(run)
    run.cfg.id_valid_start = 1
    fs, voc = run.cfg.vocoder_fs, run.vocoder
    fids, lens, truth = ['utt_a', 'utt_b'], [44, 36], {}
    os.makedirs(str(tmp_path / 'corpus' / 'wav'))
    rng = np.random.RandomState(12)
    for fid, T in zip(fids, lens):
        N = int(round(SHIFT * (T - 1) * fs))
        f0 = 150.0 + 40.0 * np.sin(np.arange(T) / 5.0 + rng.rand())
        phase = 2 * np.pi * np.cumsum(np.interp(np.arange(N) / float(fs), SHIFT * np.arange(T), f0)) / fs
        wav = 0.1 * sum(np.cos(h * phase) / h for h in range(1, 20)) + 0.01 * rng.randn(N)
        vocoders.wavwrite(str(tmp_path / 'corpus' / 'wav' / (fid + '.wav')), wav, fs)
        truth[fid] = f0
    with open(run.cfg.fileids, 'w') as f:
        f.write('\n'.join(fids) + '\n')
    run.features_extraction(None)
    nout = voc.featuressize()
    for fid, T in zip(fids, lens):
        cmp = np.fromfile(run.cfg.outpath.split(':')[0].replace('*', fid), dtype=np.float32)
        assert cmp.shape == (T * nout,) and np.isfinite(cmp).all()
        lf0 = np.fromfile(str(tmp_path / 'corpus' / ('wav_PML_lf0/' + fid + '.lf0')), dtype=np.float32)
        assert lf0.shape == (T,)
        rel = np.abs(np.exp(lf0[4:-4].astype(np.float64)) / truth[fid][4:-4] - 1.0)
        print('{}: relative F0 error mean {:.4f}, largest {:.4f}'.format(fid, rel.mean(), rel.max()))
        assert rel.max() <= GROSS
        raw = voc.f0_estimate_device(vocoders.wavread(str(tmp_path / 'corpus' / 'wav' / (fid + '.wav')))[0], 70, 600)
        assert (raw[4:-4] > 0).all()                            # voiced throughout: the written values are estimates, not fill-ins
