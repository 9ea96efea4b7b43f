"""Waveform pre-processing (csrc/preproc.hip; ops.preproc_check / resample_table / resample / highpass_tile / highpass_zerophase,
Vocoder.preprocwav, run.features_extraction(..., preproc_hp=)).

Both definitions are the build's own and are restated here as plain loops in a chosen dtype.  The reference's
resampler (pulsemodel's) is absent from its checkout, so there is nothing of it to compare with; the resampler's definition is
checked by its properties (a sine comes through, a sine above the new Nyquist frequency does not).  The high-pass filter is
mathematically scipy.signal.sosfiltfilt(butter(4, fc / (fs / 2), 'high', output='sos'), x, padtype='odd', padlen=P): the float64
restatement is held against it to 1e-10 absolute on signals of peak 0.5.

Bound of the device results, both kernels: |got - want64| <= ulp32(max |want64|), absolute, want64 being the float64 restatement on
the same float32 input.  Half of it is the one rounding to float32; the other half is room for float64 reassociation (the blocked
recurrence of the kernel against the sequential loop: test_blocked_recurrence_stays_with_the_sequential_one holds that below 1e-2 ulp
at the lowest cut-off the entry point takes; the resampler sums in the restatement's order)."""
import ctypes
import inspect
import math
import os

import numpy as np
import pytest
import torch

from percivaltts_amd import _hip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PADLEN = 15
EINVAL = -1
RATE_PAIRS = [(48000, 16000), (44100, 16000), (22050, 16000), (8000, 16000), (16000, 44100)]
HP_CASES = [(8000, 300.0), (16000, 70.0), (48000, 50.0)]
SHIFT = 0.005
F0_MIN, F0_MAX = 100.0, 400.0


# ---------------------------------------------------------------------------------------------------------------------------
# the definitions, restated
# ---------------------------------------------------------------------------------------------------------------------------
def ratio(fs_in, fs_out):
    """(up, down, c, R, hw)"""
    g = math.gcd(fs_in, fs_out)
    up, down = fs_out // g, fs_in // g
    c = 0.95 * min(1.0, up / float(down))
    R = 16.0 / c
    return up, down, c, R, int(math.ceil(R))


def table_restated(fs_in, fs_out):
    """h[p][j + hw - 1], p = 0 .. up - 1, j = -hw + 1 .. hw, float64."""
    up, down, c, R, hw = ratio(fs_in, fs_out)
    h = np.zeros((up, 2 * hw))
    for p in range(up):
        for j in range(-hw + 1, hw + 1):
            tau = p / float(up) - j
            if abs(tau) < R:
                x = c * tau
                sinc = 1.0 if x == 0.0 else math.sin(math.pi * x) / (math.pi * x)
                h[p, j + hw - 1] = c * sinc * float(np.i0(9.0 * math.sqrt(1.0 - (tau / R) ** 2))) / float(np.i0(9.0))
    return h


_tables = {}


def table(fs_in, fs_out):
    if (fs_in, fs_out) not in _tables:
        _tables[(fs_in, fs_out)] = table_restated(fs_in, fs_out)
    return _tables[(fs_in, fs_out)]


def resample_restated(x, fs_in, fs_out, dtype=np.float64):
    """y[m] = sum_j h[p][j] x[q + j] in increasing j, one output sample after the other (all of them at once per tap: the order
    of the additions of a sample is the loop's)."""
    up, down, _, _, hw = ratio(fs_in, fs_out)
    x = np.asarray(x, dtype=dtype)
    N = len(x)
    M = (N * up + down - 1) // down
    h = table(fs_in, fs_out).astype(dtype)
    xp = np.concatenate([np.zeros(hw, dtype=dtype), x, np.zeros(hw + 1, dtype=dtype)])       # xp[i + hw] = x[i]
    m = np.arange(M, dtype=np.int64)
    q, p = (m * down) // up, (m * down) % up
    acc = np.zeros(M, dtype=dtype)
    for j in range(-hw + 1, hw + 1):
        acc = acc + h[p, j + hw - 1] * xp[q + j + hw]
    return acc


def sections_restated(fs, fc):
    """[(b0, b1, b2, a1, a2)] of the two sections."""
    K = math.tan(math.pi * fc / fs)
    out = []
    for Q in (1.0 / (2.0 * math.cos(math.pi / 8.0)), 1.0 / (2.0 * math.cos(3.0 * math.pi / 8.0))):
        n = 1.0 / (1.0 + K / Q + K * K)
        out.append((n, -2.0 * n, n, 2.0 * (K * K - 1.0) * n, (1.0 - K / Q + K * K) * n))
    return out


def extend_restated(x, P):
    x = list(x)
    N = len(x)
    assert N > P
    return [2 * x[0] - x[P - k] for k in range(P)] + x + [2 * x[N - 1] - x[N - 2 - i] for i in range(P)]


def section_restated(x, coef, x_start, dt):
    b0, b1, b2, a1, a2 = (dt(v) for v in coef)
    x1 = x2 = dt(x_start)
    y1 = y2 = dt(0)
    out = []
    for v in x:
        y = ((b0 * v + b1 * x1) + b2 * x2) - a1 * y1 - a2 * y2
        out.append(y)
        x2, x1, y2, y1 = x1, v, y1, y
    return out


def pass_restated(e, coefs, dt):
    return section_restated(section_restated(e, coefs[0], e[0], dt), coefs[1], 0, dt)


def highpass_restated(x, fs, fc, P=PADLEN, dtype=np.float64):
    """The definition as plain loops; float64 runs on Python floats (the same IEEE doubles), any other dtype on numpy scalars."""
    dt = float if np.dtype(dtype) == np.float64 else np.dtype(dtype).type
    e = extend_restated([dt(v) for v in np.asarray(x, dtype=dtype)], P)
    coefs = sections_restated(fs, fc)
    r = pass_restated(pass_restated(e, coefs, dt)[::-1], coefs, dt)[::-1]
    return np.array(r[P:len(r) - P], dtype=dtype)


def section_blocked(x, coef, c, x_start, chunk, lanes):
    """The kernel's form of a section in float64: tiles of `lanes` chunks, every chunk run from a zero state (the first from the
    state carried into the tile), the end states scanned as (y[n-1], y[n-1] - y[n-2]) with the powers, by squaring, of the transition
    matrix in that basis, [[1 - c, a2], [-c, a2]] with c = 1 + a1 + a2 = 4 K^2 n = 4 K^2 b0, every chunk run again from its start."""
    b0, b1, b2, a1, a2 = coef
    n = len(x)
    tile = chunk * lanes
    ntiles = (n + tile - 1) // tile
    xp = np.zeros(ntiles * tile)
    xp[:n] = x
    v = b0 * xp + b1 * np.concatenate([[x_start], xp[:-1]]) + b2 * np.concatenate([[x_start, x_start], xp[:-2]])
    P = np.array([[1.0 - c, a2], [-c, a2]])
    s = 1
    while s < chunk:
        P, s = P @ P, 2 * s
    levels, o = [], 1
    while o < lanes:
        levels.append(P)
        P, o = P @ P, 2 * o

    def run(vt, y1, y2, keep):
        out = np.zeros_like(vt)
        for i in range(chunk):
            y = (vt[:, i] - a1 * y1) - a2 * y2
            if keep:
                out[:, i] = y
            y2, y1 = y1, y
        return out, y1, y2

    y = np.zeros_like(xp)
    carry = np.zeros(2)                                         # (y[-1], y[-1] - y[-2])
    for t in range(ntiles):
        vt = v[t * tile:(t + 1) * tile].reshape(lanes, chunk)
        y1, y2 = np.zeros(lanes), np.zeros(lanes)
        y1[0], y2[0] = carry[0], carry[0] - carry[1]
        _, e1, e2 = run(vt, y1, y2, False)
        E = np.stack([e1, e1 - e2], axis=1)
        for d, Pd in enumerate(levels):
            o = 1 << d
            E = np.concatenate([E[:o], E[:-o] @ Pd.T + E[o:]])
        start = np.concatenate([[carry], E[:-1]])
        out, _, _ = run(vt, start[:, 0].copy(), start[:, 0] - start[:, 1], True)
        y[t * tile:(t + 1) * tile] = out.reshape(-1)
        carry = E[-1]
    return y[:n]


def highpass_blocked(x, fs, fc, P, chunk, lanes):
    e = np.array(extend_restated([float(v) for v in x], P))
    coefs = sections_restated(fs, fc)
    c = [4.0 * math.tan(math.pi * fc / fs) ** 2 * k[0] for k in coefs]

    def one(e):
        return section_blocked(section_blocked(e, coefs[0], c[0], e[0], chunk, lanes), coefs[1], c[1], 0.0, chunk, lanes)
    r = one(one(e)[::-1])[::-1]
    return r[P:len(r) - P]


def signal(kind, N, fs, seed=0):
    """float32 test signals of peak about 0.5: a sine with an offset of 0.2 and noise, a unit step, zeros."""
    n = np.arange(N)
    if kind == 'sine':
        rng = np.random.RandomState(seed + N)
        return (0.25 * np.sin(2 * np.pi * 440.0 * n / fs + 0.3) + 0.2 + 0.02 * rng.randn(N)).astype(np.float32)
    if kind == 'step':
        return (n >= N // 3).astype(np.float32)
    return np.zeros(N, dtype=np.float32)


def ulp32(v):
    return float(np.spacing(np.float32(v)))


def within_one_ulp(got, want64, what):
    """|got - want64| <= ulp32(max |want64|); returns the worst error in such ulps."""
    got, want64 = np.asarray(got), np.asarray(want64, dtype=np.float64)
    assert got.dtype == np.float32 and got.shape == want64.shape, (what, got.dtype, got.shape, want64.shape)
    if want64.size == 0:
        return 0.0
    bound = ulp32(np.abs(want64).max())
    err = float(np.abs(got.astype(np.float64) - want64).max())
    assert np.isfinite(got).all() and err <= bound, '{}: error {:.3e} above {:.3e}'.format(what, err, bound)
    return err / bound


# ---------------------------------------------------------------------------------------------------------------------------
# CPU
# ---------------------------------------------------------------------------------------------------------------------------
def tile_geometry():
    chunk, tile = ctypes.c_int(0), ctypes.c_int(0)
    assert _hip.lib().ptts_highpass_tile(ctypes.byref(chunk), ctypes.byref(tile)) == 0
    return chunk.value, tile.value


def test_header_declares_and_library_exports_the_symbols():
    with open(os.path.join(ROOT, 'include', 'percival_hip.h')) as f:
        header = f.read()
    names = ['ptts_resample', 'ptts_highpass_zerophase', 'ptts_highpass_workspace_bytes', 'ptts_highpass_tile', 'ptts_highpass_sections']
    assert 'int ptts_highpass_tile(int* chunk, int* tile);' in header
    assert 'size_t ptts_highpass_workspace_bytes(long long total, int n_utts, int padlen);' in header
    for n in names:
        assert n in header and n in _hip.SIGNATURES, n
    assert os.path.exists(_hip.LIB_PATH), 'libpercival_hip.so not built (run __graft_entry__.build())'
    lib = ctypes.CDLL(_hip.LIB_PATH)
    for n in names:
        assert hasattr(lib, n), n
    for doc in ('INTEGRATION.md', 'DESIGN.md', 'README.md'):
        with open(os.path.join(ROOT, doc)) as f:
            text = f.read()
        assert 'ptts_resample' in text and 'ptts_highpass_zerophase' in text, doc
    with open(os.path.join(ROOT, 'percivaltts_amd', 'csrc', 'Makefile')) as f:
        assert 'preproc.hip' in f.read()
    chunk, tile = tile_geometry()
    assert chunk >= 2 and tile % chunk == 0 and tile // chunk >= 64


@pytest.mark.parametrize('fs,fc,N', [(8000, 300.0, 16), (8000, 70.0, 257), (16000, 70.0, 20000), (48000, 50.0, 30000)])
def test_highpass_restatement_is_sosfiltfilt(fs, fc, N):
    from scipy import signal as sig
    x = signal('sine', N, fs).astype(np.float64)
    sos = sig.butter(4, fc / (fs / 2.0), 'high', output='sos')
    want = sig.sosfiltfilt(sos, x, padtype='odd', padlen=PADLEN)
    got = highpass_restated(x, fs, fc)
    err = float(np.abs(got - want).max())
    print('fs {} fc {} N {}: restatement against sosfiltfilt {:.2e}'.format(fs, fc, N, err))
    assert err <= 1e-10


@pytest.mark.parametrize('fs,fc', HP_CASES + [(16000, 4.0), (44100, 11025.0), (32000, 15999.0)])
def test_closed_form_sections_are_butterworth(fs, fc):
    """The restatement's and the library's coefficients against scipy.signal.butter's sections, 1e-12: scipy keeps the whole gain
    in its first section, so the denominators are compared section by section and the gain as the product."""
    from scipy import signal as sig
    sos = sig.butter(4, fc / (fs / 2.0), 'high', output='sos')
    mine = sections_restated(fs, fc)
    lib_sos = (ctypes.c_double * 12)()
    assert _hip.lib().ptts_highpass_sections(float(fs), float(fc), lib_sos) == 0
    lib_sos = np.array(lib_sos).reshape(2, 6)
    np.testing.assert_allclose(lib_sos[:, [0, 1, 2, 4, 5]], np.array(mine), rtol=0, atol=1e-15)
    assert (lib_sos[:, 3] == 1.0).all()
    theirs = sorted(sos.tolist(), key=lambda r: r[5])
    for (b0, b1, b2, a1, a2), row in zip(sorted(mine, key=lambda r: r[4]), theirs):
        assert abs(a1 - row[4]) <= 1e-12 and abs(a2 - row[5]) <= 1e-12 and row[3] == 1.0
        assert b1 == -2.0 * b0 and b2 == b0
        assert abs(row[1] / row[0] + 2.0) <= 1e-12 and abs(row[2] / row[0] - 1.0) <= 1e-12
    assert abs(mine[0][0] * mine[1][0] - sos[0, 0] * sos[1, 0]) <= 1e-12


@pytest.mark.parametrize('fs,fc', [(48000, 50.0), (16000, 17.5), (16000, 4.0), (48000, 12.0)])
def test_blocked_recurrence_stays_with_the_sequential_one(fs, fc):
    """The kernel's blocked form, restated in float64 with the kernel's chunk and tile, against the sequential loop: below 1e-2
    ulp32 of the peak, also at the lowest cut-off the entry point takes, fc = fs / 4000."""
    chunk, tile = tile_geometry()
    N = 2 * tile + 1000
    x = signal('sine', N, fs, seed=5)
    want = highpass_restated(x, fs, fc)
    got = highpass_blocked(x, fs, fc, PADLEN, chunk, tile // chunk)
    err = float(np.abs(got - want).max())
    print('fs {} fc {}: blocked against sequential {:.2e} = {:.2e} ulp32'.format(fs, fc, err, err / ulp32(np.abs(want).max())))
    assert err <= 1e-2 * ulp32(np.abs(want).max())


def test_a_constant_leaves_nothing():
    """The steady-state start: a constant input gives exactly 0, in both dtypes."""
    for dtype in (np.float64, np.float32):
        y = highpass_restated(np.full(40, 0.3, dtype=dtype), 8000, 300.0, dtype=dtype)
        assert y.dtype == dtype and (y == 0).all()


def middle(y):
    return y[len(y) // 4:len(y) - len(y) // 4]


@pytest.mark.parametrize('fs_in,fs_out', RATE_PAIRS)
def test_resampler_definition_properties(fs_in, fs_out):
    """On 0.2 s sines, the middle half of the output: a 1 kHz sine comes through with an error below -90 dB, and when the rate
    goes down a sine at 0.6 fs_out comes out below -80 dB."""
    N = int(0.2 * fs_in)
    t_in = np.arange(N) / float(fs_in)
    y = resample_restated(np.sin(2 * np.pi * 1000.0 * t_in), fs_in, fs_out)
    t_out = np.arange(len(y)) / float(fs_out)
    err = 20 * np.log10(np.abs(middle(y - np.sin(2 * np.pi * 1000.0 * t_out))).max())
    print('{} -> {}: 1 kHz sine error {:.1f} dB'.format(fs_in, fs_out, err))
    assert err < -90.0
    if fs_out < fs_in:
        alias = 20 * np.log10(np.abs(middle(resample_restated(np.sin(2 * np.pi * 0.6 * fs_out * t_in), fs_in, fs_out))).max())
        print('{} -> {}: a sine at 0.6 fs_out comes out at {:.1f} dB'.format(fs_in, fs_out, alias))
        assert alias < -80.0
    up, down, _, _, hw = ratio(fs_in, fs_out)
    for n in (1, 2, down, down + 1):
        assert len(resample_restated(np.ones(n), fs_in, fs_out)) == int(math.ceil(n * up / float(down)))
    assert (resample_restated(np.zeros(50), fs_in, fs_out) == 0).all()
    from percivaltts_amd import ops
    assert ops.preproc_check(fs_in, fs_out) == (up, down, hw)
    np.testing.assert_allclose(ops.resample_table(fs_in, fs_out), table(fs_in, fs_out), rtol=0, atol=1e-15)


def test_table_sizes_named_in_the_definition():
    assert ratio(44100, 16000)[0] == 160 and 2 * ratio(44100, 16000)[4] == 94
    assert ratio(16000, 44100)[0] == 441 and 2 * ratio(16000, 44100)[4] == 34


def test_argument_checks_without_a_device(monkeypatch):
    from percivaltts_amd import ops, vocoders
    monkeypatch.setattr(torch.cuda, 'is_available', lambda: False)
    x = torch.zeros(100)
    for fs_in, fs_out in ((16000.5, 8000), (0, 8000), (-16000, 8000), (16000, 0), ('16000', 8000), (16000, None), (16000, 16411)):
        with pytest.raises(ValueError):
            ops.resample(x, fs_in, fs_out)
        with pytest.raises(ValueError):
            ops.preproc_check(fs_in, fs_out)
    assert 16411 // math.gcd(16000, 16411) > 1024
    for fc in (0.0, 1.9, 4000.0, 5000.0, -70.0, float('nan')):
        with pytest.raises(ValueError):
            ops.highpass_zerophase(x, 8000, fc)
    for padlen in (-1, 1.5, 100, 1 << 21):
        with pytest.raises(ValueError):
            ops.highpass_zerophase(x, 8000, 70.0, padlen=padlen)
    with pytest.raises(ValueError):
        ops.highpass_zerophase(torch.zeros(PADLEN), 8000, 70.0)
    with pytest.raises(ValueError):
        ops.highpass_zerophase([torch.zeros(100), torch.zeros(PADLEN)], 8000, 70.0)
    for bad in (torch.zeros(2, 50), [torch.zeros(2, 50)], np.zeros(100), None):
        with pytest.raises(ValueError):
            ops.resample(bad, 16000, 8000)
        with pytest.raises(ValueError):
            ops.highpass_zerophase(bad, 8000, 70.0)
    with pytest.raises(_hip.HipLibraryError):                   # a host tensor: there is no CPU path
        ops.resample(x, 16000, 8000)
    with pytest.raises(_hip.HipLibraryError):
        ops.highpass_zerophase(x, 8000, 70.0)
    assert ops.resample(x, 8000, 8000) is x                     # the identity makes no launch: a host tensor passes

    voc = vocoders.VocoderPML(8000, SHIFT, 9, 9, dftlen=512)
    for wav, fs, hp in ((np.zeros((2, 50)), 8000, None), (np.array([0.0, np.nan, 0.0]), 8000, None), (np.zeros(PADLEN), 8000, 70.0),
                        (np.zeros(2 * PADLEN), 16000, 70.0), (np.zeros(100), 16000.5, None), (np.zeros(100), 8000, 4000.0),
                        (np.zeros(100), 8000, 1.0), (torch.zeros(2, 50), 8000, None)):
        with pytest.raises(ValueError):
            voc.preprocwav(wav, fs, hp)


def test_entry_points_reject_bad_arguments():
    """PTTS_EINVAL before any launch, the message naming the entry point; no pointer is dereferenced."""
    lib = _hip.lib()
    p = ctypes.c_void_p(256)            # non-null, never read
    big = 1 << 30

    def hp(x=p, y=p, off=p, total=1000, n=2, fs=8000.0, fc=70.0, P=15, ws=p, nws=big):
        return lib.ptts_highpass_zerophase(x, y, off, total, n, fs, fc, P, ws, nws, None)
    need = lib.ptts_highpass_workspace_bytes(1000, 2, 15)
    assert need == 8 * (1000 + 2 * 15 * 2)
    for kw in (dict(x=None), dict(y=None), dict(off=None), dict(ws=None), dict(n=-1), dict(n=65536), dict(total=-1), dict(P=-1),
               dict(P=(1 << 20) + 1), dict(fc=1.9), dict(fc=4000.0), dict(fs=0.0), dict(fs=float('nan')), dict(nws=need - 1),
               dict(ws=ctypes.c_void_p(260))):
        assert hp(**kw) == EINVAL, kw
        assert 'highpass_zerophase' in _hip.last_error()
    assert hp(n=0) == 0 and hp(total=0, x=None, y=None, ws=None, nws=0) == 0
    assert lib.ptts_highpass_workspace_bytes(-1, 2, 15) == 0 and lib.ptts_highpass_workspace_bytes(10, -2, 15) == 0
    assert lib.ptts_highpass_workspace_bytes(10, 1, -1) == 0
    assert lib.ptts_highpass_tile(None, None) == EINVAL
    assert lib.ptts_highpass_sections(8000.0, 5000.0, (ctypes.c_double * 12)()) == EINVAL
    assert lib.ptts_highpass_sections(8000.0, 70.0, None) == EINVAL

    def rs(x=p, xoff=p, tin=1000, y=p, yoff=p, tout=500, mout=300, n=2, h=p, hb=big, up=1, down=2, hw=34):
        return lib.ptts_resample(x, xoff, tin, y, yoff, tout, mout, n, h, hb, up, down, hw, None)
    for kw in (dict(x=None), dict(xoff=None), dict(y=None), dict(yoff=None), dict(h=None), dict(n=-1), dict(n=65536), dict(up=0),
               dict(up=1025), dict(down=0), dict(hw=0), dict(up=1024, hw=300), dict(tin=-1), dict(tout=-1), dict(mout=-1), dict(mout=501),
               dict(hb=8 * 68 - 1), dict(h=ctypes.c_void_p(260))):
        assert rs(**kw) == EINVAL, kw
        assert 'resample' in _hip.last_error()
    assert rs(n=0) == 0 and rs(mout=0) == 0


def test_interface(tmp_path, monkeypatch):
    import importlib
    from percivaltts_amd import ops, ops_offline, vocoders
    names = lambda f: list(inspect.signature(f).parameters)
    assert str(inspect.signature(vocoders.Vocoder.preprocwav)) == '(self, wav, fs, highpass=None)'
    assert 'Hz' in vocoders.Vocoder.preprocwav.__doc__ and 'highpass / 4' in vocoders.Vocoder.preprocwav.__doc__
    assert names(ops.resample) == ['wav', 'fs_in', 'fs_out']
    assert str(inspect.signature(ops.highpass_zerophase)) == '(wav, fs, fc, padlen=15)'
    for name in ('preproc_check', 'resample_table', 'resample', 'highpass_tile', 'highpass_zerophase'):
        assert getattr(ops, name) is getattr(ops_offline, name) and name in ops_offline.__all__
    assert 'preprocwav' in vocoders.VocoderPML.analysisf_device.__doc__
    world = vocoders.VocoderWORLD(8000, SHIFT, 9, 4, dftlen=512)
    assert hasattr(world, 'preprocwav') and not hasattr(world, 'analysis_device') and not hasattr(world, 'synthesis_device')
    monkeypatch.setenv('PERCIVAL_CORPUS', str(tmp_path / 'corpus'))
    monkeypatch.chdir(tmp_path)
    import percivaltts_amd.run as run
    run = importlib.reload(run)
    params = list(inspect.signature(run.features_extraction).parameters.values())
    assert params[-1].name == 'preproc_hp' and params[-1].default is None


# ---------------------------------------------------------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------------------------------------------------------
def _dev(a, dtype=torch.float32):
    return torch.tensor(np.asarray(a), dtype=dtype).cuda().contiguous()


def hp_lengths(padlen=PADLEN):
    chunk, tile = tile_geometry()
    return [padlen + 1, chunk - 1, chunk, chunk + 1, tile - padlen - 1, tile - padlen, tile - padlen + 1, 2 * tile + 17]


@pytest.mark.gpu
@pytest.mark.parametrize('fs,fc', HP_CASES)
def test_highpass_against_restatement(fs, fc):
    """The end of the extended signal before, on and behind a lane's and a tile's edge; a sine with an offset and noise, a unit step
    (the steady-state start: the output tends to 0), and zeros."""
    from percivaltts_amd import ops
    worst = 0.0
    for N in hp_lengths():
        if N <= PADLEN:
            continue
        for kind in ('sine', 'step', 'zeros'):
            x = signal(kind, N, fs)
            got = ops.highpass_zerophase(_dev(x), fs, fc).cpu().numpy()
            want = highpass_restated(x, fs, fc)
            worst = max(worst, within_one_ulp(got, want, 'highpass {} {} N={} {}'.format(fs, fc, N, kind)))
            if kind == 'zeros':
                assert (got == 0).all()
            if kind == 'step' and N > 8 * fs / fc:
                assert np.abs(got[-int(fs / fc):-int(0.5 * fs / fc)]).max() < 0.05 * np.abs(got).max()
    print('highpass fs {} fc {}: worst error {:.3f} ulp32 of the peak'.format(fs, fc, worst))


@pytest.mark.gpu
@pytest.mark.parametrize('padlen', [1, 15, 40])
def test_highpass_padlen(padlen):
    from percivaltts_amd import ops
    chunk, tile = tile_geometry()
    fs, fc, N = 16000, 70.0, tile - padlen + 1
    x = signal('sine', N, fs, seed=padlen)
    got = ops.highpass_zerophase(_dev(x), fs, fc, padlen=padlen).cpu().numpy()
    r = within_one_ulp(got, highpass_restated(x, fs, fc, P=padlen), 'padlen {}'.format(padlen))
    print('highpass padlen {}: worst error {:.3f} ulp32 of the peak'.format(padlen, r))


@pytest.mark.gpu
@pytest.mark.parametrize('fs_in,fs_out', RATE_PAIRS)
def test_resample_against_restatement(fs_in, fs_out):
    """N = 1 and 2: every tap but one or two reads outside [0, N)."""
    from percivaltts_amd import ops
    worst = 0.0
    for N in (1, 2, 255, 4097):
        x = signal('sine', N, fs_in, seed=3)
        got = ops.resample(_dev(x), fs_in, fs_out).cpu().numpy()
        want = resample_restated(x, fs_in, fs_out)
        worst = max(worst, within_one_ulp(got, want, 'resample {} -> {} N={}'.format(fs_in, fs_out, N)))
    assert (ops.resample(_dev(np.zeros(300)), fs_in, fs_out).cpu().numpy() == 0).all()
    print('resample {} -> {}: worst error {:.3f} ulp32 of the peak'.format(fs_in, fs_out, worst))


@pytest.mark.gpu
def test_same_rate_is_the_identity_without_a_launch():
    from percivaltts_amd import ops
    x = _dev(signal('sine', 100, 8000))
    with _hip.KernelTimer() as timer:
        y = ops.resample(x, 8000, 8000)
        ys = ops.resample([x, x[:10]], 16000, 16000)
    assert y is x and ys[0] is x and len(ys) == 2 and timer.records == []


@pytest.mark.gpu
def test_batch_independence():
    """Five utterances of different lengths in one launch, the shortest at padlen + 1: bit-identical to five single launches."""
    from percivaltts_amd import ops
    chunk, tile = tile_geometry()
    lens = [PADLEN + 1, tile + 5, 3 * chunk, 777, 2 * tile - PADLEN]
    wavs = [_dev(signal('sine', N, 16000, seed=i)) for i, N in enumerate(lens)]
    together = ops.highpass_zerophase(wavs, 16000, 70.0)
    assert isinstance(together, list) and [t.numel() for t in together] == lens
    for w, t in zip(wavs, together):
        assert torch.equal(ops.highpass_zerophase(w, 16000, 70.0), t)
    for fs_in, fs_out in ((44100, 16000), (8000, 16000)):
        up, down = ratio(fs_in, fs_out)[:2]
        together = ops.resample(wavs, fs_in, fs_out)
        assert [t.numel() for t in together] == [(N * up + down - 1) // down for N in lens]
        for w, t in zip(wavs, together):
            assert torch.equal(ops.resample(w, fs_in, fs_out), t)


@pytest.mark.gpu
def test_guard_elements_stay():
    """The C entry points with sentinels around y and around the workspace."""
    from percivaltts_amd import ops
    from percivaltts_amd._hip import call, ptr, stream
    lib = _hip.lib()
    chunk, tile = tile_geometry()
    G, SENT = 64, -7.0
    lens = [PADLEN + 1, tile + 3, 100]
    x = torch.cat([_dev(signal('sine', N, 16000, seed=i)) for i, N in enumerate(lens)])
    total = x.numel()
    off = torch.tensor(np.concatenate([[0], np.cumsum(lens)]), dtype=torch.int64).cuda()
    ybuf = torch.full((total + 2 * G,), SENT, dtype=torch.float32, device='cuda')
    nws = lib.ptts_highpass_workspace_bytes(total, len(lens), PADLEN)
    wbuf = torch.full((nws // 8 + 2 * G,), SENT, dtype=torch.float64, device='cuda')
    call('ptts_highpass_zerophase', ptr(x), ctypes.c_void_p(ybuf.data_ptr() + 4 * G), ptr(off), total, len(lens), 16000.0, 70.0, PADLEN,
         ctypes.c_void_p(wbuf.data_ptr() + 8 * G), nws, stream())
    y, w = ybuf.cpu().numpy(), wbuf.cpu().numpy()
    assert (y[:G] == SENT).all() and (y[G + total:] == SENT).all() and (w[:G] == SENT).all() and (w[G + nws // 8:] == SENT).all()
    assert (y[G:G + total] != SENT).all() and (w[G:G + nws // 8] != SENT).all()
    want = torch.cat(ops.highpass_zerophase(list(torch.split(x, lens)), 16000, 70.0)).cpu().numpy()
    np.testing.assert_array_equal(y[G:G + total], want)

    fs_in, fs_out = 44100, 16000
    up, down, _, _, hw = ratio(fs_in, fs_out)
    outs = [(N * up + down - 1) // down for N in lens]
    yoff = torch.tensor(np.concatenate([[0], np.cumsum(outs)]), dtype=torch.int64).cuda()
    tout = sum(outs)
    ybuf = torch.full((tout + 2 * G,), SENT, dtype=torch.float32, device='cuda')
    h = ops.resample_table(fs_in, fs_out, device=x.device)
    call('ptts_resample', ptr(x), ptr(off), total, ctypes.c_void_p(ybuf.data_ptr() + 4 * G), ptr(yoff), tout, max(outs), len(lens), ptr(h),
         h.numel() * 8, up, down, hw, stream())
    y = ybuf.cpu().numpy()
    assert (y[:G] == SENT).all() and (y[G + tout:] == SENT).all() and (y[G:G + tout] != SENT).all()
    want = torch.cat(ops.resample(list(torch.split(x, lens)), fs_in, fs_out)).cpu().numpy()
    np.testing.assert_array_equal(y[G:G + tout], want)


@pytest.mark.gpu
def test_preprocwav_numpy_and_device(capsys):
    from percivaltts_amd import ops, vocoders
    voc = vocoders.VocoderPML(8000, SHIFT, 9, 9, dftlen=512)
    wav = signal('sine', 3000, 16000).astype(np.float64)
    capsys.readouterr()
    a = voc.preprocwav(wav, 16000, 100.0)
    lines = capsys.readouterr().out.splitlines()
    assert lines == ['    Resampling the waveform (new fs=8000Hz)', '    High-pass filter the waveform (cutt-off=100.0Hz)']
    b = voc.preprocwav(_dev(wav), 16000, 100.0)
    assert isinstance(a, np.ndarray) and a.dtype == np.float32 and a.shape == (1500,) and torch.is_tensor(b) and b.is_cuda
    np.testing.assert_array_equal(a, b.cpu().numpy())
    chain = ops.highpass_zerophase(ops.resample(_dev(wav), 16000, 8000), 8000, 100.0)
    np.testing.assert_array_equal(a, chain.cpu().numpy())
    want = highpass_restated(resample_restated(wav.astype(np.float32), 16000, 8000).astype(np.float32), 8000, 100.0)
    within_one_ulp(a, want, 'preprocwav')
    # the offset of 0.2 is gone: what is left of the mean over these 1100 samples is the sine's last, incomplete period, at most
    # 0.25 (2 / pi) / 60 periods = 2.7e-3, and the noise's mean, 0.02 / sqrt(1100) = 6e-4 a standard deviation
    assert abs(float(a[200:-200].mean())) < 0.01 and abs(float(wav[400:-400].mean()) - 0.2) < 0.01
    capsys.readouterr()
    same = voc.preprocwav(wav, 8000, None)                      # nothing to do: no line is printed
    assert same.dtype == np.float32
    np.testing.assert_array_equal(same, wav.astype(np.float32))
    assert capsys.readouterr().out == ''


@pytest.mark.gpu
def test_features_extraction_with_preprocessing(tmp_path, monkeypatch):
    """A vocoder at 8 kHz with dftlen 512; two 0.6 s files at 16 000 and 11 025 Hz with an offset of 0.1 go through preprocwav
    (preproc_hp='auto' = f0_min) and give exactly the streams of analysis_device(preprocwav(wavread(...))); a corpus already at
    8 kHz with preproc_hp=None gives the bytes of a direct analysisfid_device call."""
    import importlib
    from percivaltts_amd import vocoders
    monkeypatch.setenv('PERCIVAL_CORPUS', str(tmp_path / 'corpus'))
    monkeypatch.chdir(tmp_path)
    import percivaltts_amd.run as run
    run = importlib.reload(run)
    run.cfg.id_valid_start = 1
    voc = run.vocoder = vocoders.VocoderPML(8000, SHIFT, 9, 9, dftlen=512)
    run.cfg.outpath = str(tmp_path / 'corpus' / 'cmp' / '*.cmp') + ':(-1,{})'.format(voc.featuressize())
    os.makedirs(str(tmp_path / 'corpus' / 'wav'))
    os.makedirs(str(tmp_path / 'corpus' / 'wav8'))
    rng = np.random.RandomState(21)

    def synth(fs):
        N = int(0.6 * fs)
        f0 = 150.0 + 40.0 * np.sin(np.arange(N) / float(fs) * 9.0 + rng.rand())
        phase = 2 * np.pi * np.cumsum(f0) / fs
        return 0.1 + 0.1 * sum(np.cos(h * phase) / h for h in range(1, 12)) + 0.005 * rng.randn(N)

    fids, rates = ['utt_a', 'utt_b'], [16000, 11025]
    for fid, fs in zip(fids, rates):
        vocoders.wavwrite(str(tmp_path / 'corpus' / 'wav' / (fid + '.wav')), synth(fs), fs)
        vocoders.wavwrite(str(tmp_path / 'corpus' / 'wav8' / (fid + '.wav')), synth(8000), 8000)
    with open(run.cfg.fileids, 'w') as f:
        f.write('\n'.join(fids) + '\n')
    raw = [str(tmp_path / 'corpus' / d / ('*.' + d)) for d in ('lf0', 'spec', 'nm')]
    run.features_extraction(f0in_path=None, rawpaths=raw, f0_min=F0_MIN, f0_max=F0_MAX, preproc_hp='auto')
    s1 = 1 + voc.specsize()
    for fid in fids:
        wav, fs = vocoders.wavread(str(tmp_path / 'corpus' / 'wav' / (fid + '.wav')))
        pre = voc.preprocwav(wav, fs, highpass=F0_MIN)
        assert abs(float(pre.mean())) < 5e-3 and abs(float(wav.mean()) - 0.1) < 5e-3
        CMP = voc.analysis_device(pre, None, F0_MIN, F0_MAX)
        for path, cols in zip(raw, (CMP[:, 0], CMP[:, 1:s1], CMP[:, s1:])):
            np.testing.assert_array_equal(np.fromfile(path.replace('*', fid), dtype=np.float32), np.ascontiguousarray(cols).reshape(-1))
        cmp = np.fromfile(run.cfg.outpath.split(':')[0].replace('*', fid), dtype=np.float32)
        assert cmp.shape == (CMP.shape[0] * voc.featuressize(),) and np.isfinite(cmp).all()

    raw8 = [str(tmp_path / 'corpus' / ('a_' + d) / ('*.' + d)) for d in ('lf0', 'spec', 'nm')]
    direct = [str(tmp_path / 'corpus' / ('b_' + d) / ('*.' + d)) for d in ('lf0', 'spec', 'nm')]
    wav8 = str(tmp_path / 'corpus' / 'wav8' / '*.wav')
    run.features_extraction(f0in_path=None, wav_path=wav8, rawpaths=raw8, f0_min=F0_MIN, f0_max=F0_MAX, preproc_hp=None)
    for fid in fids:
        voc.analysisfid_device(fid, wav8, None, F0_MIN, F0_MAX, {'f0': direct[0], 'spec': direct[1], 'noise': direct[2]})
        for a, b in zip(raw8, direct):
            with open(a.replace('*', fid), 'rb') as fa, open(b.replace('*', fid), 'rb') as fb:
                assert fa.read() == fb.read()
