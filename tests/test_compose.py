"""Feature composition: csrc/compose.hip (ops.compose_windows / compose_sqdev / compose_normalise) and percivaltts_amd/compose.py.

The reference (percivaltts/compose.py) cannot run here (Python 2), so parity is by a numpy restatement of its three parts, written
below with its loop structure and dtypes: the normalisers (:34-183; fp32 arithmetic on fp32 files), compose (:186-362; one file at
a time, the window streams through scipy.signal.convolve in fp64, per-file sums accumulated in fp64, the centred second pass over
the fp32 files it wrote) and the time weights (:365-455).  `convention='mlpg'` restates the other tap order the same way
(convolution with the reversed window, not negated).

Tolerances, derived and not tuned (u = 2^-53, n = frames that count for the statistics):
  * static columns, min.dat, max.dat, every normaliser output and *4norm.dat: equal (rounding is monotone; the normalisers are fp32
    elementwise in numpy's operation order).
  * window columns: |got - want| <= 2^-23 |want| + 2^-50 sum_j |w_j y_j| for EVERY element -- one fp32 ulp for a different fp64
    summation order flipping the final rounding, and that fp64 error itself (two additions and three products, < 4u sum|w_j y_j|,
    doubled for the two orders).
  * mean (fp64, before the cast): |d| <= n u mean_r|y|, the first-order bound of a recursive fp64 sum of n terms divided by n.  It
    is asserted against an extended-precision sum of the restatement's rows in every case, and against the restatement's own mean;
    WITHOUT windows the reference sums each file in fp32 (Y is float32 there, numpy accumulates axis 0 in the array's dtype), so
    there the restatement's own error, sum_files (T_f - 1) 2^-24 sum_{r in f}|y| / n, is added -- the device sums in fp64 always.
  * sum of squared deviations S = sum_r (y_r - m)^2: |dS| <= (n + 3) u S + 2 b_m sum_r|y_r - m| + n b_m^2, with b_m the bound
    on the mean above: n u S for the summation, 3u S for the subtraction's and the square's roundings, and the rest for the two
    sides centring on means that may differ by b_m ((y - m - e)^2 summed is S - 2e sum(y - m) + n e^2).
"""
import ctypes
import os
import re

import numpy as np
import pytest
import scipy.linalg
import scipy.signal

from percivaltts_amd import _hip, compose, data, ops

REF_WINS = [[-0.5, 0.0, 0.5], [1.0, -2.0, 1.0]]
ASYM_WINS = [[-0.7, 0.1, 0.4], [0.9, -2.1, 1.3]]
U64, U32 = 2.0 ** -53, 2.0 ** -24


# ---------------------------------------------------------------------------------------------------------------------------
# the restatement
# ---------------------------------------------------------------------------------------------------------------------------
def closed_form(y, w, convention='reference'):
    """The issue's formula for one column y [T] (fp64) and one window; frame 0 repeats frame 1, frame T-1 frame T-2."""
    y = np.asarray(y, dtype=np.float64)
    out = np.empty_like(y)
    if convention == 'reference':
        out[1:-1] = -(w[0] * y[2:] + w[1] * y[1:-1] + w[2] * y[:-2])
    else:
        out[1:-1] = w[0] * y[:-2] + w[1] * y[1:-1] + w[2] * y[2:]
    out[0], out[-1] = out[1], out[-2]
    return out


def ref_windows(Y, wins, convention='reference'):
    """compose.py:239-250: Y [T,D] float32 -> [T,(1+len(wins))*D]; float64 as soon as there is a window, as in the reference."""
    if len(wins) == 0:
        return Y
    YWs = [Y]
    for win in wins:
        YW = np.ones(Y.shape)
        win_p = (len(win) + 1) // 2
        for d in range(Y.shape[1]):
            if convention == 'reference':
                YW[win_p - 1:-(win_p - 1), d] = -scipy.signal.convolve(Y[:, d], win)[win_p:-win_p]
            else:
                YW[win_p - 1:-(win_p - 1), d] = scipy.signal.convolve(Y[:, d], win[::-1])[win_p:-win_p]
            YW[:win_p - 1, d] = YW[win_p - 1, d]
            YW[-(win_p - 1):, d] = YW[-(win_p - 1) - 1, d]
        YWs.append(YW)
    return np.hstack(YWs)


def abs_windows(Y, wins):
    """sum_j |w_j y_j| of every composed element (0 in the static columns): the scale of the window tolerance."""
    A = np.abs(Y.astype(np.float64))
    outs = [np.zeros(Y.shape)]
    for win in wins:
        aw = [abs(float(c)) for c in win]
        outs.append(np.stack([closed_form(A[:, d], aw, 'mlpg') for d in range(Y.shape[1])], axis=1))
    return np.hstack(outs)


def _read_streams(featurepaths, fid):
    features, minlen = [], None
    for featurepath in featurepaths:
        infilepath, shape = data.getpathandshape(featurepath)
        if shape is None: shape = (-1, 1)
        feature = np.fromfile(infilepath.replace('*', fid), dtype='float32').reshape(shape)
        features.append(feature)
        minlen = feature.shape[0] if minlen is None else min(minlen, feature.shape[0])
    return np.hstack([f[:minlen, ] for f in features])


def ref_normalise_minmax(filepath, fids, outfilepath=None, featurepaths=None, nrange=None, keepidx=None, zerovarstozeros=True, verbose=1):
    if nrange is None: nrange = [-1, 1]
    if outfilepath is None: outfilepath = filepath
    mins = np.fromfile(os.path.dirname(filepath) + '/min.dat', dtype='float32')
    maxs = np.fromfile(os.path.dirname(filepath) + '/max.dat', dtype='float32')
    orisize = len(maxs)
    if keepidx is None: keepidx = np.arange(len(mins))
    mins, maxs = mins[keepidx], maxs[keepidx]
    os.makedirs(os.path.dirname(outfilepath), exist_ok=True)
    mins.astype('float32').tofile(os.path.dirname(outfilepath) + '/min4norm.dat')
    maxs.astype('float32').tofile(os.path.dirname(outfilepath) + '/max4norm.dat')
    maxmindiff = maxs - mins
    if zerovarstozeros: mins[maxmindiff == 0.0] = 0.0
    maxmindiff[maxmindiff == 0.0] = 1.0
    for fid in fids:
        Y = np.fromfile(filepath.replace('*', fid), dtype='float32').reshape((-1, orisize))
        Y = Y[:, keepidx]
        Y = (Y - mins) / maxmindiff
        Y -= 0.5
        Y *= 2.0
        Y *= (nrange[1] - nrange[0]) / 2.0
        Y += 0.5 * (nrange[0] + nrange[1])
        assert Y.dtype == np.float32
        Y.astype('float32').tofile(outfilepath.replace('*', fid))


def ref_normalise_meanstd(filepath, fids, outfilepath=None, featurepaths=None, keepidx=None, verbose=1, _nmnoscale=False):
    if outfilepath is None: outfilepath = filepath
    means = np.fromfile(os.path.dirname(filepath) + '/mean.dat', dtype='float32')
    stds = np.fromfile(os.path.dirname(filepath) + '/std.dat', dtype='float32')
    if _nmnoscale:
        f0size, specsize, nmsize = (data.getlastdim(featurepaths[i]) for i in range(3))
        raw = f0size + specsize + nmsize
        for k in range(3):
            if k == 0 or len(means) > k * raw:
                means[k * raw + f0size + specsize:k * raw + raw] = 0.0
                stds[k * raw + f0size + specsize:k * raw + raw] = 1.0
    os.makedirs(os.path.dirname(outfilepath), exist_ok=True)
    means.astype('float32').tofile(os.path.dirname(outfilepath) + '/mean4norm.dat')
    stds.astype('float32').tofile(os.path.dirname(outfilepath) + '/std4norm.dat')
    stds[stds == 0.0] = 1.0
    for fid in fids:
        Y = np.fromfile(filepath.replace('*', fid), dtype='float32').reshape((-1, len(means)))
        Y = (Y - means) / stds
        assert Y.dtype == np.float32
        Y.astype('float32').tofile(outfilepath.replace('*', fid))


def ref_normalise_meanstd_nmnoscale(filepath, fids, outfilepath=None, featurepaths=None, keepidx=None, verbose=1):
    ref_normalise_meanstd(filepath, fids, outfilepath, featurepaths, keepidx, verbose, _nmnoscale=True)


def ref_compose(featurepaths, fids, outfilepath, wins=None, id_valid_start=-1, normfn=None, dropzerovardims=False,
                convention='reference'):
    """compose.py:186-328.  Returns the fp64 statistics and what the bounds of the module docstring need."""
    if wins is None: wins = []
    outfilepath = re.sub(r':[^:]+$', '', outfilepath)
    outdir = os.path.dirname(outfilepath)
    os.makedirs(outdir, exist_ok=True)
    mins = maxs = means = None
    nbframes = 0
    rows, fp32_sum_err = [], 0.0
    for nf, fid in enumerate(fids):
        Y = ref_windows(_read_streams(featurepaths, fid), wins, convention)
        size = Y.shape[1]
        if nf < id_valid_start:
            mins = Y.min(axis=0) if mins is None else np.minimum(mins, Y.min(axis=0))
            maxs = Y.max(axis=0) if maxs is None else np.maximum(maxs, Y.max(axis=0))
            means = Y.sum(axis=0).astype('float64') if means is None else means + Y.sum(axis=0).astype('float64')
            nbframes += Y.shape[0]
            rows.append(Y.astype(np.float64))
            if Y.dtype == np.float32:
                fp32_sum_err = fp32_sum_err + (Y.shape[0] - 1) * U32 * np.abs(Y.astype(np.float64)).sum(axis=0)
        Y.astype('float32').tofile(outfilepath.replace('*', fid))
    means /= nbframes
    zerovaridx = np.where((maxs - mins) == 0.0)[0]
    mins.astype('float32').tofile(outdir + '/min.dat')
    maxs.astype('float32').tofile(outdir + '/max.dat')
    means.astype('float32').tofile(outdir + '/mean.dat')
    stds = None
    for nf, fid in enumerate(fids):
        Y = np.fromfile(outfilepath.replace('*', fid), dtype='float32').reshape((-1, size))
        if nf < id_valid_start:
            stds = ((Y - means) ** 2).sum(axis=0).astype('float64') if stds is None else stds + ((Y - means) ** 2).sum(axis=0).astype('float64')
    sqdev = stds.copy()
    with np.errstate(divide='ignore', invalid='ignore'):
        stds = np.sqrt(stds / (nbframes - 1))
    stds.astype('float32').tofile(outdir + '/std.dat')
    keepidx = np.arange(len(means))
    if dropzerovardims:
        keepidx = np.setdiff1d(np.arange(len(means)), zerovaridx)
        keepidx.astype('int32').tofile(outdir + '/keepidx.dat')
    if normfn is not None:
        normfn(outfilepath, fids, featurepaths=featurepaths, keepidx=keepidx, verbose=0)
    rows = np.vstack(rows)
    exact_mean = (rows.astype(np.longdouble).sum(axis=0) / nbframes).astype(np.float64)
    return dict(min=mins, max=maxs, mean=means, std=stds, sqdev=sqdev, nbframes=nbframes, keepidx=keepidx, exact_mean=exact_mean,
                absmean=np.abs(rows).mean(axis=0), ref_mean_err=fp32_sum_err / nbframes)


REF_NORMFN = {None: None, 'minmax': ref_normalise_minmax, 'meanstd': ref_normalise_meanstd, 'nmnoscale': ref_normalise_meanstd_nmnoscale}
DEV_NORMFN = {None: None, 'minmax': compose.normalise_minmax, 'meanstd': compose.normalise_meanstd,
              'nmnoscale': compose.normalise_meanstd_nmnoscale}


# ---------------------------------------------------------------------------------------------------------------------------
# corpora
# ---------------------------------------------------------------------------------------------------------------------------
LENS = [3, 70, 130, 5, 257, 64, 33, 4, 41]         # ragged, not multiples of the four waves, a 3-frame utterance
NSTAT = 6                                           # id_valid_start: the last three files do not count for the statistics
SPEC, NM = 70, 5                                    # D = 1 + 70 + 5 = 76: crosses one 64-lane column block


def make_corpus(root, lens=LENS, spec=SPEC, nm=NM, nstat=NSTAT, seed=0, dead=True):
    """lf0 (no shape suffix: one column, mean 5 std 0.3) | spec (random walks; with `dead` a constant column, an all-zero column
    and a harsh one: offset 1000, spread 0.01) | noise mask in [0,1].  The streams of a file differ in length (cropping); the
    files from `nstat` on hold very different values, which must not reach the statistics."""
    rng = np.random.RandomState(seed)
    raw = os.path.join(str(root), 'raw')
    os.makedirs(raw, exist_ok=True)
    fids = ['utt_{:02d}'.format(i) for i in range(len(lens))]
    for i, (fid, n) in enumerate(zip(fids, lens)):
        lf0 = 5.0 + 0.3 * rng.randn(n + 1, 1)
        sp = np.cumsum(rng.randn(n + 2, spec), axis=0) * 0.2 + rng.randn(spec)
        if dead:
            sp[:, 3] = 2.5
            sp[:, 4] = 0.0
            sp[:, 5] = 1000.0 + 0.01 * rng.randn(n + 2)
        noise = rng.rand(n, nm)
        if i >= nstat:
            lf0, sp, noise = lf0 * 100 + 1000, sp * 100 - 1000, noise * 50 + 7
        lf0.astype(np.float32).tofile(os.path.join(raw, fid + '.lf0'))
        sp.astype(np.float32).tofile(os.path.join(raw, fid + '.spec'))
        noise.astype(np.float32).tofile(os.path.join(raw, fid + '.nm'))
    paths = [raw + '/*.lf0', raw + '/*.spec:(-1,{})'.format(spec), raw + '/*.nm:(-1,{})'.format(nm)]
    return fids, paths


def listing(d):
    return sorted(os.listdir(str(d)))


def f32file(path, width=None):
    a = np.fromfile(str(path), dtype=np.float32)
    return a if width is None else a.reshape(-1, width)


def assert_same_files(da, db, what=''):
    assert listing(da) == listing(db), what
    for name in listing(da):
        with open(os.path.join(str(da), name), 'rb') as f, open(os.path.join(str(db), name), 'rb') as g:
            assert f.read() == g.read(), (what, name)


# ---------------------------------------------------------------------------------------------------------------------------
# CPU
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('wins', [REF_WINS, ASYM_WINS], ids=['ref', 'asym'])
@pytest.mark.parametrize('convention', ['reference', 'mlpg'])
def test_restatement_window_rule_equals_closed_form(wins, convention):
    rng = np.random.RandomState(1)
    for T in (3, 4, 5, 64, 700):
        Y = (rng.randn(T, 3) * [1.0, 0.01, 30.0] + [0.0, 1000.0, 5.0]).astype(np.float32)
        got = ref_windows(Y, wins, convention)
        assert got.dtype == np.float64 and got.shape == (T, 9)
        np.testing.assert_array_equal(got[:, :3], Y)
        scale = abs_windows(Y, wins)
        for k, w in enumerate(wins):
            for d in range(3):
                want = closed_form(Y[:, d], w, convention)
                err = np.abs(got[:, (k + 1) * 3 + d] - want)
                assert (err <= 2.0 ** -50 * scale[:, (k + 1) * 3 + d]).all(), (T, k, d, err.max())


def test_conventions_coincide_for_the_antisymmetric_window_only():
    rng = np.random.RandomState(2)
    Y = rng.randn(50, 4).astype(np.float32)
    a, b = ref_windows(Y, REF_WINS, 'reference'), ref_windows(Y, REF_WINS, 'mlpg')
    np.testing.assert_array_equal(a[:, :8], b[:, :8])                   # statics and [-0.5, 0, 0.5]
    np.testing.assert_array_equal(a[:, 8:], -b[:, 8:])                  # [1, -2, 1]: the negative
    assert np.abs(a[:, 8:] - b[:, 8:]).max() > 0.1
    c, d = ref_windows(Y, ASYM_WINS, 'reference'), ref_windows(Y, ASYM_WINS, 'mlpg')
    assert np.abs(c[:, 4:] - d[:, 4:]).max() > 0.1


def test_argument_errors(tmp_path, monkeypatch):
    fids, paths = make_corpus(tmp_path, lens=[5, 2, 6], nstat=3)
    out = str(tmp_path / 'out') + '/*.cmp'
    for bad in (-1, 0):
        with pytest.raises(ValueError, match='id_valid_start'):
            compose.compose(paths, fids, out, id_valid_start=bad)
    with pytest.raises(ValueError, match='id_valid_start'):
        compose.compose(paths, fids, out)                                           # the default
    for wins in ([[1.0, -1.0]], [[1, 2, 3, 4, 5]], [REF_WINS[0], [0.5]]):
        with pytest.raises(ValueError, match='three taps'):
            compose.compose(paths, fids, out, wins=wins, id_valid_start=2)
        with pytest.raises(ValueError):
            ops.compose_window_taps(wins)
    assert ops.compose_window_taps(None) == [] and ops.compose_window_taps(REF_WINS) == [-0.5, 0.0, 0.5, 1.0, -2.0, 1.0]
    with pytest.raises(ValueError, match='utt_01'):                                # 2 frames and windows
        compose.compose(paths, fids, out, wins=REF_WINS, id_valid_start=2)
    with pytest.raises(ValueError, match='win_convention'):
        compose.compose(paths, fids, out, wins=REF_WINS, id_valid_start=2, win_convention='merlin')


def test_compose_without_a_device_raises(tmp_path, monkeypatch):
    import torch
    fids, paths = make_corpus(tmp_path, lens=[5, 4, 6], nstat=3)
    monkeypatch.setattr(torch.cuda, 'is_available', lambda: False)
    with pytest.raises(_hip.HipLibraryError):
        compose.compose(paths, fids, str(tmp_path / 'out') + '/*.cmp', wins=REF_WINS, id_valid_start=2)
    np.zeros(3, np.float32).tofile(str(tmp_path / 'raw' / 'mean.dat'))
    np.ones(3, np.float32).tofile(str(tmp_path / 'raw' / 'std.dat'))
    with pytest.raises(_hip.HipLibraryError):
        compose.normalise_meanstd(str(tmp_path / 'raw') + '/*.lf0', fids, str(tmp_path / 'o2') + '/*.lf0')
    with pytest.raises(_hip.HipLibraryError):
        ops.compose_windows(torch.zeros(4, 2), torch.tensor([0, 4], dtype=torch.int32), REF_WINS)


def test_header_declares_and_library_exports_the_symbols():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, 'include', 'percival_hip.h')) as f:
        header = f.read()
    names = ['ptts_compose_windows_workspace_bytes', 'ptts_compose_windows', 'ptts_compose_sqdev_workspace_bytes',
             'ptts_compose_sqdev', 'ptts_compose_normalise']
    assert 'size_t ptts_compose_windows_workspace_bytes(int N, int D, int K);' in header
    assert 'size_t ptts_compose_sqdev_workspace_bytes(int N, int W);' in header
    for n in names:
        assert re.search(r'\b(int|size_t) {}\('.format(n), header), n
        assert n in _hip.SIGNATURES, n
    with open(os.path.join(root, 'INTEGRATION.md')) as f:
        assert 'ptts_compose_windows' in f.read()
    assert os.path.exists(_hip.LIB_PATH), 'libpercival_hip.so not built (run __graft_entry__.build())'
    lib = ctypes.CDLL(_hip.LIB_PATH)
    for n in names:
        assert hasattr(lib, n), n


def test_entry_points_reject_bad_arguments():
    """PTTS_EINVAL / PTTS_EWORKSPACE before any launch, the message naming the entry point; no pointer is dereferenced."""
    lib = _hip.lib()
    p = ctypes.c_void_p(256)            # non-null, never read
    EINVAL, EWORKSPACE = -1, -3
    big = 1 << 40
    wins = (ctypes.c_double * 6)(*[c for w in REF_WINS for c in w])

    def win(y=p, offs=p, w=wins, order=0, out=ctypes.c_void_p(512), rmin=p, rmax=p, rsum=p, ns=2, ws=p, nws=big, N=3, R=20, D=4, K=3):
        return lib.ptts_compose_windows(y, offs, w, order, out, rmin, rmax, rsum, ns, ws, nws, N, R, D, K, None)
    for kw in (dict(y=None), dict(offs=None), dict(out=None), dict(w=None), dict(N=0), dict(N=-1), dict(R=0), dict(D=0), dict(D=-5),
               dict(K=0), dict(K=9), dict(ns=-1), dict(rmin=None), dict(rsum=None), dict(out=p)):
        assert win(**kw) == EINVAL, kw
        assert 'compose_windows' in _hip.last_error(), kw
    need = lib.ptts_compose_windows_workspace_bytes(2, 4, 3)
    assert need >= 2 * 12 * 16
    assert lib.ptts_compose_windows_workspace_bytes(100000, 200, 3) >= 100000 * 600 * 16           # beyond 32 bits
    assert win(nws=need - 1) == EWORKSPACE and win(ws=None, nws=need) == EWORKSPACE
    assert 'compose_windows: workspace' in _hip.last_error()

    def sq(y=p, offs=p, mean=p, run=p, ns=2, ws=p, nws=big, N=3, R=20, W=12):
        return lib.ptts_compose_sqdev(y, offs, mean, run, ns, ws, nws, N, R, W, None)
    for kw in (dict(y=None), dict(offs=None), dict(mean=None), dict(run=None), dict(N=0), dict(R=-1), dict(W=0), dict(ns=-2)):
        assert sq(**kw) == EINVAL, kw
        assert 'compose_sqdev' in _hip.last_error(), kw
    need = lib.ptts_compose_sqdev_workspace_bytes(2, 12)
    assert need >= 2 * 12 * 8
    assert sq(nws=need - 1) == EWORKSPACE and sq(ws=None, nws=need) == EWORKSPACE
    assert 'compose_sqdev: workspace' in _hip.last_error()

    def nrm(y=p, kidx=None, a=p, b=p, mode=0, s=1.0, o=0.0, out=p, R=5, Win=4, Wout=4):
        return lib.ptts_compose_normalise(y, kidx, a, b, mode, s, o, out, R, Win, Wout, None)
    for kw in (dict(y=None), dict(a=None), dict(b=None), dict(out=None), dict(R=0), dict(R=-1), dict(Win=0), dict(Wout=-1),
               dict(mode=2), dict(mode=-1), dict(Wout=3), dict(kidx=p)):
        assert nrm(**kw) == EINVAL, kw                              # the last: a column gather in place (out == y)
        assert 'compose_normalise' in _hip.last_error(), kw


def test_create_weights_spec_hand_written(tmp_path):
    d = str(tmp_path)
    db = np.log(10.0) / 20.0                # log amplitude of 1 dB
    # fwlspec: the energy is the mean of the log spectrum; relative to the loudest frame: 0, -31, -33, -32 (the threshold), -60 dB
    rel = np.array([0.0, -31.0, -33.0, -32.0, -60.0])
    spec = (rel[:, None] * db + np.array([[0.5, -0.5, 0.25, -0.25]])).astype(np.float32) + 2.0
    spec.tofile(d + '/a.spec')
    compose.create_weights_spec(d + '/*.spec:(-1,4)', ['a'], d + '/w/*.w:(-1,1)')
    got = f32file(d + '/w/a.w')
    np.testing.assert_array_equal(got[[0, 1, 2, 4]], [1.0, 1.0, 0.0, 0.0])
    assert got.shape == (5,) and got[3] in (0.0, 1.0)                   # exactly on the threshold up to fp32 rounding
    # mcep / fwcep: the first coefficient alone decides; another threshold
    cep = np.zeros((4, 3), dtype=np.float32)
    cep[:, 0] = np.array([0.0, -10.0, -25.0, -5.0]) * db
    cep[:, 1] = [9.0, -9.0, 9.0, -9.0]
    cep.tofile(d + '/b.spec')
    for st in ('mcep', 'fwcep'):
        compose.create_weights_spec(d + '/*.spec:(-1,3)', ['b'], d + '/w2/*.w', thresh=-20, spec_type=st)
        np.testing.assert_array_equal(f32file(d + '/w2/b.w'), [1.0, 1.0, 0.0, 1.0])
    with pytest.raises(ValueError):
        compose.create_weights_spec(d + '/*.spec:(-1,3)', ['b'], d + '/w2/*.w', spec_type='lsf')


def test_create_weights_lab_hand_written(tmp_path):
    d = str(tmp_path)
    lab = ['0 512000 x^x-sil+h=e@1_1',              # 0.0000 - 0.0512 s: silence -> frames 0 .. ceil(10.24) - 1 = 10
           '512000 1210000 x^sil-h+e=l@1_2',        # 0.0512 - 0.1210 s
           '1210000 1800000 sil^h-e+l=o@2_1',       # 'sil' as a neighbour does not count
           '1800000 2530000 h^e-l+sil=x@3_1',       # ends at 0.253 s
           '2530000 3010000 e^l-sil+x=x@1_1']       # 0.253 - 0.301 s: silence -> frames floor(50.6) = 50 .. ceil(60.2) = 61
    with open(d + '/u1.lab', 'w') as f:
        f.write('\n'.join(lab) + '\n')
    with open(d + '/ids.scp', 'w') as f:
        f.write('u1\n')
    compose.create_weights_lab(d + '/*.lab', d + '/ids.scp', d + '/w/*.w:(-1,1)')
    want = np.ones(61, dtype=np.float32)
    want[:11] = 0.0
    want[50:] = 0.0
    np.testing.assert_array_equal(f32file(d + '/w/u1.w'), want)
    compose.create_weights_lab(d + '/*.lab', d + '/ids.scp', d + '/w3/*.w', silencesymbol='h', shift=0.01)
    want = np.ones(31, dtype=np.float32)
    want[5:13] = 0.0                            # floor(5.12) .. ceil(12.1) - 1
    np.testing.assert_array_equal(f32file(d + '/w3/u1.w'), want)


# ---------------------------------------------------------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------------------------------------------------------
def check_composed(dev_dir, fids, paths, wins, D, convention='reference'):
    """Static columns equal; every window element within 2^-23|want| + 2^-50 sum|w_j y_j| of the restatement's fp64 value."""
    K = 1 + len(wins)
    worst = 0.0
    for fid in fids:
        got = f32file(os.path.join(dev_dir, fid + '.cmp'), K * D)
        raw = _read_streams(paths, fid)
        assert got.shape == (raw.shape[0], K * D), fid
        np.testing.assert_array_equal(got[:, :D], raw, err_msg=fid)
        if K > 1:
            want = ref_windows(raw, wins, convention)
            tol = 2.0 ** -23 * np.abs(want) + 2.0 ** -50 * abs_windows(raw, wins)
            err = np.abs(got.astype(np.float64) - want)
            worst = max(worst, (err[:, D:] / np.where(tol[:, D:] > 0, tol[:, D:], 1.0)).max())
            assert (err <= tol).all(), (fid, worst)
    print('window columns: worst |got-want| / tolerance = {:.3f}'.format(worst))


def check_statistics(res, ref, dev_dir, ref_dir):
    """min/max equal; mean and the sum of squared deviations within the bounds of the module docstring (figures printed first)."""
    for name in ('min.dat', 'max.dat'):
        np.testing.assert_array_equal(f32file(os.path.join(dev_dir, name)), f32file(os.path.join(ref_dir, name)), err_msg=name)
    n = ref['nbframes']
    assert res['nbframes'] == n
    b_exact = n * U64 * ref['absmean']
    b_ref = b_exact + ref['ref_mean_err']
    e_exact, e_ref = np.abs(res['mean'] - ref['exact_mean']), np.abs(res['mean'] - ref['mean'])
    print('mean: worst |d| / bound: vs extended sum {:.3e}, vs restatement {:.3e} (n = {})'.format(
        (e_exact / np.where(b_exact > 0, b_exact, 1)).max(), (e_ref / np.where(b_ref > 0, b_ref, 1)).max(), n))
    assert (e_exact <= b_exact).all() and (e_ref <= b_ref).all()
    # the files: the casts of the fp64 values, hence within one fp32 ulp of the restatement's files beyond the bound
    np.testing.assert_array_equal(f32file(os.path.join(dev_dir, 'mean.dat')), res['mean'].astype(np.float32))
    np.testing.assert_array_equal(f32file(os.path.join(dev_dir, 'std.dat')), res['std'].astype(np.float32))
    ulp = 2.0 ** -23 * np.abs(ref['mean'])
    assert (np.abs(f32file(os.path.join(dev_dir, 'mean.dat')).astype(np.float64) - f32file(os.path.join(ref_dir, 'mean.dat'))) <= b_ref + ulp).all()
    # S = std^2 (n - 1) of both sides
    S_ref = ref['sqdev']
    S_dev = res['sqdev']
    absdev = np.sqrt(n * S_ref)                     # Cauchy-Schwarz: sum|y - m| <= sqrt(n S)
    b_S = (n + 3) * U64 * S_ref + 2 * b_ref * absdev + n * b_ref ** 2
    e_S = np.abs(S_dev - S_ref)
    print('sum of squared deviations: worst |d| / bound {:.3e}'.format((e_S / np.where(b_S > 0, b_S, 1)).max()))
    assert (e_S <= b_S).all()
    with np.errstate(invalid='ignore', divide='ignore'):
        np.testing.assert_array_equal(res['std'], np.sqrt(S_dev / (n - 1)))
    sref, sdev = f32file(os.path.join(ref_dir, 'std.dat')).astype(np.float64), f32file(os.path.join(dev_dir, 'std.dat')).astype(np.float64)
    # d sqrt(S/(n-1)) = dS / (2 sqrt(S (n-1))), plus one fp32 ulp for the file and the sqrt's own rounding
    with np.errstate(invalid='ignore', divide='ignore'):
        b_std = np.where(S_ref > 0, b_S / (2 * np.sqrt(S_ref * (n - 1))), 0.0) + 2.0 ** -23 * sref + 2 * U64 * sref
    assert (np.abs(sdev - sref) <= b_std).all()


WIN_CASES = [([], 'reference'), (REF_WINS[:1], 'reference'), (REF_WINS, 'reference'), (ASYM_WINS, 'reference'), (REF_WINS, 'mlpg'),
             (ASYM_WINS, 'mlpg')]


@pytest.mark.gpu
@pytest.mark.parametrize('wins,convention', WIN_CASES, ids=['K1', 'K2', 'K3', 'K3asym', 'K3-mlpg', 'K3asym-mlpg'])
def test_composed_values_and_statistics(wins, convention, tmp_path):
    """normfn=None: files, listing and statistics against the restatement; only the first NSTAT files count (the later ones
    hold values a hundred times larger, which would show in every statistic)."""
    fids, paths = make_corpus(tmp_path)
    D = 1 + SPEC + NM
    dev_dir = str(tmp_path / ('dev_' + convention))
    ref_dir = str(tmp_path / 'ref')
    res = compose.compose(paths, fids, dev_dir + '/*.cmp:(-1,{})'.format((1 + len(wins)) * D), wins=wins, id_valid_start=NSTAT,
                          win_convention=convention, verbose=0)
    ref = ref_compose(paths, fids, ref_dir + '/*.cmp', wins=wins, id_valid_start=NSTAT, convention=convention)
    assert listing(dev_dir) == listing(ref_dir) == sorted([f + '.cmp' for f in fids] + ['min.dat', 'max.dat', 'mean.dat', 'std.dat'])
    assert res['resident'] and res['size'] == (1 + len(wins)) * D
    check_composed(dev_dir, fids, paths, wins, D, convention)
    check_statistics(res, ref, dev_dir, ref_dir)
    assert res['max'][0] < 10.0 and res['mean'][0] < 10.0                   # lf0 of the late files is ~1500
    # zero-variance columns: the constant one, the all-zero one, and their window streams
    zero = np.where(res['max'] == res['min'])[0]
    np.testing.assert_array_equal(zero, sorted(k * D + c for k in range(1 + len(wins)) for c in (4, 5)))
    assert (res['std'][zero] == 0).all()


def _stats_dir(tmp_path, W, seed=3, with_zero=True):
    """Given files and given statistics files for the stand-alone normalisers."""
    rng = np.random.RandomState(seed)
    d = str(tmp_path / 'in')
    os.makedirs(d)
    fids = ['f{}'.format(i) for i in range(5)]
    scale = np.exp(rng.uniform(np.log(1e-2), np.log(30.0), size=W))
    offset = rng.randn(W) * 5
    for fid, n in zip(fids, [1, 67, 300, 4, 129]):
        Y = rng.randn(n, W) * scale + offset
        if with_zero: Y[:, 2] = -3.25
        Y.astype(np.float32).tofile(d + '/' + fid + '.cmp')
    allY = np.vstack([f32file(d + '/' + f + '.cmp', W) for f in fids])
    allY.min(axis=0).tofile(d + '/min.dat'); allY.max(axis=0).tofile(d + '/max.dat')
    allY.astype(np.float64).mean(axis=0).astype(np.float32).tofile(d + '/mean.dat')
    allY.astype(np.float64).std(axis=0, ddof=1).astype(np.float32).tofile(d + '/std.dat')
    return d, fids


@pytest.mark.gpu
@pytest.mark.parametrize('case', ['default', 'nrange01', 'keepidx', 'keepidx-nozero', 'inplace'])
def test_normalise_minmax_standalone(case, tmp_path):
    W = 76
    d, fids = _stats_dir(tmp_path, W)
    kw = {}
    if case == 'nrange01': kw['nrange'] = [0, 1]
    if case.startswith('keepidx'): kw['keepidx'] = np.setdiff1d(np.arange(W), [2, 40])
    if case == 'keepidx-nozero': kw.update(keepidx=np.arange(W), zerovarstozeros=False, nrange=[-2.0, 0.5])
    if case == 'inplace':
        import shutil
        shutil.copytree(d, str(tmp_path / 'in2'))
        compose.normalise_minmax(d + '/*.cmp', fids, **kw)
        ref_normalise_minmax(str(tmp_path / 'in2') + '/*.cmp', fids, **kw)
        assert_same_files(d, str(tmp_path / 'in2'), case)
        return
    compose.normalise_minmax(d + '/*.cmp', fids, str(tmp_path / 'dev') + '/*.cmp', **kw)
    ref_normalise_minmax(d + '/*.cmp', fids, str(tmp_path / 'ref') + '/*.cmp', **kw)
    assert_same_files(str(tmp_path / 'dev'), str(tmp_path / 'ref'), case)
    assert listing(tmp_path / 'dev') == sorted([f + '.cmp' for f in fids] + ['min4norm.dat', 'max4norm.dat'])
    wout = len(kw.get('keepidx', np.arange(W)))
    got = np.vstack([f32file(str(tmp_path / 'dev' / (f + '.cmp')), wout) for f in fids])
    if case == 'default':
        assert got[:, 3:].min() == -1.0 and got[:, 3:].max() == 1.0
        assert (got[:, 2] == (-3.25 - 0.5) * 2.0).all()         # zerovarstozeros: min := 0, divide by 1, then centre and scale
    if case == 'nrange01':
        assert got[:, 3:].min() == 0.0 and got[:, 3:].max() == 1.0


@pytest.mark.gpu
@pytest.mark.parametrize('nwins', [0, 1, 2])
@pytest.mark.parametrize('which', ['meanstd', 'nmnoscale'])
def test_normalise_meanstd_standalone(which, nwins, tmp_path):
    raw = 1 + 12 + 4
    W = raw * (1 + nwins)
    d, fids = _stats_dir(tmp_path, W, seed=4 + nwins)
    paths = ['x/*.lf0', 'x/*.spec:(-1,12)', 'x/*.nm:(-1,4)']
    DEV_NORMFN[which](d + '/*.cmp', fids, str(tmp_path / 'dev') + '/*.cmp', featurepaths=paths, keepidx=np.arange(3))
    REF_NORMFN[which](d + '/*.cmp', fids, str(tmp_path / 'ref') + '/*.cmp', featurepaths=paths, keepidx=np.arange(3))
    assert_same_files(str(tmp_path / 'dev'), str(tmp_path / 'ref'), which)
    assert listing(tmp_path / 'dev') == sorted([f + '.cmp' for f in fids] + ['mean4norm.dat', 'std4norm.dat'])
    std4 = f32file(str(tmp_path / 'dev' / 'std4norm.dat'))
    assert std4[2] == 0.0                                                   # the saved std of the constant column stays 0
    assert (f32file(str(tmp_path / 'dev' / 'f2.cmp'), W)[:, 2] == 0.0).all()
    if which == 'nmnoscale':
        src, got = f32file(d + '/f2.cmp', W), f32file(str(tmp_path / 'dev' / 'f2.cmp'), W)
        for k in range(1 + nwins):
            np.testing.assert_array_equal(got[:, k * raw + 13:(k + 1) * raw], src[:, k * raw + 13:(k + 1) * raw])
            assert (std4[k * raw + 13:(k + 1) * raw] == 1.0).all()


E2E = [(nf, wins) for nf in (None, 'minmax', 'meanstd', 'nmnoscale') for wins in ([], REF_WINS)]


@pytest.mark.gpu
@pytest.mark.parametrize('normname,wins', E2E, ids=['{}-K{}'.format(n, 1 + len(w)) for n, w in E2E])
@pytest.mark.parametrize('drop', [False, True], ids=['keep', 'dropzerovar'])
def test_compose_end_to_end(normname, wins, drop, tmp_path):
    """The directory listing equals the restatement's; the un-normalised run is within the bounds; the normalised files equal the
    numpy normaliser applied to the device's own composed files and statistics (so that an ulp in a statistic or in a window
    value is not counted twice), and the statistics files do not depend on the normaliser."""
    fids, paths = make_corpus(tmp_path)
    D = 1 + SPEC + NM
    W = (1 + len(wins)) * D
    plain, ref_dir = str(tmp_path / 'dev_reference'), str(tmp_path / 'ref')
    res0 = compose.compose(paths, fids, plain + '/*.cmp', wins=wins, id_valid_start=NSTAT, dropzerovardims=drop, verbose=0)
    ref = ref_compose(paths, fids, ref_dir + '/*.cmp', wins=wins, id_valid_start=NSTAT, normfn=REF_NORMFN[normname], dropzerovardims=drop)
    check_composed(plain, fids, paths, wins, D)
    check_statistics(res0, ref, plain, ref_dir)
    np.testing.assert_array_equal(res0['keepidx'], ref['keepidx'])
    if drop:
        assert res0['size'] == W - 2 * (1 + len(wins))
        np.testing.assert_array_equal(np.fromfile(plain + '/keepidx.dat', dtype=np.int32), ref['keepidx'])
    if normname is None:
        assert listing(plain) == listing(ref_dir)
        return
    dev = str(tmp_path / 'dev')
    res = compose.compose(paths, fids, dev + '/*.cmp', wins=wins, id_valid_start=NSTAT, normfn=DEV_NORMFN[normname],
                          dropzerovardims=drop, do_finalcheck=True, verbose=0)
    assert listing(dev) == listing(ref_dir)
    # numpy's normaliser on the device's composed files and statistics
    REF_NORMFN[normname](plain + '/*.cmp', fids, str(tmp_path / 'want') + '/*.cmp', featurepaths=paths, keepidx=res0['keepidx'])
    for name in listing(tmp_path / 'want'):
        with open(os.path.join(dev, name), 'rb') as f, open(str(tmp_path / 'want' / name), 'rb') as g:
            assert f.read() == g.read(), name
    for name in ('min.dat', 'max.dat', 'mean.dat', 'std.dat') + (('keepidx.dat',) if drop else ()):
        with open(os.path.join(dev, name), 'rb') as f, open(os.path.join(plain, name), 'rb') as g:
            assert f.read() == g.read(), name
    # do_finalcheck: the statistics of what was written, by the same kernels
    wout = res['size'] if normname == 'minmax' else W       # as in the reference, only normalise_minmax honours keepidx
    chk = res['finalcheck']
    written = np.vstack([f32file(os.path.join(dev, f + '.cmp'), wout) for f in fids[:NSTAT]]).astype(np.float64)
    np.testing.assert_array_equal(chk['verif_min'], written.min(axis=0).astype(np.float32))
    np.testing.assert_array_equal(chk['verif_max'], written.max(axis=0).astype(np.float32))
    n = written.shape[0]
    assert (np.abs(chk['verif_means'] - written.mean(axis=0)) <= n * U64 * np.abs(written).mean(axis=0)).all()
    np.testing.assert_allclose(chk['verif_stds'], written.var(axis=0, ddof=1), rtol=1e-9, atol=1e-12)
    if normname == 'meanstd' and not drop:
        live = res0['std'] > 0
        # the mean file is an fp32 rounding of the mean: off by up to 2^-24 |mean|, seen through the division by std
        slack = (2.0 ** -23 * np.abs(res0['mean'][live]) / res0['std'][live]) + 1e-5
        assert (np.abs(chk['verif_means'][live]) <= slack).all()
        np.testing.assert_allclose(chk['verif_stds'][live], 1.0, rtol=1e-4)


@pytest.mark.gpu
def test_foreign_normfn_gets_the_reference_protocol(tmp_path):
    fids, paths = make_corpus(tmp_path)
    seen = {}

    def mynorm(outfilepath, fids_, featurepaths=None, keepidx=None, verbose=1):
        seen.update(path=outfilepath, fids=list(fids_), featurepaths=featurepaths, keepidx=np.array(keepidx),
                    listing=listing(os.path.dirname(outfilepath)))
        ref_normalise_meanstd(outfilepath, fids_)
    dev = str(tmp_path / 'dev')
    compose.compose(paths, fids, dev + '/*.cmp:(-1,9)', wins=REF_WINS, id_valid_start=NSTAT, normfn=mynorm, verbose=0)
    assert seen['path'] == dev + '/*.cmp' and seen['fids'] == fids and seen['featurepaths'] == paths
    np.testing.assert_array_equal(seen['keepidx'], np.arange(3 * 76))
    assert seen['listing'] == sorted([f + '.cmp' for f in fids] + ['min.dat', 'max.dat', 'mean.dat', 'std.dat'])
    own = str(tmp_path / 'own')
    compose.compose(paths, fids, own + '/*.cmp', wins=REF_WINS, id_valid_start=NSTAT, normfn=compose.normalise_meanstd, verbose=0)
    assert_same_files(dev, own, 'foreign callable vs own normaliser')


@pytest.mark.gpu
@pytest.mark.parametrize('normname', [None, 'minmax', 'nmnoscale'])
def test_resident_and_streamed_routes_write_identical_files(normname, tmp_path, monkeypatch):
    fids, paths = make_corpus(tmp_path)
    W = 3 * 76
    kw = dict(wins=REF_WINS, id_valid_start=NSTAT, normfn=DEV_NORMFN[normname], dropzerovardims=True, verbose=0)
    a = compose.compose(paths, fids, str(tmp_path / 'a') + '/*.cmp', **kw)
    b = compose.compose(paths, fids, str(tmp_path / 'b') + '/*.cmp', **kw)
    assert a['resident'] and b['resident']
    assert_same_files(str(tmp_path / 'a'), str(tmp_path / 'b'), 'two resident runs')
    monkeypatch.setattr(compose, 'DEVICE_CAP_BYTES', 140 * W * 4)           # chunks of a few files: [3,70] [130,5] [257*] [64,33,4] ...
    with _hip.KernelTimer() as kt:
        c = compose.compose(paths, fids, str(tmp_path / 'c') + '/*.cmp', **kw)
    assert not c['resident']
    assert len([r for r in kt.records if r[0] == 'ptts_compose_windows']) >= 4
    assert_same_files(str(tmp_path / 'a'), str(tmp_path / 'c'), 'resident vs streamed')
    for k in ('mean', 'std', 'sqdev'):
        np.testing.assert_array_equal(a[k], c[k])
    monkeypatch.setattr(compose, 'DEVICE_CAP_BYTES', 8 << 30)
    monkeypatch.setattr(compose, 'CHUNK_BYTES', 300 * W * 4)                # resident, but staged in several chunks
    d = compose.compose(paths, fids, str(tmp_path / 'd') + '/*.cmp', **kw)
    assert d['resident']
    assert_same_files(str(tmp_path / 'a'), str(tmp_path / 'd'), 'one chunk vs several')


@pytest.mark.gpu
def test_ops_wrappers_validate_on_device():
    import torch
    y = torch.zeros(10, 4, device='cuda')
    offs = torch.tensor([0, 4, 10], dtype=torch.int32, device='cuda')
    stats = ops.compose_stats_buffers(12, 'cuda')
    out = ops.compose_windows(y, offs, REF_WINS, stats=stats, n_stat_utts=5)            # n_stat_utts is capped at N
    assert out.shape == (10, 12) and float(stats[2].abs().max()) == 0.0
    with pytest.raises(ValueError):
        ops.compose_windows(y, offs, REF_WINS, n_stat_utts=1)                           # statistics without buffers
    with pytest.raises(ValueError):
        ops.compose_windows(y, offs, REF_WINS, stats=ops.compose_stats_buffers(8, 'cuda'), n_stat_utts=1)
    with pytest.raises(ValueError):
        ops.compose_windows(y.view(-1), offs, REF_WINS)
    with pytest.raises(_hip.HipLibraryError):
        ops.compose_windows(y, offs.long(), REF_WINS)
    with pytest.raises(_hip.HipLibraryError):
        ops.compose_windows(y.cpu(), offs, REF_WINS)
    mean = torch.zeros(12, dtype=torch.float64, device='cuda')
    with pytest.raises(_hip.HipLibraryError):
        ops.compose_sqdev(out, offs, mean.float(), mean.clone(), 2)
    with pytest.raises(ValueError):
        ops.compose_sqdev(out, offs, mean[:5].contiguous(), mean.clone(), 2)
    a = torch.ones(12, device='cuda')
    with pytest.raises(ValueError):
        ops.compose_normalise(out, a, a, mode=5)
    with pytest.raises(ValueError):
        ops.compose_normalise(out, a[:3].contiguous(), a)
    kidx = torch.arange(12, dtype=torch.int32, device='cuda')
    with pytest.raises(ValueError):
        ops.compose_normalise(out, a, a, keepidx=kidx, out=out)                         # a gather in place
    # K = 1: a copy plus statistics (the label side)
    yl = torch.rand(10, 4, device='cuda')
    st = ops.compose_stats_buffers(4, 'cuda')
    cp = ops.compose_windows(yl, offs, None, stats=st, n_stat_utts=1)
    assert torch.equal(cp, yl) and torch.equal(st[0], yl[:4].min(0).values) and torch.equal(st[1], yl[:4].max(0).values)


# ---- closing the loop: compose -> files -> ops.mlpg ----------------------------------------------------------------------
def _mlpg_banded(mu, var, wins):
    """mu, var [T,K] fp64 of one feature -> c [T]: P = sum_k W_k^T diag(1/var_k) W_k, b = sum_k W_k^T (mu_k/var_k), the delta
    streams' variance 1e11 at both ends (mlpg_fast.py:95-135; the banded solve of tests/test_mlpg.py for one system)."""
    T, K = mu.shape
    var = np.array(var, dtype=np.float64)
    var[0, 1:] = var[-1, 1:] = 1e11
    tau, bf = 1.0 / var, mu / var
    ab, b = np.zeros((3, T)), np.zeros(T)
    ab[0] += tau[:, 0]
    b += bf[:, 0]
    for k in range(1, K):
        w = [float(c) for c in wins[k - 1]]
        for j1 in (-1, 0, 1):
            t = np.arange(max(0, -j1), min(T, T - j1))
            b[t + j1] += w[j1 + 1] * bf[t, k]
            for j2 in (-1, 0, 1):
                if j1 < j2: continue
                t = np.arange(max(0, -j2), min(T, T - j1))
                ab[j1 - j2, t + j2] += tau[t, k] * w[j1 + 1] * w[j2 + 1]
    return scipy.linalg.solveh_banded(ab, b, lower=True)


def _round_trip(cmp_dir, fids, D, dev):
    """Normalised composed files + mean4norm / std4norm -> the static trajectories [(T,D)]: on the device through ops.mlpg, or in
    the fp64 restatement."""
    mean, std = f32file(cmp_dir + '/mean4norm.dat'), f32file(cmp_dir + '/std4norm.dat')
    outs = []
    for fid in fids:
        y = f32file(cmp_dir + '/' + fid + '.cmp', 3 * D)
        if dev:
            import torch
            t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
            outs.append(ops.mlpg(t(y), REF_WINS, t(std * std), mean=t(mean), std=t(std)).cpu().numpy().astype(np.float64))
        else:
            mu = (y.astype(np.float64) * std + mean).reshape(-1, 3, D)
            var = np.tile((std * std).astype(np.float64), (y.shape[0], 1)).reshape(-1, 3, D)
            outs.append(np.stack([_mlpg_banded(mu[:, :, d], var[:, :, d], REF_WINS) for d in range(D)], axis=1))
    return outs


@pytest.mark.gpu
def test_closing_the_loop_through_mlpg(tmp_path):
    """compose(win_convention='mlpg', both reference windows, normalise_meanstd) -> ops.mlpg(var = std^2) gives back the raw
    static features.  Tolerance per column: the error of the same round trip in the fp64 restatement (restated compose + banded
    solve, from the fp32 files it writes) + 2^-23 max|column|, the TOL rule of tests/test_mlpg.py.  The restatement's own error
    is the fp32 rounding of the normalised files seen through the solve; measured on this input (the test prints it): at most
    9.5e-8 of max|column|; the device's round trip came to 0.49 of the tolerance in its worst element.  With
    win_convention='reference' the acceleration stream is the negative of what MLPG assumes and the same round trip misses that
    tolerance by orders of magnitude (measured: 4.2e6 times the tolerance)."""
    fids, paths = make_corpus(tmp_path, lens=[40, 3, 150, 77, 9], nstat=5, dead=False, spec=20, nm=4)
    D = 25
    raws = [_read_streams(paths, fid).astype(np.float64) for fid in fids]
    ref_compose(paths, fids, str(tmp_path / 'ref') + '/*.cmp', wins=REF_WINS, id_valid_start=5, normfn=ref_normalise_meanstd, convention='mlpg')
    want_err = [np.abs(c - r).max(axis=0) for c, r in zip(_round_trip(str(tmp_path / 'ref'), fids, D, dev=False), raws)]
    for conv in ('mlpg', 'reference'):
        d = str(tmp_path / conv)
        compose.compose(paths, fids, d + '/*.cmp', wins=REF_WINS, id_valid_start=5, normfn=compose.normalise_meanstd,
                        win_convention=conv, verbose=0)
        gots = _round_trip(d, fids, D, dev=True)
        worst = 0.0
        for got, raw, e_ref, fid in zip(gots, raws, want_err, fids):
            scale = np.abs(raw).max(axis=0)
            tol = e_ref + 2.0 ** -23 * scale
            err = np.abs(got - raw).max(axis=0)
            worst = max(worst, (err / tol).max())
            if conv == 'mlpg':
                assert (np.abs(got - raw) <= tol).all(), (fid, (err / tol).max())
        print("win_convention={!r}: worst round-trip error / tolerance = {:.3e}; restatement's own error up to {:.3e} of max|column|".format(
            conv, worst, max((e / np.abs(r).max(axis=0)).max() for e, r in zip(want_err, raws))))
        if conv == 'reference':
            assert worst > 1e3


# ---- downstream -----------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_generate_params_and_data_load_accept_what_compose_wrote(tmp_path):
    import percivaltts_amd
    from percivaltts_amd import modeltts_common, vocoders
    voc = vocoders.VocoderPML(16000, 0.005, 12, 4, mlpg_wins=REF_WINS)
    lens = [30, 12, 25, 18]
    fids, paths = make_corpus(tmp_path, lens=lens, nstat=4, dead=False, spec=12, nm=4)
    cmp_dir = str(tmp_path / 'cmp')
    outpath = cmp_dir + '/*.cmp:(-1,{})'.format(voc.featuressize())
    compose.compose(paths, fids, outpath, wins=voc.mlpg_wins, id_valid_start=3, normfn=compose.normalise_meanstd_nmnoscale,
                    win_convention='mlpg', verbose=0)
    assert f32file(cmp_dir + '/mean4norm.dat').shape == f32file(cmp_dir + '/std4norm.dat').shape == (voc.featuressize(),)
    Y = data.load(outpath, fids)
    assert [y.shape for y in Y] == [(n, voc.featuressize()) for n in lens]
    ctx = 19
    rng = np.random.RandomState(0)
    os.makedirs(str(tmp_path / 'lab'))
    for fid, n in zip(fids, lens):
        (rng.rand(n, ctx) * 2 - 1).astype(np.float32).tofile(str(tmp_path / 'lab' / (fid + '.lab')))
    compose.compose([str(tmp_path / 'lab') + '/*.lab:(-1,{})'.format(ctx)], fids, str(tmp_path / 'labn') + '/*.lab:(-1,{})'.format(ctx),
                    id_valid_start=3, normfn=compose.normalise_minmax, wins=[], verbose=0)
    inpath = str(tmp_path / 'labn') + '/*.lab:(-1,{})'.format(ctx)
    X = data.load(inpath, fids)
    assert [x.shape for x in X] == [(n, ctx) for n in lens] and min(x.min() for x in X[:3]) == -1.0 and max(x.max() for x in X[:3]) == 1.0
    cfg = percivaltts_amd.configuration()
    cfg.arch_hiddenwidth = 8; cfg.train_batch_size = 2
    cfg.arch_ctx_nbcnnlayers = 1; cfg.arch_ctx_winlen = 5
    cfg.arch_gen_nbcnnlayers = 2; cfg.arch_gen_nbfilters = 2; cfg.arch_gen_winlen = 3; cfg.arch_spec_freqlen = 3
    mod = modeltts_common.Generic(ctx, voc, layertypes=['FC', 'BLSTM'], cfgarch=cfg)
    stats = mod.generate_params(inpath, outpath, fids, str(tmp_path / 'gen'), do_objmeas=True, batch_size=2)
    assert np.isfinite(list(stats.values())).all()
    for fid, n in zip(fids, lens):
        got = f32file(str(tmp_path / 'gen' / (fid + '.cmp')), voc.featuressizeraw())
        assert got.shape == (n, voc.featuressizeraw()) and np.isfinite(got).all()
