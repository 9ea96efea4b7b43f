"""Parameter generation: MLPG (csrc/mlpg.hip, ops.mlpg), ModelTTS.denormalise / generate_params, the vocoders' objective measures.

The reference (modeltts.py:163-179 -> external/merlin/mlpg_fast.py:95-135, vocoders.py:112-117,209-218,333-342) cannot run here
(Python 2, TF 1.9, `bandmat`), so parity is by restatement of its formulas in fp64.  For one utterance of T frames and one raw
feature, with K = 1 + number of windows streams:

    var[0,k] = var[T-1,k] = 1e11 for k >= 1;  W_0 = I;  W_k[t,t+j] = win_k[j+1], j in {-1,0,1}, taps outside [0,T) dropped
    P = sum_k W_k^T diag(1/var[:,k]) W_k,   b = sum_k W_k^T (mu[:,k] / var[:,k]),   c = P^-1 b

`mlpg_banded` builds P in band storage and solves with scipy.linalg.solveh_banded; `mlpg_dense` builds explicit W_k matrices and
solves with numpy.linalg.solve, and guards the former.

Tolerance of the device solve, derived and not tuned: |got - want| <= 2^-23 max_t |want[:, system]| for EVERY element: one fp32
rounding of the result (2^-24) and as much again for the fp64 solve's own error, which at the condition numbers of these inputs
(<= ~2e7) is three orders smaller."""
import ctypes
import os

import numpy as np
import pytest
import scipy.linalg

REF_WINS = [[-0.5, 0.0, 0.5], [1.0, -2.0, 1.0]]
CUSTOM_WINS = [[-0.7, 0.1, 0.4], [0.9, -2.1, 1.3]]         # asymmetric
EDGE_VAR = 100000000000.0
TOL = 2.0 ** -23


# ---------------------------------------------------------------------------------------------------------------------------
# the restatement
# ---------------------------------------------------------------------------------------------------------------------------
def _edge_rule(var):
    """var [T,K,...] (a copy): the delta streams' variance at the first and last frame is 1e11 (mlpg_fast.py:122-125)."""
    var = np.array(var, dtype=np.float64)
    var[0, 1:] = EDGE_VAR
    var[-1, 1:] = EDGE_VAR
    return var


def mlpg_banded(mu, var, wins):
    """mu, var [T,K,S] float64 (S independent systems) -> c [T,S]."""
    mu = np.asarray(mu, dtype=np.float64)
    T, K, S = mu.shape
    assert K == 1 + len(wins)
    var = _edge_rule(var)
    tau, bf = 1.0 / var, mu / var
    ab = np.zeros((3, T, S))            # lower band storage: ab[i - j, j] = P[i, j]
    b = np.zeros((T, S))
    ab[0] += tau[:, 0]
    b += bf[:, 0]
    for k in range(1, K):
        w = [float(c) for c in wins[k - 1]]
        for j1 in (-1, 0, 1):
            # row t of W_k has w[j+1] at column t+j
            t = np.arange(max(0, -j1), min(T, T - j1))
            if len(t): b[t + j1] += w[j1 + 1] * bf[t, k]
            for j2 in (-1, 0, 1):
                if j1 < j2: continue
                t = np.arange(max(0, -j2), min(T, T - j1))
                if len(t): ab[j1 - j2, t + j2] += tau[t, k] * w[j1 + 1] * w[j2 + 1]
    c = np.empty((T, S))
    for s in range(S):
        c[:, s] = scipy.linalg.solveh_banded(ab[:min(3, T), :, s], b[:, s], lower=True)
    return c


def mlpg_dense(mu, var, wins):
    mu = np.asarray(mu, dtype=np.float64)
    T, K, S = mu.shape
    var = _edge_rule(var)
    Ws = [np.eye(T)]
    for w in wins:
        W = np.zeros((T, T))
        for t in range(T):
            for j in (-1, 0, 1):
                if 0 <= t + j < T: W[t, t + j] = w[j + 1]
        Ws.append(W)
    c = np.empty((T, S))
    cond = 0.0
    for s in range(S):
        P = sum(Ws[k].T @ np.diag(1.0 / var[:, k, s]) @ Ws[k] for k in range(K))
        b = sum(Ws[k].T @ (mu[:, k, s] / var[:, k, s]) for k in range(K))
        c[:, s] = np.linalg.solve(P, b)
        cond = max(cond, np.linalg.cond(P))
    return c, cond


def ldl_sweep(mu, var, wins, dtype):
    """The kernel's algorithm (an LDL^T sweep that forms the band rows on the fly), every operation in `dtype`.
    mu, var [T,K,S] -> c [T,S] in `dtype`."""
    T, K, S = mu.shape
    var = _edge_rule(var).astype(dtype)
    mu = np.asarray(mu).astype(dtype)
    one = dtype(1.0)
    p = one / var
    r = mu * p
    z0 = np.zeros((1, K, S), dtype=dtype)
    p, r = np.concatenate([z0, p, z0]), np.concatenate([z0, r, z0])       # frame t at index t + 1
    w = np.asarray(wins, dtype=dtype)
    q, l1s, l2s = (np.zeros((T, S), dtype=dtype) for _ in range(3))
    l1p = invd1 = invd2 = z1 = z2 = np.zeros(S, dtype=dtype)
    for i in range(T):
        pp, pc, pn, rp, rc, rn = p[i], p[i + 1], p[i + 2], r[i], r[i + 1], r[i + 2]
        a, e1, e2, bb = pc[0].copy(), np.zeros(S, dtype=dtype), np.zeros(S, dtype=dtype), rc[0].copy()
        for k in range(1, K):
            w0, w1, w2 = w[k - 1]
            a = a + (w2 * w2 * pp[k] + w1 * w1 * pc[k] + w0 * w0 * pn[k])
            e1 = e1 + (w1 * w2 * pp[k] + w0 * w1 * pc[k])
            e2 = e2 + w0 * w2 * pp[k]
            bb = bb + (w2 * rp[k] + w1 * rc[k] + w0 * rn[k])
        if i < 1: e1 = e1 * dtype(0)
        if i < 2: e2 = e2 * dtype(0)
        f1 = e1 - e2 * l1p
        l1, l2 = f1 * invd1, e2 * invd2
        d = a - l2 * e2 - l1 * f1
        invd = one / d
        z = bb - l1 * z1 - l2 * z2
        q[i], l1s[i], l2s[i] = z * invd, l1, l2
        l1p, invd2, invd1, z2, z1 = l1, invd1, invd, z1, z
    c = np.zeros((T, S), dtype=dtype)
    for i in range(T - 1, -1, -1):
        c[i] = q[i]
        if i + 1 < T: c[i] = c[i] - l1s[i + 1] * c[i + 1]
        if i + 2 < T: c[i] = c[i] - l2s[i + 2] * c[i + 2]
    assert c.dtype == dtype
    return c


def make_inputs(seed, B, T, D, wins, pow2_stats=False):
    """Normalised network-like output y [B,T,K*D] float32 with its statistics mean, std [K*D] float32: a random walk plus noise
    for the statics, its numerical derivative (the windows applied to the walk) plus noise for the deltas; per-stream standard
    deviations log-uniform in [1e-2, 10].  `pow2_stats`: std a power of two in that range and mean 0, so that y*std + mean is
    exact in fp32."""
    rng = np.random.RandomState(seed)
    K = 1 + len(wins)
    walk = np.cumsum(rng.randn(B, T, D), axis=1) * 0.3
    pad = np.pad(walk, ((0, 0), (1, 1), (0, 0)))
    y = np.empty((B, T, K * D))
    y[..., :D] = walk + 0.1 * rng.randn(B, T, D)
    for k, w in enumerate(wins):
        y[..., (k + 1) * D:(k + 2) * D] = w[0] * pad[:, :-2] + w[1] * pad[:, 1:-1] + w[2] * pad[:, 2:] + 0.1 * rng.randn(B, T, D)
    if pow2_stats:
        std = 2.0 ** rng.randint(-6, 4, size=K * D)
        mean = np.zeros(K * D)
    else:
        std = np.exp(rng.uniform(np.log(1e-2), np.log(10.0), size=K * D))
        mean = rng.randn(K * D) * std
    return y.astype(np.float32), mean.astype(np.float32), std.astype(np.float32)


def as_systems(a, K):
    """[T,K*D] -> [T,K,D]"""
    return np.asarray(a, dtype=np.float64).reshape(a.shape[0], K, -1)


def want_for(y, mean, std, var, wins, lengths=None):
    """The restatement for a batch: y [B,T,K*D] fp32, mean/std [K*D] fp32 or None, var [K*D] or [B,T,K*D] fp32 -> [B,T,D] fp64,
    zeros behind each utterance's end.  De-normalisation and solve in fp64, starting from the fp32 numbers: the C ABI takes the
    window taps as fp32 like every other operand, so they are rounded to fp32 here too (the reference's taps are exact)."""
    wins = [[float(np.float32(c)) for c in w] for w in wins]
    B, T, KD = y.shape
    K = 1 + len(wins)
    D = KD // K
    out = np.zeros((B, T, D))
    for b in range(B):
        L = T if lengths is None else int(lengths[b])
        mu = y[b, :L].astype(np.float64)
        if mean is not None:
            mu = mu * std.astype(np.float64) + mean.astype(np.float64)
        v = var[b, :L] if var.ndim == 3 else np.tile(var, (L, 1))
        out[b, :L] = mlpg_banded(as_systems(mu, K), as_systems(v, K), wins)
    return out


def check_tol(got, want, what, lengths=None):
    """Every element: |got - want| <= 2^-23 max_t |want[:, system]|; prints the worst ratio before asserting."""
    got = np.asarray(got, dtype=np.float64)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    scale = np.abs(want).max(axis=1, keepdims=True)
    err = np.abs(got - want)
    ratio = (err / np.where(scale > 0, scale, 1.0)).max()
    print('{}: worst |got-want| / max_t|want| = {:.3e} (bound {:.3e})'.format(what, ratio, TOL))
    assert np.isfinite(got).all(), what
    assert (err <= TOL * scale).all(), (what, ratio)
    if lengths is not None:
        for b, L in enumerate(lengths):
            assert (got[b, int(L):] == 0).all(), (what, b)


# ---------------------------------------------------------------------------------------------------------------------------
# CPU
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('T', [1, 2, 3, 5, 40])
@pytest.mark.parametrize('wins', [REF_WINS, REF_WINS[:1], CUSTOM_WINS, CUSTOM_WINS[1:]], ids=['ref3', 'ref2', 'custom3', 'custom2'])
def test_banded_restatement_equals_dense(T, wins):
    K = 1 + len(wins)
    worst, worst_cond = 0.0, 0.0
    for seed in range(6):
        y, mean, std = make_inputs(100 + seed, 1, T, 50, wins)
        mu = as_systems(y[0].astype(np.float64) * std + mean, K)
        var = as_systems(np.tile(std.astype(np.float64) ** 2, (T, 1)), K)
        cb = mlpg_banded(mu, var, wins)
        cd, cond = mlpg_dense(mu, var, wins)
        rel = (np.abs(cb - cd) / np.abs(cd).max(axis=0, keepdims=True)).max()
        worst, worst_cond = max(worst, rel), max(worst_cond, cond)
    print('T={} K={}: banded vs dense {:.3e}, cond(P) up to {:.3e}'.format(T, K, worst, worst_cond))
    assert worst <= 2.0 ** -30


def test_edge_variance_rule_is_visible():
    """With a huge static variance at both ends, the end values follow the interior (through the deltas, whose own end variance
    is 1e11, the trajectory is extrapolated), not mu."""
    T = 12
    mu = np.zeros((T, 3, 1))
    mu[:, 0, 0] = 1.0
    mu[0, 0, 0] = mu[-1, 0, 0] = 50.0
    var = np.ones((T, 3, 1))
    var[0, 0, 0] = var[-1, 0, 0] = 1e9
    c = mlpg_banded(mu, var, REF_WINS)[:, 0]
    assert abs(c[0] - 1.0) < 1e-3 and abs(c[-1] - 1.0) < 1e-3, c
    # and the delta streams' means at the ends are ignored: a wild delta mean at frame 0 changes nothing
    mu2 = mu.copy()
    mu2[0, 1:, 0] = 1e3
    np.testing.assert_allclose(mlpg_banded(mu2, var, REF_WINS)[:, 0], c, rtol=0, atol=1e-6)
    # T = 1: both rules hit frame 0, the static stream decides
    c1 = mlpg_banded(np.array([[[3.0], [7.0], [9.0]]]), np.ones((1, 3, 1)), REF_WINS)
    assert abs(c1[0, 0] - 3.0) < 1e-9


GPU_CASE = dict(seed=7, B=1, T=400, D=163)          # one of the GPU test's input sets (test_kernel_against_restatement)


def test_fp64_sweep_passes_and_fp32_sweep_misses_the_gpu_tolerance():
    """Why the kernel is fp64.  The kernel's LDL^T sweep restated in numpy: in fp64 it meets the GPU test's tolerance before the
    final rounding with orders to spare; the SAME sweep in fp32 misses it in its worst system by orders of magnitude, although
    individual well-conditioned systems pass.  Measured (seed 7, T = 400, D = 163, reference windows): fp64 worst 6.2e-11 of
    max|c|; fp32 worst 1.5e-2, five orders beyond 2^-23, best 1.1e-7, 5 of 163 systems within the bound.  The fp64 bound here is
    2^-23 / 100: what the sweep may add to the 2^-24 of the result's rounding without touching the tolerance."""
    y, mean, std = make_inputs(GPU_CASE['seed'], GPU_CASE['B'], GPU_CASE['T'], GPU_CASE['D'], REF_WINS)
    mu = as_systems(y[0].astype(np.float64) * std + mean, 3)
    var = as_systems(np.tile((std * std), (GPU_CASE['T'], 1)), 3)
    want = mlpg_banded(mu, var, REF_WINS)
    scale = np.abs(want).max(axis=0)
    e64 = (np.abs(ldl_sweep(mu, var, REF_WINS, np.float64) - want).max(axis=0) / scale)
    e32 = (np.abs(ldl_sweep(mu, var, REF_WINS, np.float32).astype(np.float64) - want).max(axis=0) / scale)
    print('fp64 sweep worst {:.3e}; fp32 sweep worst {:.3e}, best {:.3e}, systems within 2^-23: {} of {}'.format(
        e64.max(), e32.max(), e32.min(), int((e32 <= TOL).sum()), e32.size))
    assert e64.max() <= TOL / 100
    assert e32.max() >= 100 * TOL


def test_entry_points_reject_bad_arguments():
    """PTTS_EINVAL / PTTS_EWORKSPACE before any launch (no pointer is dereferenced on the host before the checks pass)."""
    from percivaltts_amd import _hip
    if not os.path.exists(_hip.LIB_PATH):
        pytest.skip('libpercival_hip.so not built (run __graft_entry__.build())')
    lib = _hip.lib()
    p = ctypes.c_void_p(256)           # non-null, never read
    EINVAL, EWORKSPACE = -1, -3
    big = 1 << 40
    go = lambda y=p, mean=None, std=None, var=p, pf=0, wins=p, lens=None, out=p, ws=p, nws=big, B=2, T=5, D=4, K=3: \
        lib.ptts_mlpg(y, mean, std, var, pf, wins, lens, out, ws, nws, B, T, D, K, None)
    for kw in (dict(y=None), dict(var=None), dict(wins=None), dict(out=None), dict(B=0), dict(T=0), dict(D=0), dict(B=-1),
               dict(K=1), dict(K=4), dict(K=0), dict(mean=p), dict(std=p)):
        assert go(**kw) == EINVAL, kw
    assert 'mlpg' in _hip.last_error()
    need = lib.ptts_mlpg_workspace_bytes(2, 5, 4)
    assert need >= 2 * 5 * 4 * 24
    assert lib.ptts_mlpg_workspace_bytes(64, 2000, 163) >= 64 * 2000 * 163 * 24        # beyond 32 bits
    assert go(nws=need - 1) == EWORKSPACE
    assert go(ws=None, nws=need) == EWORKSPACE
    assert 'workspace' in _hip.last_error()


def test_header_declares_and_library_exports_the_symbols():
    from percivaltts_amd import _hip
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, 'include', 'percival_hip.h')) as f:
        header = f.read()
    assert 'size_t ptts_mlpg_workspace_bytes(int B, int T, int D);' in header
    assert 'int ptts_mlpg(const float* y' in header
    assert 'ptts_mlpg' in _hip.SIGNATURES and 'ptts_mlpg_workspace_bytes' in _hip.SIGNATURES
    if not os.path.exists(_hip.LIB_PATH):
        pytest.skip('libpercival_hip.so not built (run __graft_entry__.build())')
    lib = ctypes.CDLL(_hip.LIB_PATH)
    assert hasattr(lib, 'ptts_mlpg') and hasattr(lib, 'ptts_mlpg_workspace_bytes')


def test_objective_measures_hand_computed():
    from percivaltts_amd import vocoders
    pml = vocoders.VocoderPML(16000, 0.005, 2, 1)
    wld = vocoders.VocoderWORLD(16000, 0.005, 2, 1)
    assert pml.features_err is not wld.features_err
    # two frames: f0 | spec(2) | nm or aper (1) [| vuv]
    ref = np.array([[np.log(100.0), 0.0, 1.0, 0.5, 1.0], [np.log(200.0), 1.0, 1.0, 0.25, 0.0]])
    gen = np.array([[np.log(103.0), 0.5, 1.0, 0.0, 1.0], [np.log(196.0), 1.0, 3.0, 0.25, 0.0]])
    db = 20.0 / np.log(10.0)
    for voc, key in ((pml, 'NM'), (wld, 'APER[dB]')):
        voc.objmeasures_add(gen, ref)
        e = voc.features_err
        assert sorted(e) == sorted(['F0[Hz]', 'SPEC[dB]', key])
        np.testing.assert_allclose(e['F0[Hz]'][0], np.sqrt((9.0 + 16.0) / 2), rtol=1e-12)
        np.testing.assert_allclose(e['SPEC[dB]'][0], [db * np.sqrt(0.25 / 2), db * np.sqrt(4.0 / 2)], rtol=1e-12)
        np.testing.assert_allclose(e[key][0], [np.sqrt(0.25 / 2)], rtol=1e-12)
        voc.objmeasures_add(ref, ref)
        stats = voc.objmeasures_stats()
        np.testing.assert_allclose(stats['F0[Hz]'], np.sqrt(12.5) / 2, rtol=1e-12)
        np.testing.assert_allclose(stats['SPEC[dB]'], db * (np.sqrt(0.125) + np.sqrt(2.0)) / 4, rtol=1e-12)
        np.testing.assert_allclose(stats[key], np.sqrt(0.125) / 2, rtol=1e-12)
    pml.objmeasures_clear()
    assert pml.features_err == {} and len(wld.features_err['F0[Hz]']) == 2          # not shared
    assert pml.objmeasures_stats() == {}
    with pytest.raises(NotImplementedError):
        pml.synthesis(None)


def test_objective_measures_stats_prints_the_reference_lines(capsys):
    from percivaltts_amd import vocoders
    voc = vocoders.VocoderPML(16000, 0.005, 2, 1)
    x = np.zeros((3, 4))
    voc.objmeasures_add(x, x + 1.0)
    capsys.readouterr()
    stats = voc.objmeasures_stats()
    lines = capsys.readouterr().out.strip().splitlines()
    assert sorted(lines) == sorted('{}: {}'.format(k, v) for k, v in stats.items())


def _cpu_model(voc):
    from percivaltts_amd import modeltts
    return modeltts.ModelTTS(5, voc)


def test_denormalise_on_the_host():
    from percivaltts_amd import vocoders
    rng = np.random.RandomState(0)
    # no windows: width unchanged
    voc = vocoders.VocoderPML(16000, 0.005, 3, 2)
    cmp_, mean, std = rng.randn(7, 6).astype(np.float32), rng.randn(6).astype(np.float32), (rng.rand(6) + 0.5).astype(np.float32)
    out = _cpu_model(voc).denormalise(cmp_, mean, std)
    np.testing.assert_array_equal(out, cmp_ * std + mean)
    np.testing.assert_array_equal(_cpu_model(voc).denormalise(cmp_, mean, std, mlpg_ignore=True), cmp_ * std + mean)
    # windows + mlpg_ignore: the static columns
    for voc in (vocoders.VocoderPML(16000, 0.005, 3, 2, mlpg_wins=REF_WINS), vocoders.VocoderWORLD(16000, 0.005, 3, 1, mlpg_wins=REF_WINS)):
        cmp_, mean, std = rng.randn(7, 18).astype(np.float32), rng.randn(18).astype(np.float32), (rng.rand(18) + 0.5).astype(np.float32)
        out = _cpu_model(voc).denormalise(cmp_, mean, std, mlpg_ignore=True)
        assert out.shape == (7, 6) and out.dtype == np.float32
        np.testing.assert_array_equal(out, (cmp_ * std + mean)[:, :6])
    with pytest.raises(ValueError):
        _cpu_model(voc).denormalise(cmp_[:, :6], mean, std, mlpg_ignore=True)       # wrong width


@pytest.mark.parametrize('wins', [[[1.0]], [[-0.5, 0.0, 0.5], [1.0]], [REF_WINS[0]] * 4, [REF_WINS[0]] * 3, []],
                         ids=['one-tap', 'second-one-tap', 'four-windows', 'three-windows', 'empty'])
def test_windows_mlpg_cannot_use_are_a_value_error(wins):
    from percivaltts_amd import ops, vocoders
    with pytest.raises(ValueError):
        ops.mlpg_windows(wins)
    if len(wins) == 0:
        return              # an empty list means "no MLPG" to the vocoder and to denormalise, as in the reference
    voc = vocoders.VocoderPML(16000, 0.005, 3, 2, mlpg_wins=wins)
    n = voc.featuressize()
    with pytest.raises(ValueError):
        _cpu_model(voc).denormalise(np.zeros((4, n), np.float32), np.zeros(n, np.float32), np.ones(n, np.float32), mlpg_ignore=True)
    with pytest.raises(ValueError):
        _cpu_model(voc).denormalise(np.zeros((4, n), np.float32), np.zeros(n, np.float32), np.ones(n, np.float32))


def test_ops_mlpg_needs_device_tensors():
    import torch
    from percivaltts_amd import _hip, ops
    y, var = torch.zeros(2, 4, 6), torch.ones(6)
    with pytest.raises(_hip.HipLibraryError):
        ops.mlpg(y, REF_WINS, var)
    with pytest.raises(ValueError):
        ops.mlpg(y.requires_grad_(True), REF_WINS, var)


# ---------------------------------------------------------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------------------------------------------------------
def _dev(a, dtype=None):
    import torch
    t = torch.from_numpy(np.ascontiguousarray(a))
    return (t.to(dtype) if dtype is not None else t).cuda()


def _run(y, mean, std, var, wins, lengths=None):
    from percivaltts_amd import ops
    out = ops.mlpg(_dev(y), wins, _dev(var), mean=None if mean is None else _dev(mean), std=None if std is None else _dev(std),
                   lengths=None if lengths is None else _dev(np.asarray(lengths, dtype=np.int32)))
    return out.cpu().numpy()


KERNEL_CASES = [
    # (seed, B, T, D, wins)
    (1, 3, 1, 5, REF_WINS), (2, 3, 2, 5, REF_WINS), (3, 3, 3, 5, REF_WINS), (4, 3, 5, 5, REF_WINS),
    (5, 2, 37, 1, REF_WINS), (6, 2, 37, 63, REF_WINS), (8, 2, 37, 64, REF_WINS), (9, 2, 37, 65, REF_WINS),
    (GPU_CASE['seed'], GPU_CASE['B'], GPU_CASE['T'], GPU_CASE['D'], REF_WINS),
    (10, 2, 3000, 7, REF_WINS),
    (11, 3, 50, 20, CUSTOM_WINS), (12, 3, 50, 20, REF_WINS[:1]), (13, 3, 5, 20, CUSTOM_WINS[1:]), (14, 2, 1, 3, REF_WINS[:1]),
]


@pytest.mark.gpu
@pytest.mark.parametrize('case', KERNEL_CASES, ids=lambda c: 's{}-B{}-T{}-D{}-K{}'.format(c[0], c[1], c[2], c[3], 1 + len(c[4])))
def test_kernel_against_restatement(case):
    """Fused mean/std with per-column variance, pre-denormalised input, and per-frame variance, each against the restatement on
    the numbers the kernel was given."""
    seed, B, T, D, wins = case
    y, mean, std = make_inputs(seed, B, T, D, wins)
    var = std * std                                                 # fp32, as denormalise forms it
    check_tol(_run(y, mean, std, var, wins), want_for(y, mean, std, var, wins), 'fused, per-column var')
    mu32 = (y.astype(np.float64) * std + mean).astype(np.float32)
    check_tol(_run(mu32, None, None, var, wins), want_for(mu32, None, None, var, wins), 'pre-denormalised, per-column var')
    rng = np.random.RandomState(seed + 1000)
    varf = (var[None, None, :] * rng.uniform(0.5, 2.0, size=y.shape)).astype(np.float32)
    check_tol(_run(y, mean, std, varf, wins), want_for(y, mean, std, varf, wins), 'fused, per-frame var')
    check_tol(_run(mu32, None, None, varf, wins), want_for(mu32, None, None, varf, wins), 'pre-denormalised, per-frame var')


@pytest.mark.gpu
def test_kernel_many_waves():
    """64 x 400 x 163: B*D fills many waves."""
    B, T, D = 64, 400, 163
    y, mean, std = make_inputs(21, B, T, D, REF_WINS)
    var = std * std
    check_tol(_run(y, mean, std, var, REF_WINS), want_for(y, mean, std, var, REF_WINS), '64x400x163')


@pytest.mark.gpu
@pytest.mark.parametrize('wins', [REF_WINS, REF_WINS[:1]], ids=['K3', 'K2'])
def test_fused_and_pre_denormalised_agree(wins):
    """With statistics for which y*std + mean is exact in fp32 (std a power of two, mean 0) both routes start from the same
    numbers: they agree with the restatement and with each other to the tolerance."""
    y, mean, std = make_inputs(31, 4, 120, 70, wins, pow2_stats=True)
    var = std * std
    mu32 = y * std + mean
    assert (mu32.astype(np.float64) == y.astype(np.float64) * std + mean).all()
    want = want_for(y, mean, std, var, wins)
    fused, pre = _run(y, mean, std, var, wins), _run(mu32, None, None, var, wins)
    check_tol(fused, want, 'fused')
    check_tol(pre, want, 'pre-denormalised')
    check_tol(fused, pre.astype(np.float64), 'fused vs pre-denormalised')


@pytest.mark.gpu
def test_ragged_lengths():
    """Each utterance is solved over its OWN length (var[len-1] = 1e11 at its own last frame), zeros behind its end, and what
    lies in the padding does not matter."""
    B, T, D = 6, 90, 65
    lengths = [90, 1, 2, 3, 57, 5]
    y, mean, std = make_inputs(41, B, T, D, REF_WINS)
    var = std * std
    want = want_for(y, mean, std, var, REF_WINS, lengths)
    got = _run(y, mean, std, var, REF_WINS, lengths)
    check_tol(got, want, 'ragged', lengths)
    # the own-last-frame rule is what makes the difference: solving the padded length and cropping is something else
    full = want_for(y, mean, std, var, REF_WINS)
    assert np.abs(full[4, :57] - want[4, :57]).max() > 100 * TOL * np.abs(want[4]).max()
    y2 = y.copy()
    for b, L in enumerate(lengths): y2[b, L:] = 1e6
    np.testing.assert_array_equal(_run(y2, mean, std, var, REF_WINS, lengths), got)
    # per-frame variance, ragged
    rng = np.random.RandomState(5)
    varf = (var[None, None, :] * rng.uniform(0.5, 2.0, size=y.shape)).astype(np.float32)
    check_tol(_run(y, mean, std, varf, REF_WINS, lengths), want_for(y, mean, std, varf, REF_WINS, lengths), 'ragged, per-frame var', lengths)
    # lengths outside [0, T] are clamped: nothing out of bounds, T frames solved / nothing solved
    odd = _run(y[:2], mean, std, var, REF_WINS, [T + 1000, -3])
    np.testing.assert_array_equal(odd[0], _run(y[:1], mean, std, var, REF_WINS)[0])
    assert (odd[1] == 0).all()


@pytest.mark.gpu
def test_batch_invariance_and_repeatability():
    B, T, D = 5, 130, 163
    y, mean, std = make_inputs(51, B, T, D, REF_WINS)
    var = std * std
    together = _run(y, mean, std, var, REF_WINS)
    np.testing.assert_array_equal(_run(y, mean, std, var, REF_WINS), together)                  # two runs
    for b in range(B):
        np.testing.assert_array_equal(_run(y[b:b + 1], mean, std, var, REF_WINS)[0], together[b])      # one by one
        np.testing.assert_array_equal(_run(y[b], mean, std, var, REF_WINS), together[b])               # [T,K*D] input
    order = [3, 0, 4, 2, 1]
    np.testing.assert_array_equal(_run(y[order], mean, std, var, REF_WINS), together[order])    # another order
    lengths = [130, 40, 7, 99, 1]
    ragged = _run(y, mean, std, var, REF_WINS, lengths)
    for b, L in enumerate(lengths):
        np.testing.assert_array_equal(ragged[b, :L], _run(y[b:b + 1, :L], mean, std, var, REF_WINS)[0])


@pytest.mark.gpu
def test_ops_mlpg_splits_a_batch_over_the_workspace_cap(monkeypatch):
    from percivaltts_amd import _hip, ops_offline
    B, T, D = 7, 60, 40
    y, mean, std = make_inputs(61, B, T, D, REF_WINS)
    var = std * std
    lengths = [60, 3, 44, 60, 1, 17, 30]
    with _hip.KernelTimer() as kt:
        whole = _run(y, mean, std, var, REF_WINS, lengths)
    assert [r[0] for r in kt.records] == ['ptts_mlpg']
    monkeypatch.setattr(ops_offline, 'MLPG_WORKSPACE_CAP', 2 * T * D * 24 + 256)            # room for two utterances
    with _hip.KernelTimer() as kt:
        split = _run(y, mean, std, var, REF_WINS, lengths)
    assert [r[1][0] for r in kt.records] == [2, 2, 2, 1]
    np.testing.assert_array_equal(split, whole)
    rng = np.random.RandomState(3)
    varf = (var[None, None, :] * rng.uniform(0.5, 2.0, size=y.shape)).astype(np.float32)
    split_f = _run(y, mean, std, varf, REF_WINS, lengths)
    monkeypatch.setattr(ops_offline, 'MLPG_WORKSPACE_CAP', 256 << 20)
    np.testing.assert_array_equal(split_f, _run(y, mean, std, varf, REF_WINS, lengths))


@pytest.mark.gpu
def test_ops_mlpg_validation_on_device():
    import torch
    from percivaltts_amd import _hip, ops
    y, var = torch.zeros(2, 4, 6, device='cuda'), torch.ones(6, device='cuda')
    with pytest.raises(ValueError):
        ops.mlpg(y, REF_WINS, var, mean=var)                        # mean without std
    with pytest.raises(ValueError):
        ops.mlpg(torch.zeros(2, 4, 7, device='cuda'), REF_WINS, torch.ones(7, device='cuda'))       # 7 is not 3*D
    with pytest.raises(ValueError):
        ops.mlpg(y, REF_WINS, torch.ones(5, device='cuda'))
    with pytest.raises(_hip.HipLibraryError):
        ops.mlpg(y, REF_WINS, var, lengths=torch.ones(2, dtype=torch.int64, device='cuda'))
    with pytest.raises(_hip.HipLibraryError):
        ops.mlpg(y, REF_WINS, var.cpu())


# ---- end to end ----------------------------------------------------------------------------------------------------------
def _small_cfg():
    import percivaltts_amd
    cfg = percivaltts_amd.configuration()
    cfg.arch_hiddenwidth = 8; cfg.train_batch_size = 2
    cfg.arch_ctx_nbcnnlayers = 1; cfg.arch_ctx_winlen = 5
    cfg.arch_gen_nbcnnlayers = 2; cfg.arch_gen_nbfilters = 2; cfg.arch_gen_winlen = 3; cfg.arch_spec_freqlen = 3
    return cfg


def _build(kind, wins):
    from percivaltts_amd import modeltts_common, vocoders
    ctx = 19
    if kind == 'dcnn-pml':
        voc = vocoders.VocoderPML(16000, 0.005, 12, 4, mlpg_wins=wins)
        return ctx, voc, modeltts_common.DCNNF0SpecNoiseFeatures(ctx, voc, _small_cfg())
    voc = (vocoders.VocoderPML(16000, 0.005, 12, 4, mlpg_wins=wins) if kind == 'generic-pml'
           else vocoders.VocoderWORLD(16000, 0.005, 12, 4, mlpg_wins=wins))
    return ctx, voc, modeltts_common.Generic(ctx, voc, layertypes=['FC', 'BLSTM'], cfgarch=_small_cfg())


def _corpus(tmp_path, ctx, voc, lens, seed=0):
    """Synthetic label / target files the way percivaltts_amd.run.synthesize_corpus makes them, with non-trivial statistics."""
    rng = np.random.RandomState(seed)
    nout = voc.featuressize()
    (tmp_path / 'lab').mkdir(); (tmp_path / 'cmp').mkdir()
    fids = ['utt_{:02d}'.format(i) for i in range(len(lens))]
    for fid, n in zip(fids, lens):
        (rng.rand(n, ctx) * 2 - 1).astype(np.float32).tofile(str(tmp_path / 'lab' / (fid + '.lab')))
        rng.randn(n + 3, nout).astype(np.float32).tofile(str(tmp_path / 'cmp' / (fid + '.cmp')))     # longer: croplen
    mean = (rng.randn(nout) * 0.3).astype(np.float32)
    mean[0] = 5.0                                               # log f0
    std = np.exp(rng.uniform(np.log(1e-2), np.log(10.0), size=nout)).astype(np.float32)
    std[0] = 0.2
    mean.tofile(str(tmp_path / 'cmp' / 'mean4norm.dat')); std.tofile(str(tmp_path / 'cmp' / 'std4norm.dat'))
    inpath = str(tmp_path / 'lab') + '/*.lab:(-1,{})'.format(ctx)
    outpath = str(tmp_path / 'cmp') + '/*.cmp:(-1,{})'.format(nout)
    return fids, inpath, outpath, mean, std


def _measures(voc_cls_args, gens, refs):
    """numpy's measures on what was written, through the formulas of the issue (not through the vocoder object)."""
    spec, nsz, key = voc_cls_args
    db = 20.0 / np.log(10.0)
    f0 = [np.sqrt(np.mean((np.exp(r[:, 0]) - np.exp(g[:, 0])) ** 2)) for g, r in zip(gens, refs)]
    sp = [np.sqrt(np.mean((db * r[:, 1:1 + spec] - db * g[:, 1:1 + spec]) ** 2, 0)) for g, r in zip(gens, refs)]
    nm = [np.sqrt(np.mean((r[:, 1 + spec:1 + spec + nsz] - g[:, 1 + spec:1 + spec + nsz]) ** 2, 0)) for g, r in zip(gens, refs)]
    return {'F0[Hz]': np.mean(f0), 'SPEC[dB]': np.mean(np.vstack(sp)), key: np.mean(np.vstack(nm))}


@pytest.mark.gpu
@pytest.mark.parametrize('kind', ['dcnn-pml', 'generic-pml', 'generic-world'])
def test_generate_params_end_to_end(kind, tmp_path):
    from percivaltts_amd import _hip, data
    ctx, voc, mod = _build(kind, REF_WINS)
    raw = voc.featuressizeraw()
    assert voc.featuressize() == 3 * raw and mod.kerasmodel.outputs[0].shape == (3 * raw,)
    lens = [41, 23, 60, 37, 9]
    fids, inpath, outpath, mean, std = _corpus(tmp_path, ctx, voc, lens)
    X = data.load(inpath, fids)

    with _hip.KernelTimer() as kt:
        stats = mod.generate_params(inpath, outpath, fids, str(tmp_path / 'gen'), do_objmeas=True, batch_size=3)
    launches = [r for r in kt.records if r[0] == 'ptts_mlpg']
    assert [r[1][0] for r in launches] == [3, 2]                 # two batched launches, nothing solved on the host

    gens, refs = [], []
    for fid, x, n in zip(fids, X, lens):
        got = np.fromfile(str(tmp_path / 'gen' / (fid + '.cmp')), dtype=np.float32).reshape(-1, raw)
        assert got.shape == (n, raw)
        y = mod.predict(x[None])                                # [1,T,3*raw] float32: what the solve was given
        want = want_for(y, mean, std, std * std, REF_WINS)[0]
        check_tol(got[None], want[None], '{} {}'.format(kind, fid))
        target = np.fromfile(str(tmp_path / 'cmp' / (fid + '.cmp')), dtype=np.float32).reshape(-1, 3 * raw)[:n]
        gens.append(got.astype(np.float64))
        refs.append((target * std + mean)[:, :raw].astype(np.float64))
        # denormalise() is the same solve for one utterance
        np.testing.assert_array_equal(mod.denormalise(y[0], mean, std), got)
    key = 'NM' if kind.endswith('pml') else 'APER[dB]'
    want_stats = _measures((12, 4, key), gens, refs)
    assert sorted(stats) == sorted(want_stats)
    for k in want_stats:
        np.testing.assert_allclose(stats[k], want_stats[k], rtol=1e-5, err_msg=k)

    # unbatched MLPG launches write identical files; no measures asked -> None
    with _hip.KernelTimer() as kt:
        assert mod.generate_params(inpath, outpath, fids, str(tmp_path / 'gen1'), do_objmeas=False, batch_size=1) is None
    assert [r[1][0] for r in kt.records if r[0] == 'ptts_mlpg'] == [1] * len(fids)
    for fid in fids:
        a = np.fromfile(str(tmp_path / 'gen' / (fid + '.cmp')), dtype=np.float32)
        b = np.fromfile(str(tmp_path / 'gen1' / (fid + '.cmp')), dtype=np.float32)
        np.testing.assert_array_equal(a, b)


@pytest.mark.gpu
@pytest.mark.parametrize('kind', ['dcnn-pml', 'generic-world'])
def test_generate_params_without_windows(kind, tmp_path):
    from percivaltts_amd import _hip, data
    ctx, voc, mod = _build(kind, None)
    raw = voc.featuressizeraw()
    lens = [30, 12]
    fids, inpath, outpath, mean, std = _corpus(tmp_path, ctx, voc, lens)
    X = data.load(inpath, fids)
    with _hip.KernelTimer() as kt:
        stats = mod.generate_params(inpath, outpath, fids, str(tmp_path / 'gen'))
    assert 'ptts_mlpg' not in [r[0] for r in kt.records]
    assert 'F0[Hz]' in stats and np.isfinite(list(stats.values())).all()
    for fid, x, n in zip(fids, X, lens):
        got = np.fromfile(str(tmp_path / 'gen' / (fid + '.cmp')), dtype=np.float32).reshape(-1, raw)
        assert got.shape == (n, raw)
        np.testing.assert_array_equal(got, mod.predict(x[None])[0] * std + mean)
    with pytest.raises(NotImplementedError):
        mod.generate_wav(inpath, outpath, fids, str(tmp_path / 'snd'))
