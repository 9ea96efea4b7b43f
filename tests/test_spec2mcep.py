"""Mel-cepstral compression of a spectral envelope (csrc/spectrum.hip ptts_spec2mcep / ptts_spec2mcep_table, ops.spec2mcep /
spec2mcep_check, VocoderF0Spec.compress_spectrum_device, VocoderPML.analysis_device with spec_type 'mcep', run.features_extraction).

The reference fits the mel-cepstrum with SPTK (vocoders.py:134-145, sp.spec2mcep), which is nowhere to be had; the definition is
the build's own and is restated here in numpy.  With L = dftlen, K = L/2 + 1, w_k = 2 pi k / L,
wt_k = w_k + 2 atan2(a sin w_k, 1 - a cos w_k), q_k the trapezoid weights of the nodes wt_k on [0, pi], C[m,k] = cos(m wt_k):

    v_k = ln max(|x_k|, FLT_MIN)  (or x_k, a logarithm already)
    c = argmin sum_k q_k (v_k - sum_m c_m C[m,k])^2 = W v,   W = G^-1 C diag(q),   G = C diag(q) C^T

The CPU tests check the restatement itself: that it inverts the decompression, that it is the reference's route (real cepstrum,
then SPTK's freqt, restated from its definition), and that G is well conditioned up to the order limit
floor((L/2) (1 - |a|) / (1 + |a|)).

Tolerance of the device results, the rule of tests/test_spectrum.py: the yardstick is the closed form in fp64 on the same fp32
input.  The same closed form is also evaluated with every array and intermediate in float32 (the table included), and its
largest error against fp64 is e32.  Every element of the kernel's result has to lie within 4 * e32 + one float32 ulp of the
value.  `check` prints e32 and the kernel's worst error before it asserts."""
import ctypes
import inspect
import os

import numpy as np
import pytest

EINVAL = -1
SPEC_TT = 8                     # frames of a workgroup (csrc/spectrum.hip)
SHIFT = 0.005
FLT_MIN = np.finfo(np.float32).tiny


def bark_alpha(fs):
    return 0.8517 * np.sqrt(np.arctan(0.06583 * fs / 1000.0)) - 0.1916


# (alpha, dftlen, M1): K = 5 leaves most lanes idle and M1 = 2 is the smallest order; M1 = 12 and 60 are no power of two;
# M1 = 257 takes a second row of workgroups (more than 256 coefficients) and K = 2049 nine chunks of bins, the last with one bin
SHAPES = [(0.3, 8, 2), (0.45, 64, 12), (0.58, 4096, 60), (0.58, 4096, 257)]
CPU_SHAPES = [(0.3, 8, 2), (0.45, 64, 12), (bark_alpha(8000), 512, 9), (0.58, 4096, 60)]
PRODUCT_SHAPES = SHAPES + [(bark_alpha(8000), 512, 25)]


# ---------------------------------------------------------------------------------------------------------------------------
# the definition, in a chosen dtype (float64: the yardstick; float32: e32)
# ---------------------------------------------------------------------------------------------------------------------------
def warped(alpha, L, dtype=np.float64):
    k = np.arange(L // 2 + 1).astype(dtype)
    w = dtype(2.0 * np.pi) * k / dtype(L)
    a = dtype(alpha)
    wt = w + dtype(2.0) * np.arctan2(a * np.sin(w), dtype(1.0) - a * np.cos(w))
    assert wt.dtype == dtype
    return wt


def node_weights(wt):
    q = np.empty_like(wt)
    q[1:-1] = (wt[2:] - wt[:-2]) / wt.dtype.type(2.0)
    q[0], q[-1] = (wt[1] - wt[0]) / wt.dtype.type(2.0), (wt[-1] - wt[-2]) / wt.dtype.type(2.0)
    return q


def cos_table(alpha, L, M1, dtype=np.float64):
    return np.cos(np.arange(M1).astype(dtype)[:, None] * warped(alpha, L, dtype)[None, :])


def normal_matrix(alpha, L, M1, dtype=np.float64):
    C, q = cos_table(alpha, L, M1, dtype), node_weights(warped(alpha, L, dtype))
    return (C * q[None, :]) @ C.T


_tables = {}


def fit_table(alpha, L, M1, dtype=np.float64):
    """W [M1, K] in `dtype` throughout; computed once per parameter set and left unchanged."""
    key = (float(alpha), L, M1, np.dtype(dtype).name)
    if key not in _tables:
        C, q = cos_table(alpha, L, M1, dtype), node_weights(warped(alpha, L, dtype))
        B = C * q[None, :]
        W = np.linalg.solve(B @ C.T, B)
        assert W.dtype == dtype
        W.setflags(write=False)
        _tables[key] = W
    return _tables[key]


def logspec(c, alpha, L, dtype=np.float64):
    """c [T,M1] -> logA [T,K]: what decompress_spectrum evaluates ('mcep')."""
    c = np.asarray(c).astype(dtype)
    return c @ cos_table(alpha, L, c.shape[1], dtype)


def log_input(x, is_log, dtype=np.float64):
    x = np.asarray(x).astype(dtype)
    return x if is_log else np.log(np.maximum(np.abs(x), dtype(FLT_MIN)))


def spec2mcep(x, alpha, M1, is_log=False, dtype=np.float64):
    """x [T,K] -> c [T,M1], everything in `dtype`."""
    L = 2 * (np.asarray(x).shape[-1] - 1)
    out = log_input(x, is_log, dtype) @ fit_table(alpha, L, M1, dtype).T
    assert out.dtype == dtype
    return out


def order_limit(alpha, L):
    return int(np.floor((L // 2) * (1.0 - abs(alpha)) / (1.0 + abs(alpha))))


def sptk_freqt(c, m2, a):
    """SPTK's freqt -m M -M m2 -a 0 -A a: c [T,M+1] -> [T,m2+1]."""
    T, M1 = c.shape
    g = np.zeros((T, m2 + 1))
    b = 1.0 - a * a
    for i in range(M1 - 1, -1, -1):
        d = g.copy()
        g[:, 0] = c[:, i] + a * d[:, 0]
        if m2 >= 1: g[:, 1] = b * d[:, 0] + a * d[:, 1]
        for j in range(2, m2 + 1):
            g[:, j] = d[:, j - 1] + a * (d[:, j] - g[:, j - 1])
    return g


def make_mcep(seed, T, M1):
    """c_0 in [-6, -1], c_m ~ N(0, sigma = 0.5 / (1 + m)); float32."""
    rng = np.random.RandomState(seed)
    c = rng.randn(T, M1) * (0.5 / (1.0 + np.arange(M1)))[None, :]
    c[:, 0] = rng.uniform(-6.0, -1.0, size=T)
    return c.astype(np.float32)


def make_logenv(seed, T, alpha, L, M1):
    """A log-envelope the order cannot represent: a cepstrum of twice the order (as far as the bins carry one) and 0.1 neper of
    bin-to-bin roughness on top; float32 [T,K]."""
    rng = np.random.RandomState(seed + 7)
    la = logspec(make_mcep(seed, T, min(2 * M1, L // 2)), alpha, L)
    return (la + 0.1 * rng.randn(*la.shape)).astype(np.float32)


def check(got, want64, want32, what, extra=0.0):
    """|got - want64| <= 4 e32 + ulp32(want64) (+ extra), every element."""
    got = np.asarray(got, dtype=np.float64)
    assert got.shape == want64.shape, (what, got.shape, want64.shape)
    assert np.isfinite(got).all(), what
    ulp = np.spacing(np.abs(want64).astype(np.float32)).astype(np.float64)
    err, e32 = np.abs(got - want64), np.abs(want32.astype(np.float64) - want64).max()
    print('{}: e32 = {:.3e}, kernel worst {:.3e}, worst error / bound = {:.3f}'.format(
        what, e32, err.max(), (err / (4.0 * e32 + ulp + extra)).max()))
    assert (err <= 4.0 * e32 + ulp + extra).all(), (what, e32, err.max())


# ---------------------------------------------------------------------------------------------------------------------------
# CPU
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('alpha,L,M1', CPU_SHAPES)
def test_restated_fit_inverts_the_decompression(alpha, L, M1):
    assert M1 <= order_limit(alpha, L)
    c = make_mcep(M1, 6, M1).astype(np.float64)
    err = np.abs(spec2mcep(logspec(c, alpha, L), alpha, M1, is_log=True) - c).max()
    print('alpha={:.3f} L={} M1={}: |W logspec(c) - c| = {:.3e}'.format(alpha, L, M1, err))
    assert err <= 1e-12
    lin = np.abs(spec2mcep(np.exp(logspec(c, alpha, L)), alpha, M1) - c).max()       # through exp and log, in fp64
    assert lin <= 1e-12


def test_restated_fit_is_the_cepstrum_then_freqt():
    """Two smooth envelopes no finite order represents, at (alpha 0.42, L 1024, M1 25): the least-squares fit against the
    reference's route, the real cepstrum by an inverse FFT (coefficients 1 .. L/2 - 1 doubled: one-sided) warped by freqt to
    order M1 - 1.  The two differ by the quadrature error of the trapezoid rule on the warped axis, which depends on the
    envelope's smoothness; measured 1e-8 on envelopes of this kind, asserted below 1e-6."""
    alpha, L, M1 = 0.42, 1024, 25
    w = 2.0 * np.pi * np.arange(L // 2 + 1) / L
    z = np.exp(-1j * w)
    poles = [(0.90, 0.35), (0.85, 1.1), (0.80, 2.3)]                   # three resonances
    res = -5.0 - sum(np.log(np.abs(1.0 - 2.0 * r * np.cos(th) * z + r * r * z * z)) for r, th in poles)
    bumps = -4.0 + 3.0 * np.exp(-((w - 0.6) / 0.35) ** 2) + 2.0 * np.exp(-((w - 1.9) / 0.5) ** 2) - 0.5 * w
    v = np.stack([res, bumps])
    cep = np.fft.irfft(v, n=L, axis=1)[:, :L // 2 + 1]
    cep[:, 1:L // 2] *= 2.0
    want = sptk_freqt(cep, M1 - 1, alpha)
    got = spec2mcep(v, alpha, M1, is_log=True)
    err = np.abs(got - want).max()
    print('|fit - freqt(cepstrum)| = {:.3e}, coefficients up to {:.2f}, fit residual {:.3e}'.format(
        err, np.abs(want).max(), np.abs(logspec(got, alpha, L) - v).max()))
    assert np.abs(logspec(got, alpha, L) - v).max() > 1e-4             # not representable at this order
    assert err < 1e-6


@pytest.mark.parametrize('alpha,L', sorted(set((a, L) for a, L, _ in CPU_SHAPES + SHAPES)))
def test_normal_matrix_is_well_conditioned_up_to_the_order_limit(alpha, L):
    M1 = order_limit(alpha, L)
    cond = np.linalg.cond(normal_matrix(alpha, L, M1))
    print('alpha={:.3f} L={}: cond(G) = {:.4f} at M1 = {}'.format(alpha, L, cond, M1))
    assert cond < 3.0


def test_argument_checks_without_a_device():
    import torch
    from percivaltts_amd import _hip, ops, vocoders
    ops.spec2mcep_check(59, 0.58, 4096)
    ops.spec2mcep_check(1, 0.3, 8)
    for alpha, L, _ in CPU_SHAPES + SHAPES:
        assert ops.spec2mcep_order_limit(alpha, L) == order_limit(alpha, L)
        ops.spec2mcep_check(min(order_limit(alpha, L), ops.SPECTRUM_MAX_M1) - 1, alpha, L)
    for order, alpha, L in ((2, 0.3, 8), (12, 0.45, 64), (109, bark_alpha(8000), 512),         # one above the limit
                            (0, 0.45, 64), (-1, 0.45, 64), (1.5, 0.45, 64), (ops.SPECTRUM_MAX_M1, 0.1, 4096),
                            (11, 1.0, 64), (11, -1.0, 64), (11, float('nan'), 64),
                            (3, 0.3, 7), (3, 0.3, 6), (3, 0.3, 1 << 21),
                            (511, 0.1, 1 << 16)):                                                  # a table of 128 MiB
        with pytest.raises(ValueError):
            ops.spec2mcep_check(order, alpha, L)
    assert ops.spec2mcep_table_bytes(512, 1 << 16) > ops.SPEC2MCEP_MAX_TABLE_BYTES == 32 << 20
    x = torch.ones(4, 33)
    with pytest.raises(ValueError):
        ops.spec2mcep(torch.ones(33), 0.45, 11)                     # no frame axis
    with pytest.raises(ValueError):
        ops.spec2mcep(torch.ones(2, 2, 4, 33), 0.45, 11)
    with pytest.raises(ValueError):
        ops.spec2mcep(torch.ones(4, 4), 0.45, 1)                    # K = 4: dftlen 6
    with pytest.raises(ValueError):
        ops.spec2mcep(x, 0.45, 0)                                   # order < 1
    with pytest.raises(ValueError):
        ops.spec2mcep(x, 0.45, 12)                                  # above the limit of dftlen 64
    with pytest.raises(ValueError):
        ops.spec2mcep(x.clone().requires_grad_(True), 0.45, 11)
    with pytest.raises(_hip.HipLibraryError):
        ops.spec2mcep(x, 0.45, 11)                                  # a well-formed CPU tensor reaches the device check
    with pytest.raises(_hip.HipLibraryError):
        ops.spec2mcep(x.double(), 0.45, 11)
    assert list(inspect.signature(ops.spec2mcep).parameters) == ['spec', 'alpha', 'order', 'log']
    assert list(inspect.signature(vocoders.VocoderF0Spec.compress_spectrum_device).parameters) == ['self', 'SPEC', 'spec_size', 'log']
    voc = vocoders.VocoderPML(8000, SHIFT, 9, 9, dftlen=512, spec_type='mcep')
    with pytest.raises(ValueError) as e:                            # the name stays with the SPTK fit
        voc.compress_spectrum(np.ones((2, 257), np.float32))
    assert 'compress_spectrum_device' in str(e.value)
    with pytest.raises(ValueError):                                 # 257 bins carry 109 coefficients at 8 kHz
        vocoders.VocoderPML(8000, SHIFT, 110, 9, dftlen=512, spec_type='mcep').analysis_device(np.zeros(400), np.full(10, 150.0), 100.0, 400.0)
    voc.spec_type = 'lsf'
    with pytest.raises(ValueError):
        voc.compress_spectrum_device(np.ones((2, 257), np.float32))
    for name in ('ptts_spec2mcep_table_bytes', 'ptts_spec2mcep_table', 'ptts_spec2mcep'):
        assert name in _hip.SIGNATURES, name


# ---------------------------------------------------------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------------------------------------------------------
def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _check_product(x, alpha, M1, is_log, what, extra=0.0):
    from percivaltts_amd import ops
    got = ops.spec2mcep(_dev(x), alpha, M1 - 1, log=is_log).cpu().numpy()
    assert got.dtype == np.float32
    flat = x.reshape(-1, x.shape[-1])
    check(got.reshape(-1, M1), spec2mcep(flat, alpha, M1, is_log), spec2mcep(flat, alpha, M1, is_log, dtype=np.float32), what, extra)
    return got


@pytest.mark.gpu
@pytest.mark.parametrize('alpha,L,M1', SHAPES)
def test_table_against_restatement(alpha, L, M1):
    """W as the header documents it: fp64 [K][M1p] at the table's start, M1p = M1 rounded up to 4, zeros behind M1.  Bound
    1e-10 max|W|: ulp-level differences of cos and atan2 summed over K <= 2049 terms at cond(G) about 2 stay orders below it,
    a wrong end weight or an index off by one is about 1e-3."""
    import torch
    from percivaltts_amd import _hip, ops_offline
    K, M1p = L // 2 + 1, (M1 + 3) // 4 * 4
    tab, nbytes = ops_offline._spec2mcep_table(torch.device('cuda', torch.cuda.current_device()), M1, alpha, L)
    assert nbytes == _hip.lib().ptts_spec2mcep_table_bytes(M1, L) == ops_offline.spec2mcep_table_bytes(M1, L)
    assert tab.dtype == torch.float64 and tab.data_ptr() % 32 == 0
    Wd = tab[:K * M1p].cpu().numpy().reshape(K, M1p)
    W = fit_table(alpha, L, M1)
    err = np.abs(Wd[:, :M1].T - W).max()
    print('alpha={} L={} M1={}: |W_device - W| = {:.3e}, max|W| = {:.3e}'.format(alpha, L, M1, err, np.abs(W).max()))
    assert np.isfinite(Wd).all() and err <= 1e-10 * np.abs(W).max()
    assert (Wd[:, M1:] == 0.0).all()


@pytest.mark.gpu
@pytest.mark.parametrize('alpha,L,M1', PRODUCT_SHAPES)
def test_product_against_restatement(alpha, L, M1):
    """T in {1, SPEC_TT - 1, SPEC_TT + 1, 19} and a [2, 5, K] batch, a linear envelope and a log-envelope each; one frame of the
    linear input has a zero bin (ln FLT_MIN after the clamp) and one negative amplitudes."""
    for T in (1, SPEC_TT - 1, SPEC_TT + 1, 19):
        la = make_logenv(100 * M1 + T, T, alpha, L, M1)
        _check_product(la, alpha, M1, True, 'T={} M1={} L={} log'.format(T, M1, L))
        x = np.exp(la)
        x[0, (3 * T) % (L // 2 + 1)] = 0.0
        x[T // 2] *= -1.0
        _check_product(x, alpha, M1, False, 'T={} M1={} L={} linear'.format(T, M1, L))
    la = make_logenv(100 * M1, 10, alpha, L, M1).reshape(2, 5, L // 2 + 1)
    assert _check_product(la, alpha, M1, True, 'B=2 T=5 M1={} L={} log'.format(M1, L)).shape == (2, 5, M1)
    assert _check_product(np.exp(la), alpha, M1, False, 'B=2 T=5 M1={} L={} linear'.format(M1, L)).shape == (2, 5, M1)


@pytest.mark.gpu
@pytest.mark.parametrize('alpha,L,M1', [(0.45, 64, 12), (bark_alpha(8000), 512, 25), (0.58, 4096, 257)])
def test_frames_do_not_depend_on_the_batch(alpha, L, M1):
    """The rows of a T = 19 call, bit for bit: the same frames one per call, and the same call again."""
    from percivaltts_amd import ops
    x = np.exp(make_logenv(5, 19, alpha, L, M1))
    for is_log, inp in ((False, x), (True, np.log(x))):
        whole = ops.spec2mcep(_dev(inp), alpha, M1 - 1, log=is_log).cpu().numpy()
        np.testing.assert_array_equal(ops.spec2mcep(_dev(inp), alpha, M1 - 1, log=is_log).cpu().numpy(), whole)
        for t in range(19):
            np.testing.assert_array_equal(ops.spec2mcep(_dev(inp[t:t + 1]), alpha, M1 - 1, log=is_log).cpu().numpy()[0], whole[t])


@pytest.mark.gpu
@pytest.mark.parametrize('alpha,L,M1', PRODUCT_SHAPES)
def test_inverse_of_mcep2spec_on_the_device(alpha, L, M1):
    """spec2mcep(mcep2spec(c, log), log) against c.  The decompression's own error is propagated exactly,
    sum_k |W[m,k]| |v_device,k - v_fp64,k|, and the product's tolerance on the input it was given comes on top."""
    from percivaltts_amd import ops
    c = make_mcep(M1 + 1, 11, M1)
    v = ops.mcep2spec(_dev(c), alpha, dftlen=L, log=True)
    got = ops.spec2mcep(v, alpha, M1 - 1, log=True).cpu().numpy()
    v = v.cpu().numpy()
    carried = np.abs(v.astype(np.float64) - logspec(c, alpha, L)) @ np.abs(fit_table(alpha, L, M1)).T
    want64, want32 = spec2mcep(v, alpha, M1, True), spec2mcep(v, alpha, M1, True, dtype=np.float32)
    ulp = np.spacing(np.abs(want64).astype(np.float32)).astype(np.float64)
    e32 = np.abs(want32.astype(np.float64) - want64).max()
    err = np.abs(got.astype(np.float64) - c.astype(np.float64))
    print('M1={} L={}: |round trip - c| = {:.3e}, carried {:.3e}, e32 = {:.3e}, worst error / bound = {:.3f}'.format(
        M1, L, err.max(), carried.max(), e32, (err / (carried + 4.0 * e32 + ulp)).max()))
    assert (err <= carried + 4.0 * e32 + ulp).all()


@pytest.mark.gpu
def test_compress_spectrum_device_inverts_decompress_spectrum():
    """numpy in, numpy out, through the linear envelope; the same propagation with v = ln of the float32 amplitudes.  A device
    tensor gives a device tensor with the same bits, and 'fwbnd' is compress_spectrum."""
    import torch
    from percivaltts_amd import vocoders
    fs, L, M1 = 8000, 512, 25
    alpha = bark_alpha(fs)
    voc = vocoders.VocoderPML(fs, SHIFT, M1, 9, dftlen=L, spec_type='mcep')
    c = make_mcep(77, 13, M1)
    A = voc.decompress_spectrum(c)
    got = voc.compress_spectrum_device(A)
    assert isinstance(got, np.ndarray) and got.dtype == np.float32 and got.shape == c.shape
    v = np.log(A.astype(np.float64))
    carried = np.abs(v - logspec(c, alpha, L)) @ np.abs(fit_table(alpha, L, M1)).T
    want64, want32 = spec2mcep(A, alpha, M1), spec2mcep(A, alpha, M1, dtype=np.float32)
    ulp = np.spacing(np.abs(want64).astype(np.float32)).astype(np.float64)
    e32 = np.abs(want32.astype(np.float64) - want64).max()
    err = np.abs(got.astype(np.float64) - c.astype(np.float64))
    print('compress(decompress(c)) - c: {:.3e}, carried {:.3e}, e32 = {:.3e}, worst error / bound = {:.3f}'.format(
        err.max(), carried.max(), e32, (err / (carried + 4.0 * e32 + ulp)).max()))
    assert (err <= carried + 4.0 * e32 + ulp).all()
    dev = voc.compress_spectrum_device(_dev(A))
    assert torch.is_tensor(dev) and dev.is_cuda
    np.testing.assert_array_equal(dev.cpu().numpy(), got)
    np.testing.assert_array_equal(voc.compress_spectrum_device(_dev(A), spec_size=9).cpu().numpy(),
                                  voc.compress_spectrum_device(_dev(A), 9, False).cpu().numpy())
    assert voc.compress_spectrum_device(A, spec_size=9).shape == (13, 9)
    np.testing.assert_array_equal(voc.compress_spectrum_device(np.log(A), log=True),
                                  voc.compress_spectrum_device(_dev(np.log(A)), log=True).cpu().numpy())
    fw = vocoders.VocoderPML(fs, SHIFT, M1, 9, dftlen=L)
    np.testing.assert_array_equal(fw.compress_spectrum_device(A), fw.compress_spectrum(A))


@pytest.mark.gpu
def test_no_frames_and_refusals():
    import torch
    from percivaltts_amd import _hip, ops
    with _hip.KernelTimer() as kt:
        out = ops.spec2mcep(torch.zeros(0, 33, device='cuda'), 0.45, 11)
        assert tuple(out.shape) == (0, 12) and out.dtype == torch.float32 and out.is_cuda
        assert tuple(ops.spec2mcep(torch.zeros(2, 0, 33, device='cuda'), 0.45, 11, log=True).shape) == (2, 0, 12)
    assert kt.records == []
    with pytest.raises(_hip.HipLibraryError):
        ops.spec2mcep(torch.ones(4, 33), 0.45, 11)                  # a CPU tensor
    lib = _hip.lib()
    p = ctypes.c_void_p(256)            # non-null, 32-byte aligned, never read
    big = 1 << 40

    def fit(x=p, out=p, T=5, M1=12, alpha=0.45, dftlen=64, tab=p, nt=big):
        return lib.ptts_spec2mcep(x, out, T, M1, alpha, dftlen, 0, tab, nt, None)

    def table(tab=p, nt=big, M1=12, alpha=0.45, dftlen=64):
        return lib.ptts_spec2mcep_table(tab, nt, M1, alpha, dftlen, None)

    common = (dict(M1=13), dict(M1=1), dict(M1=513, alpha=0.0, dftlen=4096), dict(dftlen=6), dict(dftlen=65), dict(dftlen=0),
              dict(alpha=1.0), dict(alpha=-1.0), dict(alpha=float('nan')), dict(alpha=-0.5),          # -0.5: the limit is 10
              dict(tab=None), dict(tab=ctypes.c_void_p(264)), dict(nt=16), dict(nt=lib.ptts_spec2mcep_table_bytes(12, 64) - 1),
              dict(M1=512, alpha=0.1, dftlen=1 << 16))                                                   # above the byte cap
    for go, extra in ((fit, (dict(T=-1), dict(x=None), dict(out=None))), (table, ())):
        for kw in common + extra:
            assert go(**kw) == EINVAL, (go.__name__, kw)
    assert 'spec2mcep' in _hip.last_error()
    assert fit(T=0) == 0 and fit(T=0, x=None, out=None, tab=None, nt=0) == 0
    assert fit(T=0, M1=13) == EINVAL and fit(T=0, dftlen=7) == EINVAL     # bad arguments stay bad at T = 0
    assert lib.ptts_spec2mcep_table_bytes(60, 4096) >= 8 * 2049 * 60 and lib.ptts_spec2mcep_table_bytes(1, 64) == 16


# ---- wiring ----------------------------------------------------------------------------------------------------------------
F0_MIN, F0_MAX = 100.0, 400.0


def _voiced(T, fs, seed):
    """A harmonic series on a slowly moving f0 with a little noise, and its f0 track with an unvoiced start."""
    rng = np.random.RandomState(seed)
    N = int(round(SHIFT * (T - 1) * fs))
    f0 = 150.0 + 40.0 * np.sin(np.arange(T) / 5.0 + rng.rand())
    phase = 2 * np.pi * np.cumsum(np.interp(np.arange(N) / float(fs), SHIFT * np.arange(T), f0)) / fs
    wav = 0.1 * sum(np.cos(h * phase) / h for h in range(1, 20)) + 0.01 * rng.randn(N)
    f0[:2] = 0.0
    return wav, f0


@pytest.mark.gpu
def test_analysis_device_with_mel_cepstra(tmp_path):
    """fs 8000, dftlen 512: the 'mcep' vocoder's f0 and noise-mask columns are the 'fwbnd' vocoder's, bit for bit, and its
    spectral columns are ops.spec2mcep of the log-envelope of ops.frame_harmonics."""
    from percivaltts_amd import ops, vocoders
    fs, L, T, N, NM = 8000, 512, 27, 12, 9
    wav, f0 = _voiced(T, fs, 3)
    mc = vocoders.VocoderPML(fs, SHIFT, N, NM, dftlen=L, spec_type='mcep')
    fw = vocoders.VocoderPML(fs, SHIFT, N, NM, dftlen=L)
    a, b = mc.analysis_device(wav, f0, F0_MIN, F0_MAX), fw.analysis_device(wav, f0, F0_MIN, F0_MAX)
    assert a.shape == b.shape == (T, 1 + N + NM) and a.dtype == np.float32 and np.isfinite(a).all()
    np.testing.assert_array_equal(a[:, 0], b[:, 0])
    np.testing.assert_array_equal(a[:, 1 + N:], b[:, 1 + N:])
    assert np.abs(a[:, 1:1 + N] - b[:, 1:1 + N]).max() > 1e-2
    track = ops.f0_track(f0, F0_MIN, F0_MAX, fs, SHIFT, L, wavlen=wav.size)
    hcap = ops.analysis_check(L, fs, SHIFT, F0_MIN, F0_MAX)
    lspec = ops.frame_harmonics(_dev(wav.astype(np.float32)), _dev(track), SHIFT, fs, L, hcap, log=True)[0]
    np.testing.assert_array_equal(a[:, 1:1 + N], ops.spec2mcep(lspec, bark_alpha(fs), N - 1, log=True).cpu().numpy())
    # from file to files
    path = str(tmp_path / 'a.wav')
    vocoders.wavwrite(path, wav, fs)
    outs = [str(tmp_path / 'o' / n) for n in ('a.lf0', 'a.mcep', 'a.nm')]
    assert mc.analysisf_device(path, f0.astype(np.float32), outs[0], F0_MIN, F0_MAX, outs[1], outs[2]) == T
    assert [os.path.getsize(p) for p in outs] == [4 * T, 4 * T * N, 4 * T * NM]
    back = mc.analysis_device(vocoders.wavread(path)[0], f0, F0_MIN, F0_MAX)           # the waveform went through 16 bits
    np.testing.assert_array_equal(np.fromfile(outs[1], dtype=np.float32).reshape(T, N), back[:, 1:1 + N])


@pytest.mark.gpu
def test_features_extraction_with_mel_cepstra(tmp_path, monkeypatch):
    """Two utterances from .wav and an F0 track through run.features_extraction with an 'mcep' vocoder: the raw cepstra land in
    <base>_mcep<N>/*.mcep and the time weights are those of create_weights_spec(spec_type='mcep') on them."""
    import importlib
    from percivaltts_amd import compose, vocoders
    monkeypatch.setenv('PERCIVAL_CORPUS', str(tmp_path / 'corpus'))
    monkeypatch.chdir(tmp_path)
    import percivaltts_amd.run as run
    run = importlib.reload(run)
    fs, N, NM = 8000, 12, 9
    voc = vocoders.VocoderPML(fs, SHIFT, N, NM, dftlen=512, spec_type='mcep')
    monkeypatch.setattr(run, 'vocoder', voc)
    nout = voc.featuressize()
    run.cfg.id_valid_start = 2
    run.cfg.outpath = str(tmp_path / 'corpus' / 'cmp' / '*.cmp') + ':(-1,{})'.format(nout)
    fids, lens = ['utt_a', 'utt_b'], [31, 24]
    os.makedirs(str(tmp_path / 'corpus' / 'wav'))
    os.makedirs(str(tmp_path / 'corpus' / 'f0'))
    for i, (fid, T) in enumerate(zip(fids, lens)):
        wav, f0 = _voiced(T, fs, 20 + i)
        wav[:int(0.03 * fs)] *= 1e-4                                # a silent start: some weights are 0
        vocoders.wavwrite(str(tmp_path / 'corpus' / 'wav' / (fid + '.wav')), wav, fs)
        f0.astype(np.float32).tofile(str(tmp_path / 'corpus' / 'f0' / (fid + '.f0')))
    with open(run.cfg.fileids, 'w') as f:
        f.write('\n'.join(fids) + '\n')
    run.features_extraction(str(tmp_path / 'corpus' / 'f0' / '*.f0'), f0_min=F0_MIN, f0_max=F0_MAX)
    raw = str(tmp_path / 'corpus' / 'wav_PML_mcep{}'.format(N) / '*.mcep')
    assert not os.path.exists(str(tmp_path / 'corpus' / 'wav_PML_fwlspec{}'.format(N)))
    compose.create_weights_spec(raw + ':(-1,{})'.format(N), fids, str(tmp_path / 'byhand' / '*.w') + ':(-1,1)', spec_type='mcep')
    for fid, T in zip(fids, lens):
        assert os.path.getsize(raw.replace('*', fid)) == 4 * T * N
        cmp_ = np.fromfile(run.cfg.outpath.split(':')[0].replace('*', fid), dtype=np.float32)
        assert cmp_.shape == (T * nout,) and np.isfinite(cmp_).all()
        w = np.fromfile(run.cfg.wpath.split(':')[0].replace('*', fid), dtype=np.float32)
        assert w.shape == (T,) and set(w) <= {0.0, 1.0} and w.max() == 1.0
        np.testing.assert_array_equal(w, np.fromfile(str(tmp_path / 'byhand' / (fid + '.w')), dtype=np.float32))
    for stat in ('mean4norm.dat', 'std4norm.dat'):
        assert os.path.getsize(os.path.join(os.path.dirname(run.cfg.outpath), stat)) == 4 * nout
