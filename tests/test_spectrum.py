"""Spectral envelope decompression and the mel-cepstral post-filter (csrc/spectrum.hip, ops.mcep_postfilter / mcep2spec /
fwbnd2spec, external/merlin/generate_pp.py, VocoderF0Spec.decompress_spectrum, ModelTTS.generate_params(specdir=...)).

The reference's post-filter is seven SPTK command lines (external/merlin/generate_pp.py mcep_postproc_sptk); SPTK is nowhere to be
had, so `sptk_postfilter` restates the tools from their definitions in numpy fp64 and the CPU tests check that the closed form
the kernels evaluate is that pipeline.  With L = dftlen, K = L/2 + 1, w_k = 2 pi k / L, wt_k = w_k + 2 atan2(a sin w_k, 1 - a cos w_k):

    logA_k(c) = sum_m c_m cos(m wt_k);   r0(x) = (1/L) (E_0 + E_{K-1} + 2 sum_{0<k<K-1} E_k),  E_k = exp(2 x_k)
    post-filter:  c' = c * [1, 1, pf, pf, ...];  out_0 = c'_0 + ln(r0(logA(c)) / r0(logA(c'))) / 2;  out_m = c'_m

Tolerance of the device results, a rule and not a tuned number: the yardstick is the closed form in fp64.  The same closed form
is also evaluated with every array and intermediate in float32, and its largest error against fp64 ON THE SAME INPUT is e32
(absolute for cepstra and log-spectra, relative for linear spectra).  Every element of the kernel's result has to lie within
4 * e32 + one float32 ulp of the value.  The factor 4 covers another summation order and the device's cos / exp / log; it is a
margin, not a measurement.  `check` prints e32 and the kernel's worst error before it asserts."""
import ctypes
import inspect
import os

import numpy as np
import pytest

PF = 1.4
EINVAL = -1


# ---------------------------------------------------------------------------------------------------------------------------
# the closed forms, in a chosen dtype (float64: the yardstick; float32: e32)
# ---------------------------------------------------------------------------------------------------------------------------
def bark_alpha(fs):
    return 0.8517 * np.sqrt(np.arctan(0.06583 * fs / 1000.0)) - 0.1916


def warped(alpha, L, dtype=np.float64):
    k = np.arange(L // 2 + 1).astype(dtype)
    w = dtype(2.0 * np.pi) * k / dtype(L)
    a = dtype(alpha)
    wt = w + dtype(2.0) * np.arctan2(a * np.sin(w), dtype(1.0) - a * np.cos(w))
    assert wt.dtype == dtype
    return wt


def logspec(c, alpha, L, dtype=np.float64):
    """c [T,M1] -> logA [T,K], everything in `dtype`."""
    c = np.asarray(c).astype(dtype)
    m = np.arange(c.shape[1]).astype(dtype)
    C = np.cos(m[:, None] * warped(alpha, L, dtype)[None, :])
    out = c @ C
    assert out.dtype == dtype
    return out


def r0(la, L):
    E = np.exp(la.dtype.type(2.0) * la)
    return (E[:, 0] + E[:, -1] + la.dtype.type(2.0) * E[:, 1:-1].sum(axis=1)) / la.dtype.type(L)


def postfilter(c, alpha, L, pf=PF, dtype=np.float64):
    c = np.asarray(c).astype(dtype)
    w = np.full(c.shape[1], pf, dtype=dtype)
    w[:2] = 1.0
    cp = c * w
    out = cp.copy()
    out[:, 0] = cp[:, 0] + dtype(0.5) * np.log(r0(logspec(c, alpha, L, dtype), L) / r0(logspec(cp, alpha, L, dtype), L))
    assert out.dtype == dtype
    return out


def mcep2spec(c, alpha, L, log=False, pp=False, pf=PF, dtype=np.float64):
    la = logspec(postfilter(c, alpha, L, pf, dtype) if pp else c, alpha, L, dtype)
    return la if log else np.exp(la)


def band_centres(nb, fs, dtype=np.float64):
    melmax = dtype(1127.0) * np.log(dtype(1.0) + dtype(0.5 * fs) / dtype(700.0))
    b = np.arange(nb).astype(dtype)
    return dtype(700.0) * (np.exp(b * melmax / (dtype(nb - 1) * dtype(1127.0))) - dtype(1.0))


def fwbnd_logspec(fw, fs, L, dtype=np.float64):
    """Linear interpolation (in Hz) of the band values at k fs / L, written out so that every intermediate is `dtype`."""
    fw = np.asarray(fw).astype(dtype)
    nb = fw.shape[1]
    fb = band_centres(nb, fs, dtype)
    f = np.arange(L // 2 + 1).astype(dtype) * dtype(fs) / dtype(L)
    b = np.clip(np.searchsorted(fb, f, side='right') - 1, 0, nb - 2)
    frac = np.clip((f - fb[b]) / (fb[b + 1] - fb[b]), dtype(0.0), dtype(1.0))
    out = np.ascontiguousarray(fw[:, b] + frac[None, :] * (fw[:, b + 1] - fw[:, b]))
    assert out.dtype == dtype
    return out


def fwbnd2spec(fw, fs, L, log=False, pp=False, pf=PF, dtype=np.float64):
    la = fwbnd_logspec(fw, fs, L, dtype)
    if pp:
        wt = warped(bark_alpha(fs), L, dtype)
        q = np.empty_like(wt)
        q[1:-1] = (wt[2:] - wt[:-2]) / dtype(2.0)
        q[0], q[-1] = (wt[1] - wt[0]) / dtype(2.0), (wt[-1] - wt[-2]) / dtype(2.0)
        cw = np.cos(wt)
        c0 = (la * q).sum(axis=1) / dtype(np.pi)
        c1 = dtype(2.0) * (la * q * cw).sum(axis=1) / dtype(np.pi)
        lb = dtype(pf) * la - dtype(pf - 1.0) * (c0[:, None] + c1[:, None] * cw[None, :])
        la = lb + (dtype(0.5) * np.log(r0(la, L) / r0(lb, L)))[:, None]
    assert la.dtype == dtype
    return la if log else np.exp(la)


# ---------------------------------------------------------------------------------------------------------------------------
# the SPTK command lines of mcep_postproc_sptk, restated (fp64, frames along axis 0)
# ---------------------------------------------------------------------------------------------------------------------------
def sptk_freqt(c, m2, a):
    """freqt -m M -M m2 with the all-pass constant a (for `-a a1 -A a2`: a = (a2 - a1) / (1 - a1 a2)): c [T,M+1] -> [T,m2+1]."""
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


def sptk_c2acr_r0(c, L):
    """c2acr -m M -M 0 -l L: the zero-lag autocorrelation of the spectrum exp(2 Re FFT(c padded to L))."""
    x = np.zeros((c.shape[0], L))
    x[:, :c.shape[1]] = c
    return np.exp(2.0 * np.fft.fft(x, axis=1).real).mean(axis=1)


def sptk_mc2b(c, a):
    b = c.copy()
    for i in range(c.shape[1] - 2, -1, -1):
        b[:, i] = c[:, i] - a * b[:, i + 1]
    return b


def sptk_b2mc(b, a):
    mc = b.copy()
    for i in range(b.shape[1] - 2, -1, -1):
        mc[:, i] = b[:, i] + a * b[:, i + 1]
    return mc


def sptk_postfilter(c, alpha, L, pf=PF, order=None):
    """`order`: freqt's -M (and c2acr's -m), L/2 + 1 in the reference.
    echo 1 1 pf pf ... > weight
    freqt -m M -a alpha -M L/2+1 -A 0 < mgc | c2acr -m L/2+1 -M 0 -l L > r0
    vopr -m mgc weight | freqt ... | c2acr ... > p_r0
    vopr -m mgc weight | mc2b -m M -a alpha | bcp -n M -s 0 -e 0 > b0
    vopr -d r0 p_r0 | sopr -LN -d 2 | vopr -a b0 > p_b0
    vopr -m mgc weight | mc2b -m M -a alpha | bcp -n M -s 1 -e M > p_b1
    merge -n M-1 -s 0 -N 0 p_b0 < p_b1 | b2mc -m M -a alpha > p_mgc"""
    c = np.asarray(c, dtype=np.float64)
    weight = np.full(c.shape[1], pf)
    weight[:2] = 1.0
    cw = c * weight
    order = L // 2 + 1 if order is None else order
    r0_ = sptk_c2acr_r0(sptk_freqt(c, order, -alpha), L)
    p_r0 = sptk_c2acr_r0(sptk_freqt(cw, order, -alpha), L)
    b = sptk_mc2b(cw, alpha)
    b0 = b[:, :1]                                   # bcp -s 0 -e 0
    p_b0 = np.log(r0_ / p_r0)[:, None] / 2.0 + b0
    p_b1 = b[:, 1:]                                 # bcp -s 1 -e M
    return sptk_b2mc(np.concatenate([p_b0, p_b1], axis=1), alpha)       # merge


def make_mcep(seed, T, M1):
    """c_0 in [-6, -1], c_m ~ N(0, sigma = 0.5 / (1 + m)); float32."""
    rng = np.random.RandomState(seed)
    c = rng.randn(T, M1) * (0.5 / (1.0 + np.arange(M1)))[None, :]
    c[:, 0] = rng.uniform(-6.0, -1.0, size=T)
    return c.astype(np.float32)


def make_fwbnd(seed, T, nb):
    """Log-amplitudes of the bands: a level in [-6, -1] per frame, a random walk over the bands on top; float32."""
    rng = np.random.RandomState(seed)
    return (rng.uniform(-6.0, -1.0, size=(T, 1)) + np.cumsum(rng.randn(T, nb) * 0.3, axis=1)).astype(np.float32)


def check(got, want64, want32, kind, what):
    """|got - want64| <= 4 e32 + ulp32(want64), every element; `kind`: 'abs' or 'rel'."""
    got = np.asarray(got, dtype=np.float64)
    assert got.shape == want64.shape, (what, got.shape, want64.shape)
    assert np.isfinite(got).all(), what
    ulp = np.spacing(np.abs(want64).astype(np.float32)).astype(np.float64)
    err, err32 = np.abs(got - want64), np.abs(want32.astype(np.float64) - want64)
    if kind == 'rel':
        err, err32, ulp = err / np.abs(want64), err32 / np.abs(want64), ulp / np.abs(want64)
    e32 = err32.max()
    print('{}: e32 = {:.3e}, kernel worst {:.3e} ({}), worst error / bound = {:.3f}'.format(
        what, e32, err.max(), kind, (err / (4.0 * e32 + ulp)).max()))
    assert (err <= 4.0 * e32 + ulp).all(), (what, e32, err.max())


# ---------------------------------------------------------------------------------------------------------------------------
# CPU
# ---------------------------------------------------------------------------------------------------------------------------
def test_header_declares_and_library_exports_the_symbols():
    from percivaltts_amd import _hip
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, 'include', 'percival_hip.h')) as f:
        header = f.read()
    names = ['ptts_mcep_postfilter', 'ptts_mcep2spec', 'ptts_fwbnd2spec', 'ptts_mcep_table', 'ptts_mcep_table_bytes',
             'ptts_fwbnd_table', 'ptts_fwbnd_table_bytes']
    assert 'int ptts_mcep_postfilter(const float* mcep, float* out, int T, int M1, double alpha, int dftlen, double pf_coef,' in header
    assert 'int ptts_mcep2spec(const float* mcep, float* spec, int T, int M1, double alpha, int dftlen, int log_out, int postfilter,' in header
    assert 'int ptts_fwbnd2spec(const float* fw, float* spec, int T, int nb, double fs, double alpha, int dftlen, int log_out,' in header
    for n in names:
        assert n in header and n in _hip.SIGNATURES, n
    if not os.path.exists(_hip.LIB_PATH):
        pytest.skip('libpercival_hip.so not built (run __graft_entry__.build())')
    lib = ctypes.CDLL(_hip.LIB_PATH)
    for n in names:
        assert hasattr(lib, n), n


@pytest.mark.parametrize('fs', [16000, 32000, 44100])
def test_sptk_pipeline_equals_the_closed_form(fs):
    """The seven command lines against the closed form, <= 1e-8 absolute, at L in {512, 1024} x M in {4, 24, 59}, on the inputs of
    the GPU tests (make_mcep).

    freqt cuts the unwarped cepstrum at order L/2 + 1.  cos(m wt(w)) oscillates up to m (1 + alpha) / (1 - alpha) times as fast as
    cos(m w), so coefficient m reaches unwarped orders up to about that: 219 for M = 59 at 16 kHz, 352 at 32 kHz, 426 at 44.1 kHz.
    Where the reach stays below L/2 + 1 the command lines agree with the closed form to 1e-15 .. 1e-9 as they are.  At the two
    points where it does not (M = 59, L = 512, 32 and 44.1 kHz) the command lines THEMSELVES are 1.1e-4 / 1.4e-4 off on these
    inputs: that is the reference's truncation, not the reduction, and the kernels evaluate the untruncated form.  There the
    test asserts (a) that the gap IS the truncation: with freqt's order raised to L - 1, all an L-point FFT can hold, the same
    command lines on the same inputs come at least a thousand times closer (measured 1.1e-4 -> 7e-15 and 1.4e-4 -> 2e-8, the
    rest being the orders beyond L - 1), and (b) the command lines as they are, <= 1e-8, on inputs whose high coefficients have
    died out (c_m * 0.8^m: measured 2e-13 / 1.5e-11)."""
    alpha = bark_alpha(fs)
    for L in (512, 1024):
        for M in (4, 24, 59):
            c = make_mcep(1000 + M, 3, M + 1).astype(np.float64)
            reach = M * (1.0 + alpha) / (1.0 - alpha)
            if reach > L // 2 + 1:
                raw = np.abs(sptk_postfilter(c, alpha, L) - postfilter(c, alpha, L)).max()
                full = np.abs(sptk_postfilter(c, alpha, L, order=L - 1) - postfilter(c, alpha, L)).max()
                print('fs={} L={} M={}: reach {:.0f} > {}: as they are {:.3e}, freqt order L-1 {:.3e}'.format(
                    fs, L, M, reach, L // 2 + 1, raw, full))
                assert full <= 1e-3 * raw, (fs, L, M, raw, full)
                c[:, 1:] *= 0.8 ** np.arange(1, M + 1)
            want = postfilter(c, alpha, L)
            got = sptk_postfilter(c, alpha, L)
            err = np.abs(got - want).max()
            print('fs={} L={} M={}: |pipeline - closed form| = {:.3e}'.format(fs, L, M, err))
            assert err <= 1e-8, (fs, L, M, err)
            np.testing.assert_array_equal(want[:, 1], c[:, 1])
            np.testing.assert_array_equal(want[:, 2:], c[:, 2:] * PF)
            assert np.abs(want[:, 0] - c[:, 0]).min() > 1e-4          # the correction is there


def test_m1_equal_2_is_the_identity():
    c = make_mcep(3, 5, 2).astype(np.float64)
    for alpha in (0.0, bark_alpha(16000), bark_alpha(44100)):
        np.testing.assert_array_equal(postfilter(c, alpha, 512), c)
        np.testing.assert_allclose(sptk_postfilter(c, alpha, 512), c, rtol=0, atol=1e-14)


def test_bark_alpha():
    from percivaltts_amd import ops, vocoders
    from percivaltts_amd.external.merlin import generate_pp
    for fs in (8000, 16000, 22050, 32000, 44100, 48000):
        want = 0.8517 * np.sqrt(np.arctan(0.06583 * fs / 1000.0)) - 0.1916
        for fn in (ops.bark_alpha, vocoders.bark_alpha, generate_pp.bark_alpha):
            assert abs(fn(fs) - want) <= 1e-15, (fs, fn)
    assert abs(ops.bark_alpha(16000) - 0.58) < 0.01 and abs(ops.bark_alpha(44100) - 0.76) < 0.01       # the textbook values


def test_fwbnd_restatement_is_numpy_interp_on_the_documented_axis():
    for nb, fs, L in ((2, 16000, 8), (9, 44100, 512), (65, 16000, 1024)):
        fb = band_centres(nb, fs)
        assert fb[0] == 0.0 and abs(fb[-1] - fs / 2.0) <= 1e-9 * fs and (np.diff(fb) > 0).all()
        fw = make_fwbnd(5, 4, nb).astype(np.float64)
        f = np.arange(L // 2 + 1) * fs / L
        want = np.stack([np.interp(f, fb, row) for row in fw])
        np.testing.assert_allclose(fwbnd_logspec(fw, fs, L), want, rtol=0, atol=1e-12)
    # the two properties of the spectral-domain post-filter, on the restatement itself
    fw = make_fwbnd(6, 3, 33)
    la, out = fwbnd_logspec(fw, 32000, 512), fwbnd2spec(fw, 32000, 512, log=True, pp=True)
    np.testing.assert_allclose(r0(out, 512), r0(la, 512), rtol=1e-12)
    np.testing.assert_array_equal(fwbnd2spec(fw, 32000, 512, pp=True, pf=1.0), fwbnd2spec(fw, 32000, 512))


def test_ops_argument_checks_run_before_the_device_is_touched():
    """Every one of these is a ValueError with CPU tensors: the shape and value checks come first.  A well-formed CPU tensor is
    what reaches the device check."""
    import torch
    from percivaltts_amd import _hip, ops
    c, fw = torch.zeros(4, 5), torch.zeros(4, 9)
    for fn, x, a in ((ops.mcep_postfilter, c, 0.5), (ops.mcep2spec, c, 0.5), (ops.fwbnd2spec, fw, 16000)):
        for kw in (dict(dftlen=7), dict(dftlen=6), dict(dftlen=513), dict(dftlen=1 << 21), dict(pf_coef=0.0), dict(pf_coef=float('nan'))):
            with pytest.raises(ValueError):
                fn(x, a, **kw)
        with pytest.raises(ValueError):
            fn(torch.zeros(5), a)                               # no frame axis
        with pytest.raises(ValueError):
            fn(torch.zeros(2, 2, 4, 5), a)
        with pytest.raises(ValueError):
            fn(torch.zeros(4, 1), a)                            # M1 < 2, nb < 2
        with pytest.raises(ValueError):
            fn(x.clone().requires_grad_(True), a)
        with pytest.raises(_hip.HipLibraryError):
            fn(x, a, dftlen=64)                                 # CPU tensor
        with pytest.raises(_hip.HipLibraryError):
            fn(x.double(), a, dftlen=64)
    for fn in (ops.mcep_postfilter, ops.mcep2spec):
        for alpha in (1.0, -1.0, 1.5, float('nan')):
            with pytest.raises(ValueError):
                fn(c, alpha)
        with pytest.raises(ValueError):
            fn(torch.zeros(4, ops.SPECTRUM_MAX_M1 + 1), 0.5)
    for fs in (0, -16000, float('nan')):
        with pytest.raises(ValueError):
            ops.fwbnd2spec(fw, fs)
    with pytest.raises(ValueError):
        ops.fwbnd2spec(torch.zeros(4, ops.SPECTRUM_MAX_NB + 1), 16000)


def test_entry_points_reject_bad_arguments():
    """PTTS_EINVAL before any launch; T = 0 is a success without one (no pointer is dereferenced on the host)."""
    from percivaltts_amd import _hip
    if not os.path.exists(_hip.LIB_PATH):
        pytest.skip('libpercival_hip.so not built (run __graft_entry__.build())')
    lib = _hip.lib()
    p = ctypes.c_void_p(256)            # non-null, 32-byte aligned, never read
    big = 1 << 40

    def pf(mcep=p, out=p, T=5, M1=4, alpha=0.5, dftlen=64, pfc=1.4, tab=p, nt=big):
        return lib.ptts_mcep_postfilter(mcep, out, T, M1, alpha, dftlen, pfc, tab, nt, None)

    def m2s(mcep=p, out=p, T=5, M1=4, alpha=0.5, dftlen=64, pfc=1.4, tab=p, nt=big):
        return lib.ptts_mcep2spec(mcep, out, T, M1, alpha, dftlen, 0, 1, pfc, tab, nt, None)

    def f2s(fw=p, out=p, T=5, nb=4, fs=16000.0, alpha=0.5, dftlen=64, pfc=1.4, tab=p, nt=big):
        return lib.ptts_fwbnd2spec(fw, out, T, nb, fs, alpha, dftlen, 0, 1, pfc, tab, nt, None)

    common = (dict(T=-1), dict(dftlen=6), dict(dftlen=65), dict(dftlen=0), dict(alpha=1.0), dict(alpha=-1.0), dict(alpha=float('nan')),
              dict(out=None), dict(tab=None), dict(nt=16), dict(pfc=0.0))
    for go, extra in ((pf, (dict(M1=1), dict(M1=0), dict(M1=513), dict(mcep=None))),
                      (m2s, (dict(M1=1), dict(M1=513), dict(mcep=None))),
                      (f2s, (dict(nb=1), dict(nb=1025), dict(fw=None), dict(fs=0.0)))):
        for kw in common + extra:
            assert go(**kw) == EINVAL, (go.__name__, kw)
        assert go(T=0) == 0 and go(T=0, out=None, tab=None) == 0
        assert go(T=0, dftlen=7) == EINVAL                      # bad arguments stay bad at T = 0
    assert 'fwbnd2spec' in _hip.last_error()
    # tables
    assert lib.ptts_mcep_table_bytes(60, 4096) >= 60 * 2052 * 4 and lib.ptts_fwbnd_table_bytes(4096) >= 4 * 2052 * 8
    assert lib.ptts_mcep_table(p, big, 1, 0.5, 64, None) == EINVAL
    assert lib.ptts_mcep_table(p, big, 4, 1.0, 64, None) == EINVAL
    assert lib.ptts_mcep_table(p, 16, 4, 0.5, 64, None) == EINVAL
    assert lib.ptts_mcep_table(None, big, 4, 0.5, 64, None) == EINVAL
    assert lib.ptts_fwbnd_table(p, big, 1, 16000.0, 0.5, 64, None) == EINVAL
    assert lib.ptts_fwbnd_table(p, big, 4, 16000.0, 0.5, 63, None) == EINVAL
    assert lib.ptts_fwbnd_table(p, 16, 4, 16000.0, 0.5, 64, None) == EINVAL


def test_vocoder_spec_type_and_generate_params_signature():
    from percivaltts_amd import modeltts, vocoders
    assert vocoders.VocoderPML(16000, 0.005, 12, 4).spec_type == 'fwbnd'
    assert vocoders.VocoderWORLD(16000, 0.005, 12, 4).spec_type == 'fwbnd'
    assert vocoders.VocoderPML(16000, 0.005, 12, 4, spec_type='mcep').spec_type == 'mcep'
    assert vocoders.VocoderWORLD(16000, 0.005, 12, 4, mlpg_wins=None, spec_type='mcep').spec_type == 'mcep'
    assert list(inspect.signature(vocoders.VocoderPML.__init__).parameters)[-1] == 'spec_type'
    assert list(inspect.signature(vocoders.VocoderWORLD.__init__).parameters)[-1] == 'spec_type'
    sig = inspect.signature(modeltts.ModelTTS.generate_params).parameters
    assert sig['pp_mcep'].default is False and sig['specdir'].default is None
    assert sig['do_objmeas'].default is True and sig['batch_size'].default == 8
    d = inspect.signature(vocoders.VocoderF0Spec.decompress_spectrum).parameters
    assert d['spec_type'].default is None and d['pp_mcep'].default is False
    voc = vocoders.VocoderPML(16000, 0.005, 12, 4)
    with pytest.raises(NotImplementedError):
        voc.synthesis(None)
    voc.spec_type = 'lsf'
    with pytest.raises(ValueError):
        voc.decompress_spectrum(np.zeros((3, 12), np.float32))


# ---------------------------------------------------------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------------------------------------------------------
TS = (1, 3, 67, 130)
ALPHAS = (0.0, bark_alpha(16000), bark_alpha(44100))


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _check_mcep_case(c, alpha, L, what):
    """The four results for one input, each against fp64 with its own e32."""
    from percivaltts_amd import ops
    cd = _dev(c)
    check(ops.mcep_postfilter(cd, alpha, dftlen=L).cpu().numpy(), postfilter(c, alpha, L), postfilter(c, alpha, L, dtype=np.float32),
          'abs', what + ' postfilter')
    for log, pp in ((False, False), (True, False), (False, True), (True, True)):
        got = ops.mcep2spec(cd, alpha, dftlen=L, log=log, pp=pp).cpu().numpy()
        check(got, mcep2spec(c, alpha, L, log, pp), mcep2spec(c, alpha, L, log, pp, dtype=np.float32), 'abs' if log else 'rel',
              '{} mcep2spec log={} pp={}'.format(what, int(log), int(pp)))


@pytest.mark.gpu
@pytest.mark.parametrize('dftlen', [8, 512, 1024])
@pytest.mark.parametrize('M1', [2, 3, 25, 60])
def test_mcep_kernels_against_restatement(M1, dftlen):
    """T in {1, 3, 67, 130} x alpha in {0, bark(16 kHz), bark(44.1 kHz)} for this (M1, dftlen).  K = 5 leaves most lanes idle,
    K = 257 / 513 is no multiple of the wave or the vector width, 67 and 130 frames are no multiple of a workgroup's."""
    from percivaltts_amd import ops
    for ai, alpha in enumerate(ALPHAS):
        for T in TS:
            c = make_mcep(100 * M1 + 10 * ai + T, T, M1)
            _check_mcep_case(c, alpha, dftlen, 'T={} M1={} L={} alpha={:.3f}'.format(T, M1, dftlen, alpha))
    if M1 == 2:     # the identity, bit for bit
        c = make_mcep(7, 67, 2)
        np.testing.assert_array_equal(ops.mcep_postfilter(_dev(c), ALPHAS[1], dftlen=dftlen).cpu().numpy(), c)


@pytest.mark.gpu
def test_mcep_kernels_many_workgroups():
    """T = 4100 at dftlen = 512: 513 workgroups, more than one round of them."""
    _check_mcep_case(make_mcep(11, 4100, 60), bark_alpha(16000), 512, 'T=4100 M1=60 L=512')


@pytest.mark.gpu
@pytest.mark.parametrize('fs', [16000, 44100])
@pytest.mark.parametrize('nb', [2, 9, 65])
def test_fwbnd_kernel_against_restatement(nb, fs):
    from percivaltts_amd import ops
    for L in (8, 512, 1024):
        for T in TS:
            fw = make_fwbnd(100 * nb + T + L, T, nb)
            fd = _dev(fw)
            what = 'T={} nb={} fs={} L={}'.format(T, nb, fs, L)
            for log, pp in ((False, False), (True, False), (False, True), (True, True)):
                got = ops.fwbnd2spec(fd, fs, dftlen=L, log=log, pp=pp).cpu().numpy()
                check(got, fwbnd2spec(fw, fs, L, log, pp), fwbnd2spec(fw, fs, L, log, pp, dtype=np.float32), 'abs' if log else 'rel',
                      '{} fwbnd2spec log={} pp={}'.format(what, int(log), int(pp)))
            # the post-filter keeps r0.  Each amplitude is one fp32 rounding (2^-24) off, its square 2^-23, and a sum of positive
            # terms is no further off than its worst term; the fp64 arithmetic in front of the rounding is orders below.
            plain = ops.fwbnd2spec(fd, fs, dftlen=L).cpu().numpy()
            pp_out = ops.fwbnd2spec(fd, fs, dftlen=L, pp=True).cpu().numpy().astype(np.float64)
            want_r0 = r0(fwbnd_logspec(fw, fs, L), L)
            got_r0 = (pp_out[:, 0] ** 2 + pp_out[:, -1] ** 2 + 2.0 * (pp_out[:, 1:-1] ** 2).sum(axis=1)) / L
            rel = np.abs(got_r0 / want_r0 - 1.0).max()
            print('{}: r0 after / before - 1 = {:.3e}'.format(what, rel))
            assert rel <= 2.0 ** -23 + 1e-12
            # pf_coef = 1 is the plain envelope, bit for bit
            np.testing.assert_array_equal(ops.fwbnd2spec(fd, fs, dftlen=L, pp=True, pf_coef=1.0).cpu().numpy(), plain)


@pytest.mark.gpu
def test_fwbnd_kernel_many_workgroups():
    from percivaltts_amd import ops
    fw = make_fwbnd(13, 4100, 65)
    for pp in (False, True):
        check(ops.fwbnd2spec(_dev(fw), 16000, dftlen=512, pp=pp).cpu().numpy(), fwbnd2spec(fw, 16000, 512, pp=pp),
              fwbnd2spec(fw, 16000, 512, pp=pp, dtype=np.float32), 'rel', 'T=4100 nb=65 L=512 pp={}'.format(int(pp)))


@pytest.mark.gpu
def test_batch_invariance_and_repeatability():
    """[B,T,.] equals the per-utterance calls bit for bit, whatever the utterance's position does to the frames' places in a
    workgroup (T = 13 is no multiple of a workgroup's frames); two calls give the same bits."""
    from percivaltts_amd import ops
    B, T, L = 3, 13, 512
    alpha = bark_alpha(16000)
    c, fw = make_mcep(21, B * T, 25).reshape(B, T, 25), make_fwbnd(22, B * T, 33).reshape(B, T, 33)
    fns = [lambda x: ops.mcep_postfilter(x, alpha, dftlen=L), lambda x: ops.mcep2spec(x, alpha, dftlen=L),
           lambda x: ops.mcep2spec(x, alpha, dftlen=L, pp=True), lambda x: ops.mcep2spec(x, alpha, dftlen=L, log=True)]
    for fn in fns:
        whole = fn(_dev(c)).cpu().numpy()
        assert whole.shape[:2] == (B, T)
        np.testing.assert_array_equal(fn(_dev(c)).cpu().numpy(), whole)
        for b in range(B):
            np.testing.assert_array_equal(fn(_dev(c[b])).cpu().numpy(), whole[b])
    for pp in (False, True):
        whole = ops.fwbnd2spec(_dev(fw), 16000, dftlen=L, pp=pp).cpu().numpy()
        assert whole.shape == (B, T, L // 2 + 1)
        np.testing.assert_array_equal(ops.fwbnd2spec(_dev(fw), 16000, dftlen=L, pp=pp).cpu().numpy(), whole)
        for b in range(B):
            np.testing.assert_array_equal(ops.fwbnd2spec(_dev(fw[b]), 16000, dftlen=L, pp=pp).cpu().numpy(), whole[b])
    # no frames: the shapes, and nothing launched
    import torch
    from percivaltts_amd import _hip
    with _hip.KernelTimer() as kt:
        assert ops.mcep2spec(torch.zeros(0, 25, device='cuda'), alpha, dftlen=L).shape == (0, L // 2 + 1)
        assert ops.mcep_postfilter(torch.zeros(2, 0, 25, device='cuda'), alpha, dftlen=L).shape == (2, 0, 25)
        assert ops.fwbnd2spec(torch.zeros(0, 33, device='cuda'), 16000, dftlen=L).shape == (0, L // 2 + 1)
    assert kt.records == []


@pytest.mark.gpu
def test_neighbours_in_a_padded_buffer_stay_untouched():
    """Guard rows in front of and behind the output, through the C ABI: T = 11 frames (a partial workgroup), K = 257 (a partial
    vector at the end of every row, rows on every alignment)."""
    import torch
    from percivaltts_amd import _hip
    from percivaltts_amd._hip import call, ptr, stream
    lib = _hip.lib()
    T, M1, nb, L, G, SENT = 11, 25, 33, 512, 3, -777.0
    K = L // 2 + 1
    alpha = bark_alpha(16000)
    nmt, nft = lib.ptts_mcep_table_bytes(M1, L), lib.ptts_fwbnd_table_bytes(L)
    mtab = torch.empty(nmt // 4, dtype=torch.float32, device='cuda')
    ftab = torch.empty(nft // 8, dtype=torch.float64, device='cuda')
    call('ptts_mcep_table', ptr(mtab), nmt, M1, alpha, L, stream())
    call('ptts_fwbnd_table', ptr(ftab), nft, nb, 16000.0, alpha, L, stream())
    c, fw = _dev(make_mcep(31, T, M1)), _dev(make_fwbnd(32, T, nb))

    def guarded(width, launch):
        buf = torch.full(((T + 2 * G) * width,), SENT, dtype=torch.float32, device='cuda')
        launch(ctypes.c_void_p(buf.data_ptr() + G * width * 4))
        out = buf.cpu().numpy().reshape(T + 2 * G, width)
        assert (out[:G] == SENT).all() and (out[G + T:] == SENT).all()
        assert (out[G:G + T] != SENT).all() and np.isfinite(out[G:G + T]).all()
        return out[G:G + T]

    got = guarded(M1, lambda o: call('ptts_mcep_postfilter', ptr(c), o, T, M1, alpha, L, PF, ptr(mtab), nmt, stream()))
    check(got, postfilter(c.cpu().numpy(), alpha, L), postfilter(c.cpu().numpy(), alpha, L, dtype=np.float32), 'abs', 'guarded postfilter')
    for pp in (0, 1):
        guarded(K, lambda o: call('ptts_mcep2spec', ptr(c), o, T, M1, alpha, L, 0, pp, PF, ptr(mtab), nmt, stream()))
        guarded(K, lambda o: call('ptts_fwbnd2spec', ptr(fw), o, T, nb, 16000.0, alpha, L, 0, pp, PF, ptr(ftab), nft, stream()))


@pytest.mark.gpu
def test_reference_names_numpy_in_numpy_out():
    import torch
    from percivaltts_amd import vocoders
    from percivaltts_amd.external.merlin import generate_pp
    c = make_mcep(41, 20, 25)
    got = generate_pp.mcep_postproc_sptk(c.astype(np.float64), 16000, dftlen=512)
    assert isinstance(got, np.ndarray) and got.dtype == np.float32 and got.shape == c.shape
    alpha = bark_alpha(16000)
    check(got, postfilter(c, alpha, 512), postfilter(c, alpha, 512, dtype=np.float32), 'abs', 'mcep_postproc_sptk')
    for spec_type, x, want in (('mcep', c, lambda pp: mcep2spec(c, alpha, 512, pp=pp)),
                               ('fwbnd', make_fwbnd(42, 20, 25), None)):
        voc = vocoders.VocoderPML(16000, 0.005, 25, 4, dftlen=512, spec_type=spec_type)
        for pp in (False, True):
            a = voc.decompress_spectrum(x, pp_mcep=pp)
            b = voc.decompress_spectrum(_dev(x), voc.spec_type, pp_mcep=pp)
            assert isinstance(a, np.ndarray) and a.dtype == np.float32 and a.shape == (20, 257)
            assert torch.is_tensor(b) and b.is_cuda
            np.testing.assert_array_equal(b.cpu().numpy(), a)
            w64 = want(pp) if want is not None else fwbnd2spec(x, 16000, 512, pp=pp)
            w32 = (mcep2spec(x, alpha, 512, pp=pp, dtype=np.float32) if want is not None
                   else fwbnd2spec(x, 16000, 512, pp=pp, dtype=np.float32))
            check(a, w64, w32, 'rel', 'decompress_spectrum {} pp={}'.format(spec_type, int(pp)))


# ---- end to end ----------------------------------------------------------------------------------------------------------
REF_WINS = [[-0.5, 0.0, 0.5], [1.0, -2.0, 1.0]]
E2E_DFTLEN = 256


def _model(spec_type, wins):
    import percivaltts_amd
    from percivaltts_amd import modeltts_common, vocoders
    cfg = percivaltts_amd.configuration()
    cfg.arch_hiddenwidth = 8; cfg.train_batch_size = 2
    ctx = 19
    voc = vocoders.VocoderPML(16000, 0.005, 12, 4, dftlen=E2E_DFTLEN, mlpg_wins=wins, spec_type=spec_type)
    return ctx, voc, modeltts_common.Generic(ctx, voc, layertypes=['FC', 'BLSTM'], cfgarch=cfg)


def _corpus(tmp_path, ctx, voc, lens, seed=0):
    """Synthetic label files and normalisation statistics that keep the de-normalised spectral columns in a speech-like range
    (f0 | 12 spectral columns around a level of -3 | noise mask)."""
    rng = np.random.RandomState(seed)
    nout, raw = voc.featuressize(), voc.featuressizeraw()
    (tmp_path / 'lab').mkdir(); (tmp_path / 'cmp').mkdir()
    fids = ['utt_{:02d}'.format(i) for i in range(len(lens))]
    for fid, n in zip(fids, lens):
        (rng.rand(n, ctx) * 2 - 1).astype(np.float32).tofile(str(tmp_path / 'lab' / (fid + '.lab')))
    mean = (rng.randn(nout) * 0.1).astype(np.float32)
    mean[0], mean[1] = 5.0, -3.0
    std = np.exp(rng.uniform(np.log(0.05), np.log(0.5), size=nout)).astype(np.float32)
    mean.tofile(str(tmp_path / 'cmp' / 'mean4norm.dat')); std.tofile(str(tmp_path / 'cmp' / 'std4norm.dat'))
    return fids, str(tmp_path / 'lab') + '/*.lab:(-1,{})'.format(ctx), str(tmp_path / 'cmp') + '/*.cmp:(-1,{})'.format(nout), raw


@pytest.mark.gpu
@pytest.mark.parametrize('wins', [REF_WINS, None], ids=['mlpg', 'no-windows'])
@pytest.mark.parametrize('spec_type', ['fwbnd', 'mcep'])
def test_generate_params_writes_the_envelopes(spec_type, wins, tmp_path):
    from percivaltts_amd import _hip
    ctx, voc, mod = _model(spec_type, wins)
    lens = [21, 9, 34]
    fids, inpath, outpath, raw = _corpus(tmp_path, ctx, voc, lens)
    K = E2E_DFTLEN // 2 + 1
    spectrum_calls = ('ptts_mcep2spec', 'ptts_fwbnd2spec', 'ptts_mcep_postfilter', 'ptts_mcep_table', 'ptts_fwbnd_table')

    with _hip.KernelTimer() as kt:
        assert mod.generate_params(inpath, outpath, fids, str(tmp_path / 'plain'), do_objmeas=False, batch_size=2) is None
    assert not [r for r in kt.records if r[0] in spectrum_calls]                    # the default launches nothing new
    for pp in (False, True):
        gen, specdir = tmp_path / 'gen{}'.format(int(pp)), tmp_path / 'spec{}'.format(int(pp))
        with _hip.KernelTimer() as kt:
            mod.generate_params(inpath, outpath, fids, str(gen), do_objmeas=False, batch_size=2, pp_mcep=pp, specdir=str(specdir))
        main = 'ptts_fwbnd2spec' if spec_type == 'fwbnd' else 'ptts_mcep2spec'
        assert [r[0] for r in kt.records if r[0] in spectrum_calls and not r[0].endswith('_table')] == [main] * len(fids)
        for fid, n in zip(fids, lens):
            with open(str(gen / (fid + '.cmp')), 'rb') as f, open(str(tmp_path / 'plain' / (fid + '.cmp')), 'rb') as g:
                assert f.read() == g.read()                                         # the parameters do not know about specdir
            cmp_ = np.fromfile(str(gen / (fid + '.cmp')), dtype=np.float32).reshape(n, raw)
            spec = np.fromfile(str(specdir / (fid + '.spec')), dtype=np.float32)
            assert spec.size == n * K
            spec = spec.reshape(n, K)
            cols = cmp_[:, 1:1 + voc.specsize()]
            # what was on the device is what was written: the same kernel on the same numbers
            np.testing.assert_array_equal(voc.decompress_spectrum(cols, pp_mcep=pp), spec)
            if spec_type == 'fwbnd':
                w64, w32 = fwbnd2spec(cols, 16000, E2E_DFTLEN, pp=pp), fwbnd2spec(cols, 16000, E2E_DFTLEN, pp=pp, dtype=np.float32)
            else:
                a = bark_alpha(16000)
                w64, w32 = mcep2spec(cols, a, E2E_DFTLEN, pp=pp), mcep2spec(cols, a, E2E_DFTLEN, pp=pp, dtype=np.float32)
            check(spec, w64, w32, 'rel', '{} {} pp={}'.format(spec_type, fid, int(pp)))
    a = np.fromfile(str(tmp_path / 'spec0' / (fids[0] + '.spec')), dtype=np.float32)
    b = np.fromfile(str(tmp_path / 'spec1' / (fids[0] + '.spec')), dtype=np.float32)
    assert np.abs(a / b - 1.0).max() > 1e-3                                         # the post-filter did something
