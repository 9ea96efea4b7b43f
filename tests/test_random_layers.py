"""Dropout and GaussianNoiseInput on the library's counter-based generator (csrc/random.hip).

The CPU half pins a numpy restatement of Philox4x32-10 against the known-answer vectors of the Random123 distribution and
checks the argument validation of the new entry points; the GPU half compares the kernels, the autograd functions, the
layers, a Generic model and a resumed training run with that restatement."""
import ctypes
import math
import os

import numpy as np
import pytest
import torch

# ---------------------------------------------------------------------------------------------------------------------------
# numpy restatement (uint64 arithmetic masked to 32 bits)
# ---------------------------------------------------------------------------------------------------------------------------
M32 = np.uint64(0xFFFFFFFF)
PH_M0, PH_M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
PH_W0, PH_W1 = np.uint64(0x9E3779B9), np.uint64(0xBB67AE85)
S32 = np.uint64(32)


def philox4x32_10(ctr, key):
    """ctr: four uint64 arrays holding 32-bit words, key: two; returns the four output words (Salmon et al., SC'11)."""
    c0, c1, c2, c3 = [np.asarray(c, dtype=np.uint64) & M32 for c in ctr]
    k0, k1 = [np.asarray(k, dtype=np.uint64) & M32 for k in key]
    for _ in range(10):
        p0, p1 = PH_M0 * c0, PH_M1 * c2            # 32 x 32 -> 64 bits: no overflow in uint64
        hi0, lo0, hi1, lo1 = p0 >> S32, p0 & M32, p1 >> S32, p1 & M32
        c0, c1, c2, c3 = hi1 ^ c1 ^ k0, lo1, hi0 ^ c3 ^ k1, lo0
        k0, k1 = (k0 + PH_W0) & M32, (k1 + PH_W1) & M32
    return c0, c1, c2, c3


def philox_words(index, call, seed):
    """[len(index), 4] words of the library's layout: counter = (index lo, index hi, call lo, call hi), key = (seed lo, seed hi)."""
    index = np.asarray(index, dtype=np.uint64)
    call, seed = np.uint64(call), np.uint64(seed)
    w = philox4x32_10((index & M32, index >> S32, call & M32, call >> S32), (seed & M32, seed >> S32))
    return np.stack([np.broadcast_to(x, index.shape) for x in w], axis=-1)


def u24(w):
    return (np.asarray(w, dtype=np.uint64) >> np.uint64(8)).astype(np.int64)


def dropout_mask(seed, call, B, D, rate, b0=0):
    """bool [B, D]: word d & 3 of block (b0 + b) * ceil(D/4) + (d >> 2); kept where float32(w >> 8) * 2^-24 < 1 - rate in fp32."""
    DG = (D + 3) // 4
    idx = (np.arange(B, dtype=np.uint64)[:, None] + np.uint64(b0)) * np.uint64(DG) + np.arange(DG, dtype=np.uint64)[None, :]
    w = philox_words(idx.reshape(-1), call, seed).reshape(B, DG * 4)[:, :D]
    u = u24(w).astype(np.float32) * np.float32(2.0 ** -24)
    return u < (np.float32(1) - np.float32(rate))


def inv_keep(rate):
    return np.float32(1) / (np.float32(1) - np.float32(rate))


def normal_restatement(seed, call, n, stddev, i0=0, dtype=np.float64):
    """Box-Muller on the word pairs (0, 1) and (2, 3) of block e >> 2 for element e = i0 + i, in `dtype` arithmetic."""
    kb = np.arange(i0 >> 2, ((i0 + n - 1) >> 2) + 1, dtype=np.uint64)
    w = philox_words(kb, call, seed)
    f = dtype
    z = np.empty((kb.size, 4), dtype=f)
    for h in range(2):
        u1 = (u24(w[:, 2 * h]) + 1).astype(f) * f(2.0 ** -24)
        u2 = u24(w[:, 2 * h + 1]).astype(f) * f(2.0 ** -24)
        r = f(stddev) * np.sqrt(f(-2) * np.log(u1))
        ang = f(2 * math.pi) * u2
        z[:, 2 * h], z[:, 2 * h + 1] = r * np.cos(ang), r * np.sin(ang)
    lo = i0 - 4 * (i0 >> 2)
    return z.reshape(-1)[lo:lo + n]


MASK_CASES = [(3, 7, 5), (16, 20, 256), (5, 33, 70), (64, 400, 256), (2, 9, 1100)]
RATES = [0.2, 0.5]
SEED = 20240607
NOISE_N = 64 * 400 * 100


def kept_fraction_bound(rate, B, D):
    return 6.0 * math.sqrt(rate * (1.0 - rate) / (B * D))


# ---------------------------------------------------------------------------------------------------------------------------
# CPU
# ---------------------------------------------------------------------------------------------------------------------------
def test_numpy_philox_reproduces_the_random123_known_answers():
    """kat_vectors of the Random123 distribution, philox4x32 with 10 rounds: counter and key all zero, all ones, and the digits of pi."""
    kat = [((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
           ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
           ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1))]
    for ctr, key, want in kat:
        got = tuple(int(x) for x in philox4x32_10(ctr, key))
        assert got == want, (ctr, key, [hex(g) for g in got])
    # the library's word layout is the same function
    w = philox_words([0x85a308d3243f6a88], 0x0370734413198a2e, 0x299f31d0a4093822)
    assert tuple(int(x) for x in w[0]) == kat[2][2]


def test_entry_points_reject_bad_arguments():
    """PTTS_EINVAL before any launch (the pointers are never dereferenced on the host): null pointers, B, T, D < 1, rate outside
    [0, 1), stddev < 0, an unknown input mode."""
    from percivaltts_amd import _hip
    if not os.path.exists(_hip.LIB_PATH):
        pytest.skip('libpercival_hip.so not built (run __graft_entry__.build())')
    lib = _hip.lib()
    p = ctypes.c_void_p(256)           # non-null, never read
    EINVAL = -1
    fwd = lambda x=p, sc=None, sh=None, y=p, st=p, used=p, rate=0.2, alpha=0.3, mode=0, B=2, T=3, D=4, b0=0: \
        lib.ptts_dropout_fwd(x, sc, sh, y, st, used, rate, alpha, mode, B, T, D, b0, None)
    bwd = lambda dy=p, da=p, used=p, st=p, rate=0.2, B=2, T=3, D=4, b0=0: lib.ptts_dropout_bwd(dy, da, used, st, rate, B, T, D, b0, None)
    fill = lambda out=p, st=p, used=p, stddev=1.0, i0=0, n=8: lib.ptts_normal_fill(out, st, used, stddev, i0, n, None)
    for kw in (dict(x=None), dict(y=None), dict(st=None), dict(used=None), dict(B=0), dict(T=0), dict(D=0), dict(rate=-0.1),
               dict(rate=1.0), dict(rate=1.5), dict(rate=float('nan')), dict(mode=2), dict(mode=-1), dict(mode=7), dict(sc=p), dict(sh=p),
               dict(sc=p, sh=p, mode=0), dict(b0=-1)):
        assert fwd(**kw) == EINVAL, kw
    for kw in (dict(dy=None), dict(da=None), dict(used=None), dict(st=None), dict(B=0), dict(T=-1), dict(D=0), dict(rate=-0.5),
               dict(rate=1.0), dict(b0=-2)):
        assert bwd(**kw) == EINVAL, kw
    for kw in (dict(out=None), dict(st=None), dict(used=None), dict(stddev=-1.0), dict(stddev=float('nan')), dict(n=0), dict(i0=-4)):
        assert fill(**kw) == EINVAL, kw
    assert 'normal_fill' in _hip.last_error()
    assert lib.ptts_rng_seed(None, 1, 0, None) == EINVAL
    out = (ctypes.c_ulonglong * 2)()
    assert lib.ptts_rng_state_get(None, ctypes.cast(out, ctypes.c_void_p), None) == EINVAL
    assert lib.ptts_rng_state_get(p, None, None) == EINVAL


def test_restatement_meets_the_statistical_bounds():
    """The bounds the GPU tests assert follow from the binomial variance (kept fraction: 6 sigma of a mean of B*D Bernoulli draws) and
    from the normal distribution's moments (mean: 6 stddev / sqrt(n); variance: 6 stddev^2 sqrt(2 / n)).  The restatement itself must
    meet them for the seeds and call counters the GPU tests use."""
    for (B, T, D) in MASK_CASES:
        for ri, rate in enumerate(RATES):
            m = dropout_mask(SEED, 3 + ri, B, D, rate)
            assert abs(m.mean() - (1.0 - rate)) <= kept_fraction_bound(rate, B, D), (B, D, rate, m.mean())
    for stddev in (1.0, 0.37):
        z = normal_restatement(SEED, 5, NOISE_N, stddev)
        assert np.isfinite(z).all()
        assert abs(z.mean()) <= 6.0 * stddev / math.sqrt(NOISE_N)
        assert abs(z.var() - stddev ** 2) <= 6.0 * stddev ** 2 * math.sqrt(2.0 / NOISE_N)


def fp32_restatement_error(stddev, n=NOISE_N):
    z64 = normal_restatement(SEED, 5, n, stddev)
    z32 = normal_restatement(SEED, 5, n, stddev, dtype=np.float32)
    assert z32.dtype == np.float32
    return float(np.abs(z32.astype(np.float64) - z64).max())


def test_fp32_restatement_error_is_what_the_noise_tolerance_assumes():
    """Largest |fp32 - fp64| of the Box-Muller restatement over the 2.56 M values of the GPU test, stddev 1: measured 1.7e-6 (numpy
    2.2, x86-64).  The GPU test recomputes it and allows four times as much."""
    e = fp32_restatement_error(1.0)
    print('fp32 Box-Muller restatement: max abs error {:.3e}'.format(e))
    assert 1e-7 < e < 5e-6


# ---------------------------------------------------------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------------------------------------------------------
gpu = pytest.mark.gpu


def close(got, want, rtol=1e-4, atol=1e-5, what=''):
    """|got - want| <= atol + rtol |want| elementwise, want in fp64 (the helper of tests/test_ops_gpu.py, same defaults)."""
    got = torch.as_tensor(got).detach().cpu().to(torch.float64)
    want = torch.as_tensor(want).detach().cpu().to(torch.float64)
    assert got.shape == want.shape, '{}: shape {} vs {}'.format(what, tuple(got.shape), tuple(want.shape))
    err = (got - want).abs()
    bad = err > atol + rtol * want.abs()
    assert not bad.any(), '{}: {} / {} mismatches, worst |err| {:.3e}, max |want| {:.3e}'.format(
        what, int(bad.sum()), bad.numel(), float(err.max()), float(want.abs().max()))


@pytest.fixture
def ops():
    from percivaltts_amd import ops as _ops
    return _ops


def _seed(ops, seed=SEED, call=0):
    ops.rng_seed(seed, call, device=torch.device('cuda', torch.cuda.current_device()))


def _raw_dropout(ops, x, rate, b0=0, scale=None, shift=None, mode=0, alpha=0.3):
    from percivaltts_amd import _hip
    B, T, D = x.shape
    y = torch.full_like(x, float('nan'))
    used = torch.full((1,), -1, dtype=torch.int64, device=x.device)
    st = ops._RNG.state(x.device)
    _hip.call('ptts_dropout_fwd', _hip.ptr(x), _hip.ptr(scale), _hip.ptr(shift), _hip.ptr(y), _hip.ptr(st), _hip.ptr(used), rate, alpha,
              mode, B, T, D, b0, _hip.stream())
    return y, used


@gpu
@pytest.mark.parametrize('rate', RATES)
@pytest.mark.parametrize('shape', MASK_CASES)
def test_dropout_mask_is_exact_and_shared_along_time(ops, shape, rate):
    B, T, D = shape
    call = 3 + RATES.index(rate)
    _seed(ops, SEED, call)
    y, used = _raw_dropout(ops, torch.ones(B, T, D, device='cuda'), rate)
    assert int(used.item()) == call and ops.rng_state() == (SEED, call + 1)
    m = dropout_mask(SEED, call, B, D, rate)
    want = np.where(m, inv_keep(rate), np.float32(0)).astype(np.float32)
    got = y.cpu().numpy()
    assert np.array_equal(got, np.broadcast_to(want[:, None, :], (B, T, D)))        # bit for bit, constant along t
    frac = float((got[:, 0, :] != 0).mean())
    print('kept fraction {:.5f} (1 - rate = {}), bound {:.5f}'.format(frac, 1 - rate, kept_fraction_bound(rate, B, D)))
    assert abs(frac - (1.0 - rate)) <= kept_fraction_bound(rate, B, D)
    # the backward kernel regenerates the same mask from `used`, whatever the live counter has become
    from percivaltts_amd import _hip
    dy = torch.randn(B, T, D, device='cuda')
    da = torch.empty_like(dy)
    _hip.call('ptts_dropout_bwd', _hip.ptr(dy), _hip.ptr(da), _hip.ptr(used), _hip.ptr(ops._RNG.state(dy.device)), rate, B, T, D, 0,
              _hip.stream())
    assert np.array_equal(da.cpu().numpy(), dy.cpu().numpy() * want[:, None, :])


@gpu
@pytest.mark.parametrize('affine', [True, False])
@pytest.mark.parametrize('shape', [(6, 50, 256), (3, 11, 70)])
def test_dropout_fuses_a_pending_activation(ops, shape, affine):
    """Lazy(z, scale, shift, lrelu) input: the output is dropout(affine_act(z, ...)) bit for bit under the same call counter, without
    a ptts_affine_act launch; gradients against fp64 at the tolerances of tests/test_ops_gpu.py::test_affine_act_bwd_wide."""
    from percivaltts_amd import _hip
    B, T, D = shape
    rate, call = 0.2, 11
    g = torch.Generator().manual_seed(21)
    z = torch.randn(B, T, D, generator=g, dtype=torch.float64)
    sc = (torch.rand(D, generator=g, dtype=torch.float64) + 0.5) if affine else None
    sh = torch.randn(D, generator=g, dtype=torch.float64) if affine else None
    dy = torch.randn(B, T, D, generator=g, dtype=torch.float64)
    dev = lambda t, grad=False: None if t is None else t.to(torch.float32).cuda().contiguous().requires_grad_(grad)
    zd, scd, shd = dev(z, True), dev(sc, True), dev(sh, True)
    _seed(ops, SEED, call)
    with _hip.KernelTimer() as kt:
        y = ops.dropout(ops.Lazy(zd, scd, shd, lrelu=True, alpha=0.3), rate)
    names = [r[0] for r in kt.records]
    assert names == ['ptts_dropout_fwd'], names                    # no ptts_affine_act forward launch
    _seed(ops, SEED, call)
    with torch.no_grad():
        a = ops.affine_act(zd.detach(), None if scd is None else scd.detach(), None if shd is None else shd.detach(), 'lrelu', 0.3)
        y2 = ops.dropout(a, rate)
    assert torch.equal(y, y2)
    m = torch.from_numpy(dropout_mask(SEED, call, B, D, rate).astype(np.float64))[:, None, :] / (1.0 - float(np.float32(rate)))
    zr = z.clone().requires_grad_(True)
    scr, shr = (sc.clone().requires_grad_(True), sh.clone().requires_grad_(True)) if affine else (None, None)
    p = zr * scr + shr if affine else zr
    yr = torch.where(p > 0, p, 0.3 * p) * m
    close(y, yr, what='y')
    yr.backward(dy)
    y.backward(dev(dy))
    close(zd.grad, zr.grad, what='dz')
    if affine:
        close(scd.grad, scr.grad, rtol=2e-4, atol=2e-3, what='dscale')
        close(shd.grad, shr.grad, rtol=2e-4, atol=2e-3, what='dshift')
    # a plain tensor input (no activation pending)
    _seed(ops, SEED, call)
    xd = dev(z, True)
    y3 = ops.dropout(xd, rate)
    close(y3, z * m, what='y plain')
    y3.backward(dev(dy))
    close(xd.grad, dy * m, what='dx plain')


@gpu
def test_dropout_of_a_sharded_batch_draws_the_whole_batch_masks(ops):
    B, T, D, rate = 8, 13, 36, 0.5
    x = torch.randn(B, T, D, device='cuda')
    _seed(ops, SEED, 7)
    whole = ops.dropout(x, rate, b0=0)
    halves = []
    for r in range(2):
        _seed(ops, SEED, 7)                  # every rank's generator is at the same call
        halves.append(ops.dropout(x[r * B // 2:(r + 1) * B // 2].contiguous(), rate, b0=r * B // 2))
    assert torch.equal(torch.cat(halves, 0), whole)
    assert not torch.equal(halves[0] != 0, halves[1] != 0)
    # the noise of a sharded batch: disjoint parts of one sequence
    n = 5 * 7 * 6
    _seed(ops, SEED, 7)
    allz = ops.normal((2, 5, 7, 6), 1.0, i0=0)
    parts = []
    for r in range(2):
        _seed(ops, SEED, 7)
        parts.append(ops.normal((5, 7, 6), 1.0, i0=r * n))      # n = 210: the second rank starts inside a Philox block
    assert torch.equal(torch.stack(parts, 0), allz)


@gpu
def test_normal_fill_matches_box_muller_and_the_normal_moments(ops):
    """Against the fp64 Box-Muller restatement from the same Philox words.  Tolerance: four times the largest absolute error of the
    numpy fp32 restatement against the fp64 one (measured 1.7e-6 at stddev 1 over these 2.56 M values; the device's log / sincos may
    differ from numpy's by a few ulp), scaled by stddev."""
    e32 = fp32_restatement_error(1.0)
    for stddev, call in ((1.0, 5), (0.37, 5)):
        _seed(ops, SEED, call)
        z = ops.normal((64, 400, 100), stddev)
        assert ops.rng_state() == (SEED, call + 1)
        got = z.cpu().numpy().astype(np.float64).reshape(-1)
        want = normal_restatement(SEED, call, NOISE_N, stddev)
        err = float(np.abs(got - want).max())
        print('stddev {}: max abs error {:.3e}, allowed {:.3e} (fp32 restatement {:.3e})'.format(stddev, err, 4 * e32 * stddev, e32))
        assert np.isfinite(got).all()
        assert err <= 4 * e32 * stddev
        assert abs(got.mean()) <= 6.0 * stddev / math.sqrt(NOISE_N)
        assert abs(got.var() - stddev ** 2) <= 6.0 * stddev ** 2 * math.sqrt(2.0 / NOISE_N)
    # odd length, unaligned start
    _seed(ops, SEED, 9)
    z = ops.normal((1, 3, 7), 2.0, i0=6)
    np.testing.assert_allclose(z.cpu().numpy().reshape(-1), normal_restatement(SEED, 9, 21, 2.0, i0=6), rtol=0, atol=4 * e32 * 2.0)
    z0 = ops.normal((3, 50, 9), 0.0)
    assert (z0 == 0).all()


def _generic(H=16, ctx=31):
    import percivaltts_amd
    from percivaltts_amd import vocoders, modeltts_common
    cfg = percivaltts_amd.configuration()
    cfg.arch_hiddenwidth = H
    cfg.train_batch_size = 3
    voc = vocoders.VocoderPML(16000, 0.005, 9, 3)
    np.random.seed(4)
    model = modeltts_common.Generic(ctx, voc, layertypes=['FC', 'DO', 'FC', ['RND', 8], 'FC'], cfgarch=cfg)
    return cfg, voc, model


def _compose(model, X, training, mask, noise):
    """fp64 torch composition of Generic(['FC', 'DO', 'FC', ['RND', 8], 'FC']) + the PML heads from the model's weights."""
    from percivaltts_amd import layers as kl
    a = torch.as_tensor(X, dtype=torch.float64)
    outs = []
    for lay in model.kerasmodel.layers_list:
        p = {k: v.detach().cpu().double() for k, v in lay.weights()}
        if isinstance(lay, kl.Dense):
            if lay.lname in ('lo_f0spec', 'lo_nm'):
                o = a @ p['kernel'] + p['bias']
                outs.append(torch.sigmoid(o) if lay.activation == 'sigmoid' else o)
            else:
                a = a @ p['kernel'] + (p['bias'] if 'bias' in p else 0.0)
        elif isinstance(lay, kl.BatchNormalization):
            if training:
                mu, var = a.mean((0, 1)), a.var((0, 1), unbiased=False)
            else:
                mu, var = p['moving_mean'], p['moving_variance']
            a = (a - mu) / torch.sqrt(var + 1e-3) * p['gamma'] + p['beta']
        elif isinstance(lay, kl.LeakyReLU):
            a = torch.where(a > 0, a, 0.3 * a)
        elif isinstance(lay, kl.Dropout):
            if training:
                a = a * mask
        elif isinstance(lay, kl.GaussianNoiseInput):
            a = torch.cat([a, noise], -1)
        elif isinstance(lay, kl.Concatenate):
            pass
        else:
            raise AssertionError('unexpected layer ' + type(lay).__name__)
    return torch.cat(outs, -1)


@gpu
def test_generic_model_with_dropout_and_noise_layers(ops, monkeypatch):
    """Training-mode forward against a torch composition with the restatement's mask and noise (the Dense-stack tolerance of
    tests/test_model_gpu.py: rtol 5e-4, atol 5e-5); predict leaves Dropout out and still adds noise; no concatenation of RND's
    input is made in front of the Dense layer; an LSE Adam step lowers the cost."""
    from percivaltts_amd import _hip, backend_hip, optimizertts
    cfg, voc, model = _generic()
    B, T, H, W, ctx = 3, 21, 16, 8, 31
    rng = np.random.RandomState(0)
    X = (rng.rand(B, T, ctx) * 2 - 1).astype(np.float32)
    dev = model.to_device()
    rate = [l for l in model.kerasmodel.layers_list if type(l).__name__ == 'Dropout'][0].rate
    assert rate == 0.2
    cats = []
    orig_cat = torch.cat
    monkeypatch.setattr(torch, 'cat', lambda ts, *a, **k: (cats.append([tuple(t.shape) for t in ts]), orig_cat(ts, *a, **k))[1])
    backend_hip.set_random_seed(77)
    with _hip.KernelTimer() as kt:
        with torch.no_grad():
            y = model.kerasmodel(torch.as_tensor(X).to(dev), training=True)
    monkeypatch.setattr(torch, 'cat', orig_cat)
    names = [r[0] for r in kt.records]
    assert names.count('ptts_dropout_fwd') == 1 and names.count('ptts_normal_fill') == 1, names
    # neither layer's input is materialised: the one activation pass of the model is the sigmoid of the noise-mask head, behind them
    assert 'ptts_affine_act' not in names[:names.index('ptts_normal_fill')] and names.count('ptts_affine_act') == 1, names
    prods = [r[1] for r in kt.records if r[0] in ('ptts_gemm', 'ptts_dense_bf16x6', 'ptts_dense_bf16x6_stats', 'ptts_dense_bf16x6_res')]
    ks = sorted(t[2] for t in prods)
    assert H + W not in ks and W in ks, ks               # RND's consumer: one product per part, none over the concatenated width
    assert cats and not any(sum(sh[-1] for sh in c) == H + W for c in cats), cats      # (the output heads are concatenated, nothing else)
    mask = torch.from_numpy(dropout_mask(77, 0, B, H, rate).astype(np.float64))[:, None, :] / (1.0 - float(np.float32(rate)))
    noise = torch.from_numpy(normal_restatement(77, 1, B * T * W, 1.0)).view(B, T, W)
    close(y, _compose(model, X, True, mask, noise), 5e-4, 5e-5, 'training forward')
    # inference: no Dropout launch, noise still drawn (call 0 after the seed)
    backend_hip.set_random_seed(78)
    with _hip.KernelTimer() as kt:
        yp = model.predict(X)
    names = [r[0] for r in kt.records]
    assert 'ptts_dropout_fwd' not in names and names.count('ptts_normal_fill') == 1
    noise = torch.from_numpy(normal_restatement(78, 0, B * T * W, 1.0)).view(B, T, W)
    close(torch.from_numpy(yp), _compose(model, X, False, None, noise), 5e-4, 5e-5, 'predict')
    backend_hip.set_random_seed(79)
    assert not np.array_equal(model.predict(X), yp)
    # one LSE optimiser on the model: the cost goes down
    opt = optimizertts.OptimizerTTS(cfg, model)
    opt.prepare()
    Y = rng.randn(B, T, voc.featuressize()).astype(np.float32)
    c0 = opt.train_on_batch(0, X, Y)
    for i in range(30):
        c = opt.train_on_batch(i + 1, X, Y)
    print('LSE cost {:.5f} -> {:.5f}'.format(c0, c))
    assert np.isfinite(c0) and np.isfinite(c) and c < c0


@gpu
def test_seeds_calls_and_layers_draw_reproducibly(ops):
    from percivaltts_amd import backend_hip
    cfg, voc, model = _generic()
    dev = model.to_device()
    X = torch.as_tensor((np.random.RandomState(1).rand(3, 17, 31) * 2 - 1).astype(np.float32)).to(dev)
    run = lambda: model.kerasmodel(X, training=True).detach().cpu().numpy()
    with torch.no_grad():
        backend_hip.set_random_seed(5); a1 = run(); a2 = run()
        backend_hip.set_random_seed(5); b1 = run()
        backend_hip.set_random_seed(6); c1 = run()
    assert np.array_equal(a1, b1) and not np.array_equal(a1, a2) and not np.array_equal(a1, c1)
    # two Dropout layers of one model, and two successive calls of one: different masks
    from percivaltts_amd import layers as kl
    l_in = kl.Input(shape=(None, 64))
    model2 = kl.Model(inputs=l_in, outputs=kl.Dropout(0.5)(kl.Dropout(0.5)(l_in))).to(dev)
    x = torch.ones(4, 5, 64, device=dev)
    backend_hip.set_random_seed(5)
    y = model2(x, training=True).cpu().numpy()[:, 0, :]
    m0, m1 = dropout_mask(5, 0, 4, 64, 0.5), dropout_mask(5, 1, 4, 64, 0.5)
    assert np.array_equal(y, np.where(m0 & m1, np.float32(4), np.float32(0)))
    assert not np.array_equal(m0, m1)
    y2 = model2(x, training=True).cpu().numpy()[:, 0, :]
    assert np.array_equal(y2, np.where(dropout_mask(5, 2, 4, 64, 0.5) & dropout_mask(5, 3, 4, 64, 0.5), np.float32(4), np.float32(0)))
    assert torch.equal(model2(x, training=False), x)                  # inference: the input, unchanged


@gpu
def test_captured_graph_draws_fresh_masks_and_backward_sees_its_own(ops):
    B, T, D, rate = 6, 9, 64, 0.5
    _seed(ops, SEED, 0)
    x = (torch.rand(B, T, D, device='cuda') + 0.5).requires_grad_(True)
    gy = torch.rand(B, T, D, device='cuda') + 0.5
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(3):
            y = ops.dropout(x, rate)
            torch.autograd.grad(y, x, gy)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    call0 = ops.rng_state()[1]
    assert call0 == 3
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        y = ops.dropout(x, rate)
        (dx,) = torch.autograd.grad(y, x, gy)
    seen = []
    for rep in range(2):
        graph.replay()
        torch.cuda.synchronize()
        yh, dxh = y.detach().cpu().numpy(), dx.detach().cpu().numpy()
        assert np.array_equal(dxh == 0, yh == 0)                         # the backward pass used the mask of ITS forward pass
        m = dropout_mask(SEED, call0 + rep, B, D, rate)
        assert np.array_equal(yh != 0, np.broadcast_to(m[:, None, :], (B, T, D)))
        seen.append(yh != 0)
    assert not np.array_equal(seen[0], seen[1])
    assert ops.rng_state()[1] == call0 + 2


@gpu
def test_resumed_run_with_dropout_and_noise_reproduces_the_uninterrupted_one(tmp_path, monkeypatch):
    """tests/test_run_synthetic.py's pattern on a Generic model with a DO and an RND layer under the LSE optimiser, deterministic mode:
    4 epochs straight against 2 epochs + a resumed run of 2 more started from OTHER seeds end with the same weights and optimiser
    state bit for bit -- the training state carries the library generator's {seed, call counter}."""
    import importlib, pickle
    from percivaltts_amd import ops, backend_hip, modeltts_common
    monkeypatch.setenv('PERCIVAL_CORPUS', str(tmp_path / 'corpus'))
    import percivaltts_amd.run as run
    ops.deterministic(True)
    try:
        states = {}
        for name, plan in (('straight', [(4, False)]), ('resumed', [(2, False), (4, True)])):
            wd = tmp_path / name
            wd.mkdir()
            monkeypatch.chdir(wd)
            run = importlib.reload(run)
            run.errtype = 'LSE'
            run.build_model = lambda: modeltts_common.Generic(run.ctxsize, run.vocoder, layertypes=['FC', 'DO', 'FC', ['RND', 8], 'FC'],
                                                              cfgarch=run.cfg)
            run.cfg.id_valid_start = 8; run.cfg.id_valid_nb = 1; run.cfg.id_test_nb = 1
            run.cfg.train_min_nbepochs = 1; run.cfg.train_cancel_nodecepochs = 10
            run.cfg.train_nbepochs_scalewdata = False
            run.cfg.train_batch_size = 2; run.cfg.arch_hiddenwidth = 8
            run.cfg.train_batch_lengthmax = 60
            if not os.path.exists(run.cfg.fileids):
                run.synthesize_corpus(nfiles=10, minlen=90, maxlen=140)
            for (nep, cont) in plan:
                backend_hip.set_random_seed(999 if cont else 123)      # a resumed run must not depend on the fresh seeds
                run.cfg.train_max_nbepochs = nep
                run.training(cont=cont)
            st = 'model-trainingstate-last.h5'
            with open(st + '.model.cfgextras.pkl', 'rb') as f:
                _, extras, _ = pickle.load(f)
            states[name] = {k: dict(np.load(st + k)) for k in ('.model.weights.npz', '.optimizer.npz')}
            states[name]['extras'] = extras
    finally:
        ops.deterministic(False)
    a, b = states['straight'], states['resumed']
    assert a['extras']['epoch'] == b['extras']['epoch'] == 4
    assert a['extras']['ptts_rng'] == b['extras']['ptts_rng'] and a['extras']['ptts_rng'][0] == 123 and a['extras']['ptts_rng'][1] > 8
    for part in ('.model.weights.npz', '.optimizer.npz'):
        assert sorted(a[part]) == sorted(b[part])
        for k in a[part]:
            assert np.array_equal(a[part][k], b[part][k]), part + ':' + k
