"""Ragged inference on the GPU: a zero-padded batch with a length per row (csrc/lstm.hip ptts_lstm_fwd_ragged, csrc/gru.hip
ptts_gru_fwd_ragged, csrc/elementwise.hip ptts_affine_act_rows; layers.ragged_input; ModelTTS.predict_batch;
generate_params(predict_batched=True)).  tests/test_ragged_rule.py shows in float64 why masking the convolutions' inputs and
walking the recurrences per row is enough.

The recurrence kernels are held to the dense entry point run on each row ALONE (B = 1, T = lens[b]) bit for bit: a row's MFMA
products and the fixed-order sum over the four waves do not depend on the other rows of the tile, and the scalar kernel's fma
chain is per lane.  Pad frames are exactly 0.0f; the output buffers start as NaN, so a frame no step wrote would show.  The
model is held to the oracle's lone forward under tests/test_model_gpu.py's own bound for predict."""
import math

import numpy as np
import pytest
import torch

from oracle import percival_oracle as O

import test_gru as tg
import test_lstm as tl
import test_model_gpu as tm
import test_ragged_rule as rr

pytestmark = pytest.mark.gpu

T = 12
LENS = {17: [12, 11, 2, 1, 5, 7, 12, 3, 9, 1, 6, 12, 4, 8, 10, 2, 11],      # the second sample tile holds one valid row
        3: [11, 1, 12]}


def _dev(t):
    return t.to(torch.float32).cuda().contiguous()


def _nan(*shape):
    return torch.full(shape, float('nan'), dtype=torch.float32, device='cuda')


def _bytes_equal(got, want, what):
    assert got.shape == want.shape, what
    same = got.contiguous().view(torch.int32) == want.contiguous().view(torch.int32)
    assert bool(same.all()), '{}: {} of {} values differ in their bytes'.format(what, int((~same).sum()), same.numel())


def _exact_zero(t, what):
    assert bool((t.contiguous().view(torch.int32) == 0).all()), '{}: pad frames are not +0.0f'.format(what)


# ---------------------------------------------------------------------------------------------------------------------------
# 3: the recurrence kernels
# ---------------------------------------------------------------------------------------------------------------------------
def _lstm_dense(xproj, U, nd, reverse):
    from percivaltts_amd import _hip
    B, Tn, H = xproj.shape[0], xproj.shape[1], U.shape[1]
    h, c, gates = _nan(B, Tn, nd * H), _nan(B, Tn, nd * H), _nan(B, Tn, nd * 4 * H)
    ws = torch.empty(max(_hip.lib().ptts_lstm_fwd_workspace_bytes(B, Tn, H, nd), 16), dtype=torch.uint8, device='cuda')
    _hip.call('ptts_lstm_fwd', _hip.ptr(xproj), _hip.ptr(U), _hip.ptr(h), _hip.ptr(gates), _hip.ptr(c), _hip.ptr(ws), ws.numel(),
              B, Tn, H, nd, int(reverse), None)
    return h


def _lstm_ragged(xproj, U, lens, nd, reverse):
    from percivaltts_amd import _hip
    B, Tn, H = xproj.shape[0], xproj.shape[1], U.shape[1]
    h = _nan(B, Tn, nd * H)
    carry = (nd * B * H * 4 + 255) // 256 * 256
    ws = torch.empty(carry + max(_hip.lib().ptts_lstm_fwd_workspace_bytes(B, Tn, H, nd), 16), dtype=torch.uint8, device='cuda')
    _hip.call('ptts_lstm_fwd_ragged', _hip.ptr(xproj), _hip.ptr(U), _hip.ptr(h), None, None, _hip.ptr(lens), _hip.ptr(ws),
              ws.numel(), B, Tn, H, nd, int(reverse), None)
    return h


@pytest.mark.parametrize('nd,reverse', [(2, False), (1, False), (1, True)])
@pytest.mark.parametrize('H', [64, 192, 128, 256, 48, 16, 5])     # packed <4>, <4>, <8>, <16>; MFMA partial chunk, one k-step; scalar
def test_lstm_ragged_is_each_row_alone(H, nd, reverse):
    g = torch.Generator().manual_seed(100 + H)
    for B in (17, 3):
        xproj64 = torch.randn(B, T, nd * 4 * H, generator=g, dtype=torch.float64)
        U64 = torch.randn(nd, H, 4 * H, generator=g, dtype=torch.float64) / math.sqrt(H)
        xproj, U = _dev(xproj64), _dev(U64)
        eye, zero = torch.eye(nd * 4 * H, dtype=torch.float64), torch.zeros(nd * 4 * H, dtype=torch.float64)
        tag = 'H={} nd={} reverse={} B={}'.format(H, nd, reverse, B)
        for lens in (LENS[B], [T] * B):
            ld = torch.tensor(lens, dtype=torch.int32, device='cuda')
            h = _lstm_ragged(xproj, U, ld, nd, reverse)
            torch.cuda.synchronize()
            assert not bool(torch.isnan(h).any()), tag + ': a frame was never written'
            worst = 0.0
            for b, n in enumerate(lens):
                alone = _lstm_dense(xproj[b:b + 1, :n].contiguous(), U, nd, reverse)
                _bytes_equal(h[b, :n], alone[0], '{} row {} (len {})'.format(tag, b, n))
                _exact_zero(h[b, n:], '{} row {}'.format(tag, b))
                # x = the projection itself through an identity kernel: test_lstm.py's fp64 loop on the fp32 operands
                want = tl.lstm_states(xproj[b:b + 1, :n].cpu().double(), eye, U.cpu().double(), zero, reverse=reverse)[0][0]
                err = (h[b, :n].cpu().double() - want).abs()
                tol = tl.H_TOL[1] + tl.H_TOL[0] * want.abs()
                worst = max(worst, float((err / tol).max()))
                assert bool((err <= tol).all()), '{} row {}: fp64 worst err/tol {:.3f}'.format(tag, b, float((err / tol).max()))
            print('{} lens {}: bit-equal to each row alone; fp64 worst err/tol {:.4f}'.format(tag, 'ragged' if lens is LENS[B] else 'full', worst))
            if lens == [T] * B:
                _bytes_equal(h, _lstm_dense(xproj, U, nd, reverse), tag + ' all lengths T against ptts_lstm_fwd')


def test_lstm_ragged_stores_gates_and_cells_where_given():
    """gates and c_out are optional; given, they hold on the real frames what ptts_lstm_fwd keeps for the row alone."""
    from percivaltts_amd import _hip
    H, nd, B = 64, 2, 3
    g = torch.Generator().manual_seed(7)
    xproj = _dev(torch.randn(B, T, nd * 4 * H, generator=g, dtype=torch.float64))
    U = _dev(torch.randn(nd, H, 4 * H, generator=g, dtype=torch.float64) / math.sqrt(H))
    lens = LENS[B]
    ld = torch.tensor(lens, dtype=torch.int32, device='cuda')
    h, c, gates = _nan(B, T, nd * H), _nan(B, T, nd * H), _nan(B, T, nd * 4 * H)
    carry = (nd * B * H * 4 + 255) // 256 * 256
    ws = torch.empty(carry + _hip.lib().ptts_lstm_fwd_workspace_bytes(B, T, H, nd), dtype=torch.uint8, device='cuda')
    _hip.call('ptts_lstm_fwd_ragged', _hip.ptr(xproj), _hip.ptr(U), _hip.ptr(h), _hip.ptr(gates), _hip.ptr(c), _hip.ptr(ld),
              _hip.ptr(ws), ws.numel(), B, T, H, nd, 0, None)
    for b, n in enumerate(lens):
        xb = xproj[b:b + 1, :n].contiguous()
        h1, c1, g1 = _nan(1, n, nd * H), _nan(1, n, nd * H), _nan(1, n, nd * 4 * H)
        _hip.call('ptts_lstm_fwd', _hip.ptr(xb), _hip.ptr(U), _hip.ptr(h1), _hip.ptr(g1), _hip.ptr(c1), _hip.ptr(ws[carry:]),
                  ws.numel() - carry, 1, n, H, nd, 0, None)
        _bytes_equal(h[b, :n], h1[0], 'h'); _bytes_equal(c[b, :n], c1[0], 'c'); _bytes_equal(gates[b, :n], g1[0], 'gates')
    # a workspace without room for the carry is refused before any launch
    assert _hip.lib().ptts_lstm_fwd_ragged(_hip.ptr(xproj), _hip.ptr(U), _hip.ptr(h), None, None, _hip.ptr(ld), _hip.ptr(ws),
                                           carry - 1, B, T, H, nd, 0, None) == -3


def _gru_call(name, xproj, U, nd, lens=None):
    from percivaltts_amd import _hip
    B, Tn, H = xproj.shape[0], xproj.shape[1], U.shape[1]
    h = _nan(B, Tn, nd * H)
    nws = _hip.lib().ptts_gru_fwd_workspace_bytes(B, Tn, H, nd)
    if lens is None:
        gates, rh = _nan(B, Tn, nd * 3 * H), _nan(B, Tn, nd * H)
        ws = torch.empty(nws, dtype=torch.uint8, device='cuda')
        _hip.call(name, _hip.ptr(xproj), _hip.ptr(U), _hip.ptr(h), _hip.ptr(gates), _hip.ptr(rh), _hip.ptr(ws), ws.numel(), B, Tn, H,
                  nd, None)
    else:
        ws = torch.empty(nws + 2 * nd * B * H * 4, dtype=torch.uint8, device='cuda')
        _hip.call(name, _hip.ptr(xproj), _hip.ptr(U), _hip.ptr(h), None, None, _hip.ptr(lens), _hip.ptr(ws), ws.numel(), B, Tn, H,
                  nd, None)
    return h


@pytest.mark.parametrize('nd', [2, 1])
@pytest.mark.parametrize('H', [5, 16, 40])
def test_gru_ragged_is_each_row_alone(H, nd):
    g = torch.Generator().manual_seed(200 + H)
    for B in (17, 3):
        xproj = _dev(torch.randn(B, T, nd * 3 * H, generator=g, dtype=torch.float64))
        U = _dev(torch.randn(nd, H, 3 * H, generator=g, dtype=torch.float64) / math.sqrt(H))
        # x = the projection itself; W[d] picks direction d's columns: test_gru.py's fp64 restatement on the fp32 operands
        W = torch.zeros(nd, nd * 3 * H, 3 * H, dtype=torch.float64)
        for d in range(nd):
            W[d, d * 3 * H:(d + 1) * 3 * H] = torch.eye(3 * H, dtype=torch.float64)
        zero = torch.zeros(nd, 3 * H, dtype=torch.float64)
        tag = 'H={} nd={} B={}'.format(H, nd, B)
        for lens in (LENS[B], [T] * B):
            ld = torch.tensor(lens, dtype=torch.int32, device='cuda')
            h = _gru_call('ptts_gru_fwd_ragged', xproj, U, nd, ld)
            torch.cuda.synchronize()
            assert not bool(torch.isnan(h).any()), tag + ': a frame was never written'
            for b, n in enumerate(lens):
                alone = _gru_call('ptts_gru_fwd', xproj[b:b + 1, :n].contiguous(), U, nd)
                _bytes_equal(h[b, :n], alone[0], '{} row {} (len {})'.format(tag, b, n))
                _exact_zero(h[b, n:], '{} row {}'.format(tag, b))
                want = tg.gru_ref(xproj[b:b + 1, :n].cpu().double(), W, U.cpu().double(), zero)
                tg.close(h[b:b + 1, :n], want, 2e-4, 2e-5, '{} row {} against fp64'.format(tag, b))
            if lens == [T] * B:
                _bytes_equal(h, _gru_call('ptts_gru_fwd', xproj, U, nd), tag + ' all lengths T against ptts_gru_fwd')


# ---------------------------------------------------------------------------------------------------------------------------
# 4: ptts_affine_act_rows
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('C,F', [(4, 1), (4, 5), (3, 1), (3, 5)])        # float4 and scalar kernels; inner = C and inner = F*C
def test_affine_act_rows_is_affine_act_with_the_rows_ended(C, F):
    from percivaltts_amd import _hip
    B, Tn, alpha = 3, 101, 0.3
    lens = [101, 40, 1]
    inner = F * C
    per_lane = 4 if C % 4 == 0 else 1
    assert (B * Tn) % 256 != 0 and (B * Tn * inner // per_lane) % 256 != 0 and B * Tn * inner // per_lane > 256    # several blocks, a partial one
    g = torch.Generator().manual_seed(3)
    x = _dev(torch.randn(B, Tn, inner, generator=g, dtype=torch.float64))
    scale, shift = _dev(torch.randn(C, generator=g, dtype=torch.float64)), _dev(torch.randn(C, generator=g, dtype=torch.float64))
    ld = torch.tensor(lens, dtype=torch.int32, device='cuda')
    for act in (0, 1, 2, 3):
        for sc, sh in ((None, None), (scale, shift)):
            want = _nan(B, Tn, inner)
            _hip.call('ptts_affine_act', _hip.ptr(x), _hip.ptr(sc), _hip.ptr(sh), _hip.ptr(want), B * Tn * F, C, act, alpha, None)
            got = _nan(B, Tn, inner)
            _hip.call('ptts_affine_act_rows', _hip.ptr(x), _hip.ptr(sc), _hip.ptr(sh), _hip.ptr(got), _hip.ptr(ld), B, Tn, inner, C,
                      act, alpha, None)
            inplace = x.clone()
            _hip.call('ptts_affine_act_rows', _hip.ptr(inplace), _hip.ptr(sc), _hip.ptr(sh), _hip.ptr(inplace), _hip.ptr(ld), B, Tn,
                      inner, C, act, alpha, None)
            for b, n in enumerate(lens):
                what = 'C={} F={} act={} affine={} row {}'.format(C, F, act, sc is not None, b)
                _bytes_equal(got[b, :n], want[b, :n], what)
                _exact_zero(got[b, n:], what)
            _bytes_equal(inplace, got, 'in place')
    lib = _hip.lib()
    p = _hip.ptr(x)
    assert lib.ptts_affine_act_rows(p, None, None, p, None, B, Tn, inner, C, 0, alpha, None) == -1        # no lengths
    assert lib.ptts_affine_act_rows(p, _hip.ptr(scale), None, p, _hip.ptr(ld), B, Tn, inner, C, 0, alpha, None) == -1
    assert lib.ptts_affine_act_rows(p, None, None, p, _hip.ptr(ld), B, Tn, inner + 1, C, 0, alpha, None) == -1   # inner % C


# ---------------------------------------------------------------------------------------------------------------------------
# 5: the model
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('geom', ['test', 'default', 'nocnn', 'gated', 'gated_dilated'])
def test_predict_batch_matches_each_utterance_alone(geom):
    _, _, mod, _, a, gw, _, _, _, _ = tm.build(geom)
    Tmax = tm.GEOMS[geom]['T']
    lens = [Tmax, Tmax - 1, 3, 1]
    gen = torch.Generator().manual_seed(8)
    xs = [torch.rand(n, a.ctxsize, generator=gen, dtype=torch.float64) * 2 - 1 for n in lens]
    got = mod.predict_batch([x.numpy().astype(np.float32) for x in xs])
    assert [y.shape for y in got] == [(n, a.outsize) for n in lens]
    with torch.no_grad():
        for i, (x, y) in enumerate(zip(xs, got)):
            want = O.generator_forward(gw, a, x[None], training=False)[0]
            tm.close(torch.from_numpy(y), want, rr.GPU_RTOL, rr.GPU_ATOL, '{} utterance {} (T = {})'.format(geom, i, lens[i]))
    # tensors in, device tensors out; the padded result's pad rows are exactly zero
    dev = mod.predict_device_batch([x.to(torch.float32) for x in xs])
    for y, d in zip(got, dev):
        assert d.is_cuda and d.dtype == torch.float32
        np.testing.assert_array_equal(d.cpu().numpy(), y)
    xpad = torch.zeros(len(lens), Tmax, a.ctxsize, dtype=torch.float32, device='cuda')
    for i, x in enumerate(xs):
        xpad[i, :lens[i]] = x.to(torch.float32).cuda()
    ld = torch.tensor(lens, dtype=torch.int32, device='cuda')
    with torch.no_grad():
        ypad = mod.kerasmodel(xpad, training=False, memo={'lengths': ld})
    for i, n in enumerate(lens):
        np.testing.assert_array_equal(ypad[i, :n].cpu().numpy(), got[i])
        _exact_zero(ypad[i, n:], '{} utterance {}'.format(geom, i))
    # lengths are for inference
    with torch.no_grad():
        with pytest.raises(ValueError, match='training'):
            mod.kerasmodel(xpad, training=True, memo={'lengths': ld})
        for bad in (ld.long(), ld.cpu(), ld[:2], [int(n) for n in lens]):
            with pytest.raises(ValueError, match='lengths'):
                mod.kerasmodel(xpad, training=False, memo={'lengths': bad})
    with pytest.raises(ValueError, match='no_grad'):
        mod.kerasmodel(xpad, training=False, memo={'lengths': ld})


def _randomise(model, seed):
    """Random weights with non-trivial BatchNorm statistics, so that pad rows are non-zero behind the first layer."""
    g = torch.Generator().manual_seed(seed)
    ws = []
    for name, w in model.kerasmodel.weights():
        name = name.split('/')[-1]
        if name == 'moving_variance':
            ws.append((torch.rand(w.shape, generator=g) + 0.5).numpy())
        elif w.dim() == 1 or name in ('bias', 'beta', 'gamma', 'moving_mean'):
            ws.append((torch.randn(w.shape, generator=g) * 0.3 + (1.0 if name == 'gamma' else 0.0)).numpy())
        else:
            ws.append((torch.randn(w.shape, generator=g) / math.sqrt(w.shape[-2])).numpy())
    model.kerasmodel.set_weights(ws)


def test_predict_batch_generic_fc_bgru_cnn1d():
    import percivaltts_amd
    from percivaltts_amd import modeltts_common, vocoders
    cfg = percivaltts_amd.configuration()
    cfg.arch_hiddenwidth = 6; cfg.train_batch_size = 2
    voc = vocoders.VocoderPML(16000, 0.005, 12, 4)
    mod = modeltts_common.Generic(19, voc, layertypes=['FC', 'BGRU', ['CNN1D', 7, 5]], cfgarch=cfg)
    _randomise(mod, 4)
    Tmax = 20
    lens = [Tmax, Tmax - 1, 3, 1]
    gen = torch.Generator().manual_seed(8)
    xs = [(torch.rand(n, 19, generator=gen) * 2 - 1).numpy() for n in lens]
    got = mod.predict_batch(xs)
    worst_unmasked = 0.0
    xpad = np.zeros((len(lens), Tmax, 19), dtype=np.float32)
    for i, x in enumerate(xs):
        xpad[i, :lens[i]] = x
    plain = mod.predict(xpad)                                   # the padded batch with no lengths: what the rule prevents
    for i, (x, y) in enumerate(zip(xs, got)):
        want = mod.predict(x[None])[0]
        tm.close(torch.from_numpy(y), torch.from_numpy(want), rr.GPU_RTOL, rr.GPU_ATOL, 'Generic utterance {} (T = {})'.format(i, lens[i]))
        if lens[i] < Tmax:
            worst_unmasked = max(worst_unmasked, float(np.abs(plain[i, :lens[i]] - want).max()))
    assert worst_unmasked > 100 * rr.GPU_ATOL                   # the inputs have teeth here too


def test_conv2dstack_refuses_lengths():
    from percivaltts_amd import layers as kl
    l_in = kl.Input(shape=(None, 9))
    model = kl.Model(l_in, kl.Conv2DStack(2, 2, [3, 3], name='critic_stack')(l_in)).cuda()
    x = torch.zeros(2, 6, 9, device='cuda')
    ld = torch.tensor([6, 2], dtype=torch.int32, device='cuda')
    with torch.no_grad():
        assert model(x, training=False).shape == (2, 6, 9, 2)
        with pytest.raises(ValueError, match='critic_stack'):
            model(x, training=False, memo={'lengths': ld})


# ---------------------------------------------------------------------------------------------------------------------------
# 6: generate_params
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('wins', [None, 'ref'])
def test_generate_params_predict_batched(wins, tmp_path):
    import test_mlpg as tmlpg
    from percivaltts_amd import _hip
    wins = tmlpg.REF_WINS if wins == 'ref' else None
    ctx, voc, mod = tmlpg._build('dcnn-pml', wins)
    _randomise(mod, 9)
    raw = voc.featuressizeraw()
    lens = [41, 23, 60, 37, 9]
    fids, inpath, outpath, mean, std = tmlpg._corpus(tmp_path, ctx, voc, lens)
    mod.generate_params(inpath, outpath, fids, str(tmp_path / 'one'), do_objmeas=False, batch_size=3)
    with _hip.KernelTimer() as kt:
        mod.generate_params(inpath, outpath, fids, str(tmp_path / 'bat'), do_objmeas=False, batch_size=3, predict_batched=True)
    names = [r[0] for r in kt.records]
    assert names.count('ptts_lstm_fwd_ragged') == 2 and 'ptts_lstm_fwd' not in names        # groups of 3 and 2, one forward each
    # the default path does not depend on batch_size (byte-identical files)
    mod.generate_params(inpath, outpath, fids, str(tmp_path / 'one1'), do_objmeas=False, batch_size=1)
    # de-normalised values: the bound of predict scaled by std per column (MLPG's solve is a weighted average of the statics and
    # deltas of one feature: the statics' column scale bounds it)
    stdraw = std[:raw].astype(np.float64)
    for fid, n in zip(fids, lens):
        one = np.fromfile(str(tmp_path / 'one' / (fid + '.cmp')), dtype=np.float32).reshape(-1, raw)
        bat = np.fromfile(str(tmp_path / 'bat' / (fid + '.cmp')), dtype=np.float32).reshape(-1, raw)
        np.testing.assert_array_equal(one, np.fromfile(str(tmp_path / 'one1' / (fid + '.cmp')), dtype=np.float32).reshape(-1, raw))
        assert one.shape == bat.shape == (n, raw)
        norm_one = (one.astype(np.float64) - mean[:raw]) / stdraw
        err = np.abs(bat.astype(np.float64) - one) / stdraw
        tol = rr.GPU_ATOL + rr.GPU_RTOL * np.abs(norm_one)
        print('{}: worst err / bound {:.4f}'.format(fid, float((err / tol).max())))
        assert (err <= tol).all(), '{}: worst err / bound {:.3f}'.format(fid, float((err / tol).max()))
