"""Validation costs on ragged batches (OptimizerTTSWGAN.validation_costs_batch, cfg.train_validation_batch_size,
data.length_groups) against the CPU oracle run on ONE utterance at a time -- tests/test_ragged_critic_rule.py shows in float64
why the masked batch gives exactly that.  The bound is the one tests/test_model_gpu.py::test_evaluation_mode_losses_whole_utterances
applies to the same quantities at batch 1 (rtol 5e-4, atol 1e-5); where both sides of a comparison are device results, each
within that bound of the oracle, it is doubled."""
import functools

import numpy as np
import pytest
import torch

from oracle import percival_oracle as O

import test_model_gpu as tm

gpu = pytest.mark.gpu

RTOL, ATOL = 5e-4, 1e-5
LENS = [37, 1, 40, 9, 23]
TRANSIDX = 30.0
KEYS = ('gen_total', 'gen_wgan', 'gen_ls', 'critic_total', 'l_valid', 'l_fake', 'gp')


@functools.lru_cache(maxsize=None)
def setup(geom):
    """The prepared optimiser of `geom`, five utterances with injected alphas, and the oracle's costs of each utterance alone
    (computed once; nobody writes to any of it -- every test checks that the weights are what they were)."""
    from percivaltts_amd import optimizertts_wgan
    cfg, voc, mod, crit, a, gw, cw, _, _, _ = tm.build(geom)
    cfg.train_wgan_critic_LSWGANtransidx = TRANSIDX
    opt = optimizertts_wgan.OptimizerTTSWGAN(cfg, mod, errtype='WLSWGAN', critic=crit)
    opt.prepare()
    gen = torch.Generator().manual_seed(77)
    g = tm.GEOMS[geom]
    xs = [torch.rand(n, g['ctx'], generator=gen, dtype=torch.float64) * 2 - 1 for n in LENS]
    ys = [torch.randn(n, a.outsize, generator=gen, dtype=torch.float64) for n in LENS]
    al = torch.rand(len(LENS), generator=gen, dtype=torch.float64)
    w_ls, ww = O.wls_weights(a.specsize, a.noisesize, 0, 0.25, TRANSIDX)
    want = {k: [] for k in KEYS + ('sq_err', 'nbel')}
    for i in range(len(LENS)):
        total, parts = O.critic_step_loss(cw, gw, a, xs[i][None], ys[i][None], al[i:i + 1], gp_lambda=10.0, training=False)
        gtot, gparts = O.generator_step_loss(cw, gw, a, xs[i][None], ys[i][None], 'WLSWGAN', torch.tensor(w_ls), ww, training=False)
        for k, v in (('gen_total', gtot), ('gen_wgan', gparts['wgan']), ('gen_ls', gparts['ls']), ('critic_total', total),
                     ('l_valid', parts['valid']), ('l_fake', parts['fake']), ('gp', parts['gp']),
                     ('sq_err', ((ys[i] - gparts['pred'][0]) ** 2).sum()), ('nbel', torch.tensor(float(ys[i].numel())))):
            want[k].append(float(v.detach()))
    want = {k: torch.tensor(v, dtype=torch.float64) for k, v in want.items()}
    return opt, mod, crit, gw, cw, xs, ys, al, want


def unchanged(mod, crit, gw, cw):
    for (k, t), w in zip(mod.kerasmodel.weights(), gw):
        assert torch.equal(t.detach().cpu(), w.to(torch.float32)), 'generator weight changed: ' + k
    for (k, t), w in zip(crit.model.weights(), cw):
        assert torch.equal(t.detach().cpu(), w.to(torch.float32)), 'critic weight changed: ' + k


def f32np(ts):
    return [t.numpy().astype(np.float32) for t in ts]


@gpu
@pytest.mark.parametrize('geom', ['test', 'default'])
@pytest.mark.parametrize('batch_size', [2, 5, 1])
def test_costs_of_each_utterance_against_the_oracle(geom, batch_size):
    from percivaltts_amd import _hip
    opt, mod, crit, gw, cw, xs, ys, al, want = setup(geom)
    with _hip.KernelTimer() as kt:
        got = opt.validation_costs_batch(f32np(xs), f32np(ys), alphas=al, batch_size=batch_size)
    names = [r[0] for r in kt.records]
    ngroups = -(-len(LENS) // batch_size)
    assert names.count('ptts_lstm_fwd_ragged') == ngroups and 'ptts_lstm_fwd' not in names      # ONE generator forward per group
    assert names.count('ptts_wlse_rows') == ngroups and names.count('ptts_gp_penalty_rows') == ngroups
    assert 'ptts_affine_act_rows_bwd' in names
    assert set(got) == set(want)
    for k, v in got.items():
        assert v.is_cuda and v.shape == (len(LENS),), k
        assert v.dtype == (torch.float64 if k in ('sq_err', 'nbel') else torch.float32), k
    assert torch.equal(got['nbel'].cpu(), want['nbel'])
    for k in KEYS + ('sq_err',):
        for i, n in enumerate(LENS):
            print('{} batch_size {} utterance {} (T = {}) {}: {:+.8e}, oracle {:+.8e}'.format(
                geom, batch_size, i, n, k, float(got[k][i]), float(want[k][i])))
        tm.close(got[k], want[k], RTOL, ATOL, '{} at batch_size {}'.format(k, batch_size))
    rmse = torch.sqrt(got['sq_err'].sum() / got['nbel'].sum())
    tm.close(rmse, torch.sqrt(want['sq_err'].sum() / want['nbel'].sum()), RTOL, ATOL, 'pooled RMSE')
    # nothing inside makes the host wait for the device: no .item(), no download, no blocking upload
    torch.cuda.set_sync_debug_mode('error')
    try:
        again = opt.validation_costs_batch(f32np(xs), f32np(ys), alphas=al, batch_size=batch_size)
    finally:
        torch.cuda.set_sync_debug_mode('default')
    for k in KEYS:
        tm.close(again[k], want[k], RTOL, ATOL, '{} at batch_size {}, second sweep'.format(k, batch_size))
    unchanged(mod, crit, gw, cw)


@gpu
def test_wgan_costs_have_no_least_squares_term():
    from percivaltts_amd import optimizertts_wgan
    cfg, voc, mod, crit, a, gw, cw, _, _, _ = tm.build('test')
    opt = optimizertts_wgan.OptimizerTTSWGAN(cfg, mod, errtype='WGAN', critic=crit)
    opt.prepare()
    _, _, _, _, _, xs, ys, al, want = setup('test')
    got = opt.validation_costs_batch(f32np(xs), f32np(ys), alphas=al, batch_size=3, sort=False)
    assert torch.equal(got['gen_total'], got['gen_wgan']) and float(got['gen_ls'].abs().sum()) == 0.0
    tm.close(got['gen_wgan'], want['gen_wgan'], RTOL, ATOL, 'gen_wgan (WGAN)')
    tm.close(got['critic_total'], want['critic_total'], RTOL, ATOL, 'critic_total (WGAN)')


def new_costs():
    return {k: [] for k in ('model_rmse_validation', 'model_validation', 'critic_training', 'critic_validation', 'critic_validation_ltm')}


@gpu
def test_update_validation_cost_both_ways():
    from percivaltts_amd import _hip, data
    opt, mod, crit, gw, cw, xs, ys, al, want = setup('default')
    Xv, Yv = f32np(xs), f32np(ys)
    assert opt.cfg.train_validation_batch_size is None
    opt.validation_alphas = al
    try:
        # what the parent's update_validation_cost launches: its three passes per utterance, through functions this change leaves alone
        ald = tm.f32(al)
        opt.costs_tra_critic_batches.append_device(torch.tensor(0.5, device='cuda'))
        opt.update_validation_cost(new_costs(), Xv, Yv)            # (weight-keyed operand caches warm: both counts below see them filled)
        with _hip.KernelTimer() as kt_ref:
            data.cost_model_prediction_rmse(mod, [Xv], Yv)
            with torch.no_grad():
                for x, y in zip(Xv, Yv):
                    opt.generator_loss(opt._to_dev(x[None]), opt._to_dev(y[None]), training=False)
            for i, (x, y) in enumerate(zip(Xv, Yv)):
                opt.critic_loss(opt._to_dev(x[None]), opt._to_dev(y[None]), ald[i:i + 1], training=False)
        opt.costs_tra_critic_batches.append_device(torch.tensor(0.5, device='cuda'))
        one = new_costs()
        with _hip.KernelTimer() as kt_one:
            ret_one = opt.update_validation_cost(one, Xv, Yv)
        assert [r[0] for r in kt_one.records] == [r[0] for r in kt_ref.records], 'the default path launches something else'
        assert 'ptts_lstm_fwd_ragged' not in [r[0] for r in kt_one.records]

        opt.cfg.train_validation_batch_size = 2
        opt.costs_tra_critic_batches.append_device(torch.tensor(0.5, device='cuda'))
        bat = new_costs()
        with _hip.KernelTimer() as kt_bat:
            ret_bat = opt.update_validation_cost(bat, Xv, Yv)
        names = [r[0] for r in kt_bat.records]
        assert names.count('ptts_lstm_fwd_ragged') == 3 and 'ptts_lstm_fwd' not in names
    finally:
        opt.cfg.train_validation_batch_size = None
        opt.validation_alphas = None
    assert list(one) == list(bat) and all(len(v) == 1 for v in one.values()) and all(len(v) == 1 for v in bat.values())
    for k in ('model_rmse_validation', 'model_validation', 'critic_validation'):
        print('{}: one by one {:+.8e}, batched {:+.8e}'.format(k, one[k][0], bat[k][0]))
        tm.close(torch.tensor(bat[k][0]), torch.tensor(one[k][0]), 2 * RTOL, 2 * ATOL, k)
    # ... and each within the bound of the oracle's definition: the pooled RMSE, the per-utterance costs averaged
    tm.close(torch.tensor(bat['model_rmse_validation'][0]), torch.sqrt(want['sq_err'].sum() / want['nbel'].sum()), RTOL, ATOL, 'RMSE')
    tm.close(torch.tensor(bat['model_validation'][0]), want['gen_total'].mean(), RTOL, ATOL, 'model_validation')
    tm.close(torch.tensor(bat['critic_validation'][0]), want['critic_total'].mean(), RTOL, ATOL, 'critic_validation')
    assert one['critic_training'] == bat['critic_training'] == [0.5]
    assert ret_one == one['critic_validation_ltm'][0] == one['critic_validation'][0]
    assert ret_bat == bat['critic_validation_ltm'][0] == bat['critic_validation'][0]
    assert len(opt.costs_tra_critic_batches) == 0
    unchanged(mod, crit, gw, cw)


@gpu
def test_batched_rmse_of_the_lse_optimiser():
    from percivaltts_amd import data, optimizertts
    opt, mod, crit, gw, cw, xs, ys, al, want = setup('test')
    Xv, Yv = f32np(xs), f32np(ys)
    rmse = torch.sqrt(want['sq_err'].sum() / want['nbel'].sum())
    for bs in (None, 1, 2, 5):
        tm.close(torch.tensor(data.cost_model_prediction_rmse(mod, [Xv], Yv, batch_size=bs)), rmse, RTOL, ATOL, 'RMSE at {}'.format(bs))
    lse = optimizertts.OptimizerTTS(opt.cfg, mod, train_validation_batch_size=2)
    costs = new_costs()
    assert lse.update_validation_cost(costs, Xv, Yv) == costs['model_rmse_validation'][0]
    tm.close(torch.tensor(costs['model_rmse_validation'][0]), rmse, RTOL, ATOL, 'OptimizerTTS.update_validation_cost')
    with pytest.raises(ValueError, match='train_validation_batch_size'):
        optimizertts.OptimizerTTS(opt.cfg, mod, train_validation_batch_size=0).update_validation_cost(new_costs(), Xv, Yv)
    opt.cfg.train_validation_batch_size = None


def padding(lens, groups):
    return sum(len(g) * max(lens[i] for i in g) - sum(lens[i] for i in g) for g in groups)


def test_length_groups():
    from percivaltts_amd import data
    rng = np.random.RandomState(4)
    cases = [[1, 1, 10], [10, 10, 1], [1, 1, 5, 9, 9], LENS, [7], [3, 3, 3, 3]] + [list(rng.randint(1, 700, size=n)) for n in (2, 8, 13, 31)]
    for lens in cases:
        for bs in (1, 2, 3, 4, 8, 64):
            plain, srt = data.length_groups(lens, bs, sort=False), data.length_groups(lens, bs)
            for groups in (plain, srt):
                assert sorted(i for g in groups for i in g) == list(range(len(lens)))          # every index once
                assert all(1 <= len(g) <= bs for g in groups)
                assert len(groups) == -(-len(lens) // bs)
            assert [i for g in plain for i in g] == list(range(len(lens)))                      # sort=False keeps the input order
            assert padding(lens, srt) <= padding(lens, plain)                                   # sorting never adds padding
            order = [i for g in srt for i in g]
            assert all((lens[a], a) < (lens[b], b) for a, b in zip(order, order[1:]))           # a STABLE sort by length
    assert data.length_groups(LENS, 2) == [[1, 3], [4], [0, 2]]
    assert padding([1, 1, 5, 9, 9], data.length_groups([1, 1, 5, 9, 9], 2)) == 0                # the short group stands where it costs least
    with pytest.raises(ValueError, match='batch_size'):
        data.length_groups(LENS, 0)


@gpu
def test_generate_params_group_by_length(tmp_path):
    import test_mlpg as tmlpg
    import test_ragged_gpu as trg
    import test_ragged_rule as rr
    from percivaltts_amd import _hip
    ctx, voc, mod = tmlpg._build('dcnn-pml', None)
    trg._randomise(mod, 9)
    raw = voc.featuressizeraw()
    lens = [41, 23, 60, 37, 9]
    fids, inpath, outpath, mean, std = tmlpg._corpus(tmp_path, ctx, voc, lens)
    mod.generate_params(inpath, outpath, fids, str(tmp_path / 'bat'), do_objmeas=False, batch_size=2, predict_batched=True)
    mod.generate_params(inpath, outpath, fids, str(tmp_path / 'off'), do_objmeas=False, batch_size=2, predict_batched=True, group_by_length=False)
    with _hip.KernelTimer() as kt:
        mod.generate_params(inpath, outpath, fids, str(tmp_path / 'grp'), do_objmeas=False, batch_size=2, predict_batched=True, group_by_length=True)
    assert [r[0] for r in kt.records].count('ptts_lstm_fwd_ragged') == 3
    with pytest.raises(ValueError, match='predict_batched'):
        mod.generate_params(inpath, outpath, fids, str(tmp_path / 'bad'), do_objmeas=False, batch_size=2, group_by_length=True)
    stdraw = std[:raw].astype(np.float64)
    for fid, n in zip(fids, lens):
        bat = np.fromfile(str(tmp_path / 'bat' / (fid + '.cmp')), dtype=np.float32).reshape(-1, raw)
        off = np.fromfile(str(tmp_path / 'off' / (fid + '.cmp')), dtype=np.float32).reshape(-1, raw)
        grp = np.fromfile(str(tmp_path / 'grp' / (fid + '.cmp')), dtype=np.float32).reshape(-1, raw)
        np.testing.assert_array_equal(bat, off)                      # without the keyword: the same bytes
        assert grp.shape == bat.shape == (n, raw)
        err = np.abs(grp.astype(np.float64) - bat) / stdraw
        tol = rr.GPU_ATOL + rr.GPU_RTOL * np.abs((bat.astype(np.float64) - mean[:raw]) / stdraw)
        print('{}: worst err / bound {:.4f}'.format(fid, float((err / tol).max())))
        assert (err <= tol).all(), '{}: worst err / bound {:.3f}'.format(fid, float((err / tol).max()))


@gpu
def test_refusals():
    from percivaltts_amd import networks_critic, optimizertts_wgan
    cfg, voc, mod, crit, a, gw, cw, X, Y, al = tm.build('default')
    # a Conv2DStack critic takes no lengths: refused when the optimiser is prepared, both options named
    cfg.arch_critic_bf16 = True
    stack = networks_critic.Critic(voc, tm.GEOMS['default']['ctx'], cfg)
    opt = optimizertts_wgan.OptimizerTTSWGAN(cfg, mod, errtype='WLSWGAN', critic=stack, train_validation_batch_size=2)
    with pytest.raises(ValueError, match='train_validation_batch_size.*arch_critic_bf16'):
        opt.prepare()
    opt.cfg.train_validation_batch_size = None
    opt.prepare()                                               # ... and only then
    with pytest.raises(ValueError, match='arch_critic_bf16'):
        opt.validation_costs_batch([X[0].numpy()], [Y[0].numpy()])
    # the input-gradient mode is evaluation: training=True raises, whichever way the model is entered
    crit.model.cuda()
    lengths = torch.tensor([50, 7, 20], dtype=torch.int32, device='cuda')
    memo = {'lengths': lengths, 'lengths_input_grad': True}
    Xd, Yd = tm.f32(X), tm.f32(Y)
    with pytest.raises(ValueError, match='training=True'):
        crit.model(Yd, Xd, training=True, memo=dict(memo))
    with pytest.raises(ValueError, match='training=True'):
        crit.model.forward_multi_at(crit.node_spec_in, [Yd[:, :, 1:66].contiguous()], {crit.input_ctx: Xd}, training=True, memo=dict(memo))
    with pytest.raises(ValueError, match='training=True'):
        crit.model.forward_multi(0, [Yd], [Xd], training=True, memo=dict(memo))
    # gradients are allowed there, and only there; the generator's recurrence refuses them in either mode
    assert crit.model(Yd, Xd, training=False, memo=dict(memo)).requires_grad
    with pytest.raises(ValueError, match='no_grad'):
        crit.model(Yd, Xd, training=False, memo={'lengths': lengths})
    mod.to_device()
    with pytest.raises(ValueError, match='no_grad'):
        mod.kerasmodel(Xd, training=False, memo=dict(memo))
