"""Masked training through the training driver: run.training() with cfg.train_batch_padtype = 'randshiftpad', for the least-squares
optimiser (host loader) and for WLSWGAN (host loader, and the training set resident on the device), on a synthetic corpus that holds utterances shorter and longer than train_batch_lengthmax (the shrunk configuration of
tests/test_run_synthetic.py).  With train_batch_length set to it every batch has T == lengthmax and carries its lengths, the costs are finite, and --continue reproduces
the uninterrupted run in deterministic mode (the draws per batch are fixed by the padtype: one per row).  With the default
padtype one step launches what it launched: no entry point of masked training, and the same list whether or not the optimiser was
prepared for masked batches."""
import importlib
import os
import pickle

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

LENGTHMAX = 60


def _configure(run, errtype='LSE', on_device=False):
    run.errtype = errtype
    run.cfg.train_data_on_device = bool(on_device)
    run.cfg.id_valid_start = 8; run.cfg.id_valid_nb = 1; run.cfg.id_test_nb = 1
    run.cfg.train_min_nbepochs = 1; run.cfg.train_cancel_nodecepochs = 10
    run.cfg.train_nbepochs_scalewdata = False
    run.cfg.train_batch_size = 2; run.cfg.arch_hiddenwidth = 8; run.cfg.arch_gen_nbcnnlayers = 2
    run.cfg.train_batch_length = LENGTHMAX               # a given length: every batch has it, whatever its rows (unset, a batch of short rows is as long as its longest)
    run.cfg.train_batch_lengthmax = LENGTHMAX
    run.cfg.train_batch_padtype = 'randshiftpad'


@pytest.mark.parametrize('errtype,on_device', [('LSE', False), ('WLSWGAN', False), ('WLSWGAN', True)])
def test_masked_run_and_resume(tmp_path, monkeypatch, errtype, on_device):
    from percivaltts_amd import ops, optimizertts, optimizertts_wgan
    monkeypatch.setenv('PERCIVAL_CORPUS', str(tmp_path / 'corpus'))
    import percivaltts_amd.run as run
    seen = []
    cls = optimizertts.OptimizerTTS if errtype == 'LSE' else optimizertts_wgan.OptimizerTTSWGAN
    plain = cls.train_on_batch

    def spy(self, batchid, X, Y, lengths=None):
        seen.append((tuple(X.shape), None if lengths is None else np.asarray(lengths).copy()))
        return plain(self, batchid, X, Y, lengths=lengths)
    monkeypatch.setattr(cls, 'train_on_batch', spy)
    parts = ('.model.weights.npz', '.optimizer.npz') if errtype == 'LSE' else \
        ('.model.weights.npz', '.critic.weights.npz', '.generator.optimizer.npz', '.critic.optimizer.npz')
    ops.deterministic(True)
    try:
        states = {}
        for name, plan in (('straight', [(4, False)]), ('resumed', [(2, False), (4, True)])):
            wd = tmp_path / name
            wd.mkdir()
            monkeypatch.chdir(wd)
            run = importlib.reload(run)
            _configure(run, errtype, on_device)
            if not os.path.exists(run.cfg.fileids):
                run.synthesize_corpus(nfiles=10, minlen=50, maxlen=140)
            for (nep, cont) in plan:
                np.random.seed(123); __import__('torch').manual_seed(123)
                if cont:
                    np.random.seed(999); __import__('torch').manual_seed(999)      # a resumed run must not depend on the fresh seeds
                run.cfg.train_max_nbepochs = nep
                run.training(cont=cont)
            st = 'model-trainingstate-last.h5'
            with open(st + '.model.cfgextras.pkl', 'rb') as f:
                _, extras, _ = pickle.load(f)
            states[name] = {k: dict(np.load(st + k)) for k in parts}
            states[name]['extras'] = extras
    finally:
        ops.deterministic(False)
    assert seen and all(shape[1] == LENGTHMAX and n is not None for shape, n in seen), 'a batch without T == lengthmax or without lengths'
    ns = np.concatenate([n for _, n in seen])
    assert ns.min() >= 1 and ns.max() == LENGTHMAX and ns.min() < LENGTHMAX, 'the corpus gave no short and no full row: {}'.format(sorted(set(ns.tolist())))
    a, b = states['straight'], states['resumed']
    assert a['extras']['epoch'] == b['extras']['epoch'] == 4
    keys = ('model_training', 'model_rmse_validation') + (() if errtype == 'LSE' else ('critic_training', 'critic_validation', 'model_validation'))
    for k in keys:
        assert np.isfinite(a['extras']['costs'][k]).all(), k
        np.testing.assert_allclose(b['extras']['costs'][k], a['extras']['costs'][k], rtol=1e-6, atol=1e-7, err_msg=k)
    for part in parts:
        assert sorted(a[part]) == sorted(b[part])
        for k in a[part]:
            np.testing.assert_allclose(b[part][k], a[part][k], rtol=1e-6, atol=1e-8, err_msg=part + ':' + k)


def test_the_default_step_launches_what_it_launched():
    """The launches of one default train_on_batch worth of work (critic step + generator step, eager), recorded as
    tests/test_validation_batched_gpu.py records them: none of them is an entry point of masked training, and an optimiser prepared
    for 'randshiftpad' launches the same list when it is given a batch without lengths.  The masked step is another list."""
    import torch
    import test_model_gpu as tm
    from percivaltts_amd import _hip, optimizertts_wgan
    new = ('ptts_colstats_rows', 'ptts_affine_act_rows_bwd_params', 'ptts_axpby_cols_rows', 'ptts_lstm_bwd_ragged', 'ptts_gru_bwd_ragged',
           'ptts_rows_combine', 'ptts_rows_mean_bwd', 'ptts_wlse_rows_bwd', 'ptts_affine_act_rows', 'ptts_affine_act_rows_bwd',
           'ptts_lstm_fwd_ragged', 'ptts_gru_fwd_ragged', 'ptts_rows_mean', 'ptts_wlse_rows')
    lists = {}
    for padtype in ('randshift', 'randshiftpad'):
        cfg, voc, mod, crit, a, gw, cw, X, Y, al = tm.build('default')
        cfg.train_wgan_critic_LSWGANtransidx = 30.0
        cfg.train_wgan_hipgraph = False
        cfg.train_batch_padtype = padtype
        opt = optimizertts_wgan.OptimizerTTSWGAN(cfg, mod, errtype='WLSWGAN', critic=crit)
        opt.prepare()
        Xd, Yd = tm.f32(X), tm.f32(Y)
        opt.device_step(0, Xd, Yd, alpha=tm.f32(al))                 # warm: caches of derived operands are filled
        with _hip.KernelTimer() as kt:
            opt.device_step(10, Xd, Yd, alpha=tm.f32(al))
        torch.cuda.synchronize()
        lists[padtype] = [r[0] for r in kt.records]
        if padtype == 'randshiftpad':
            with _hip.KernelTimer() as kt:
                opt.device_step(20, Xd, Yd, alpha=tm.f32(al), lengths=np.array([50, 49, 3], dtype=np.int32))
            torch.cuda.synchronize()
            lists['masked'] = [r[0] for r in kt.records]
    assert len(lists['randshift']) > 50
    assert not [n for n in lists['randshift'] if n in new], 'the default step launches an entry point of masked training'
    assert lists['randshiftpad'] == lists['randshift'], 'prepared for masked batches, the dense step launches something else'
    assert set(new[:8]) - {'ptts_gru_bwd_ragged'} <= set(lists['masked']), 'the masked step misses one of its kernels'
