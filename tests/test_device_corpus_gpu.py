"""The device-resident training set on the GPU: the gather kernel (csrc/batchgather.hip, ptts_batch_windows) against a numpy
gather, data.DeviceCorpus.batch against load_inoutset (windows, random draws, rank shards), what one batch launches and
uploads, and a training run fed from the resident corpus against the same run fed by the host loader.  The feature moves
bytes and computes nothing: every comparison is exact."""
import functools
import os

import numpy as np
import pytest
import torch

import test_device_corpus as tdc

pytestmark = pytest.mark.gpu

UTT_LENS = [1, 2, 7, 7, 9, 12, 30, 4]
# (utt, shift, n) at T = 7: utterance 0 at corpus offset 0 with n = 1 (and n < T at shift 0); the last utterance, ending on the
# corpus's last row; shift = len - T with n = T, twice the same utterance; shift = len - T of the longest
ROWS_T7 = [(0, 0, 1), (7, 0, 4), (5, 5, 7), (5, 0, 7), (6, 23, 7)]


def packed(lens, dims, seed):
    rng = np.random.RandomState(seed)
    return [rng.randn(sum(lens), d).astype(np.float32) for d in dims]


def gather_and_check(lens, srcs, rows, T):
    """ops.batch_windows into NaN-filled destinations that sit inside larger NaN buffers, against the numpy gather: an element
    left unwritten, padding that is not exactly 0.0 or a write outside the destination fails."""
    from percivaltts_amd import ops
    row_off = np.concatenate(([0], np.cumsum(lens))).astype(np.int64)
    B = len(rows)
    bufs = [torch.full((B + 2, T, s.shape[1]), float('nan'), device='cuda') for s in srcs]
    outs = [b[1:B + 1] for b in bufs]
    tabs = [torch.tensor([r[k] for r in rows], dtype=torch.int32) for k in range(3)]
    got = ops.batch_windows([torch.from_numpy(s).cuda() for s in srcs], torch.from_numpy(row_off), tabs[0], tabs[1], tabs[2], T, out=outs)
    assert all(g is o for g, o in zip(got, outs))
    for s, buf in zip(srcs, bufs):
        want = np.zeros((B, T, s.shape[1]), dtype=np.float32)
        for b, (u, sh, n) in enumerate(rows):
            want[b, :n] = s[row_off[u] + sh:row_off[u] + sh + n]
        host = buf.cpu().numpy()
        assert np.array_equal(host[1:B + 1], want)
        assert np.isnan(host[0]).all() and np.isnan(host[B + 1]).all()
    fresh = ops.batch_windows([torch.from_numpy(s).cuda() for s in srcs], torch.from_numpy(row_off), tabs[0], tabs[1], tabs[2], T)
    assert all(torch.equal(f, o) for f, o in zip(fresh, outs))


@pytest.mark.parametrize('dims', [(1, 3), (3, 86), (86, 601), (601, 1), (601, 86, 1)])
def test_gather_kernel_against_numpy(dims):
    assert ROWS_T7[1][1] + ROWS_T7[1][2] == UTT_LENS[-1] and all(sh + n <= UTT_LENS[u] for u, sh, n in ROWS_T7)
    gather_and_check(UTT_LENS, packed(UTT_LENS, dims, 1), ROWS_T7, 7)


@pytest.mark.parametrize('dims', [(601, 86), (3, 1, 86)])
def test_gather_kernel_one_row_and_one_frame(dims):
    srcs = packed(UTT_LENS, dims, 2)
    gather_and_check(UTT_LENS, srcs, [(4, 2, 7)], 7)                              # B = 1
    gather_and_check(UTT_LENS, srcs, [(0, 0, 1), (6, 29, 1), (1, 1, 1), (7, 3, 1)], 1)      # T = 1


def test_gather_kernel_at_the_production_row_length():
    lens = [400, 523, 410]
    gather_and_check(lens, packed(lens, (601, 86, 1), 3), [(0, 0, 400), (1, 123, 400), (2, 100, 310)], 400)


# ---- the corpus against load_inoutset -------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def files(tmp_path_factory):
    return tdc.make_files(tmp_path_factory.mktemp('corpus'))


@functools.lru_cache(maxsize=None)
def corpus_of(files, cropmode):
    from percivaltts_amd import data
    indir, outdir, wdir, fids = files
    return data.DeviceCorpus(indir, outdir, wdir, list(fids), cropmode=cropmode, device='cuda')


def equal(dev, host):
    return dev.is_cuda and dev.dtype == torch.float32 and np.array_equal(dev.cpu().numpy(), host)


@pytest.mark.parametrize('cropmode', tdc.CROPMODES)
@pytest.mark.parametrize('padtype', tdc.PADTYPES)
def test_batches_are_those_of_load_inoutset(files, cropmode, padtype):
    from percivaltts_amd import data
    indir, outdir, wdir, fids = files
    corpus = corpus_of((indir, outdir, wdir, tuple(fids)), cropmode)
    assert corpus.X.is_cuda and 0 < corpus.nbytes <= corpus.maxbytes
    for k, (ids, lengthmax) in enumerate(((fids, 120), (fids[::-1], None), ([fids[2], fids[2], fids[5]], 77))):
        np.random.seed(k)
        Xh, Yh, Wh = data.load_inoutset(indir, outdir, wdir, ids, length=None, lengthmax=lengthmax, maskpadtype=padtype, cropmode=cropmode)
        after_host = np.random.get_state()
        np.random.seed(k)
        X, Y, W = corpus.batch(ids, None, lengthmax, padtype, want_w=True)
        assert tdc.same_state(np.random.get_state(), after_host)
        assert equal(X, Xh) and equal(Y, Yh) and equal(W, Wh)
        np.random.seed(k)
        XY = corpus.batch([fids.index(f) for f in ids], None, lengthmax, padtype)          # indices; without the weights
        assert len(XY) == 2 and equal(XY[0], Xh) and equal(XY[1], Yh)


@pytest.mark.parametrize('world', [2, 3])
def test_rank_shards_make_the_global_batch(files, world):
    from percivaltts_amd import data, parallel
    indir, outdir, wdir, fids = files
    corpus = corpus_of((indir, outdir, wdir, tuple(fids)), 'begendbigger')
    u = np.random.RandomState(5).random_sample(len(fids))
    for padtype in tdc.PADTYPES:
        Xh, Yh, Wh = data.load_inoutset(indir, outdir, wdir, fids, length=None, lengthmax=150, maskpadtype=padtype, cropmode='begendbigger', rand=u)
        parts = [corpus.batch(fids, None, 150, padtype, rand=u, rows=parallel.shard_batch(len(fids), world, r), want_w=True) for r in range(world)]
        assert all(p[0].shape[0] == len(fids) // world for p in parts)
        for k, host in enumerate((Xh, Yh, Wh)):
            assert equal(torch.cat([p[k] for p in parts]), host)


def test_one_batch_is_one_launch_and_one_small_upload(files, monkeypatch):
    from percivaltts_amd import _hip, data
    indir, outdir, wdir, fids = files
    corpus = corpus_of((indir, outdir, wdir, tuple(fids)), 'begend')
    corpus.batch(fids, None, 120)
    uploads, real_upload = [], data.upload

    def upload(t, dev):
        uploads.append((t.dtype, t.numel()))
        return real_upload(t, dev)
    monkeypatch.setattr(data, 'upload', upload)
    np.random.seed(3)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode('error')           # nothing makes the host wait for the device
    try:
        with _hip.KernelTimer() as kt:
            X, Y, W = corpus.batch(fids, None, 120, want_w=True)
    finally:
        torch.cuda.set_sync_debug_mode('default')
    assert [r[0] for r in kt.records] == ['ptts_batch_windows']                 # one gather for the three streams
    assert uploads == [(torch.int32, 3 * len(fids))]                            # utt, shift and n, nothing else
    np.random.seed(3)
    Xh, Yh, Wh = data.load_inoutset(indir, outdir, wdir, fids, lengthmax=120, maskpadtype='randshift', cropmode='begend')
    assert equal(X, Xh) and equal(Y, Yh) and equal(W, Wh)


# ---- a training run from the resident corpus -----------------------------------------------------------------------------
PARTS = ('.model.weights.npz', '.critic.weights.npz', '.generator.optimizer.npz', '.critic.optimizer.npz')
COSTS = ('model_training', 'critic_training', 'critic_validation', 'model_validation', 'model_rmse_validation')


def test_training_from_the_device_corpus_is_the_host_loaders_run(tmp_path, monkeypatch, capsys):
    """tests/test_run_synthetic.py::test_training_run_with_and_without_the_generator_look_ahead's tiny run, two epochs in
    deterministic mode: fed by the host loader, fed from the resident corpus (cfg.train_data_on_device), and with the switch on
    but a corpus over its memory limit (the host loader again, and a line in the log).  Generator and critic weights with the
    BatchNorm moving statistics, both Adam states and the cost histories must be the same bytes."""
    import importlib, pickle
    from percivaltts_amd import data, ops
    monkeypatch.setenv('PERCIVAL_CORPUS', str(tmp_path / 'corpus'))
    import percivaltts_amd.run as run
    gathered = []
    real_batch = data.DeviceCorpus.batch

    def spy(self, *a, **k):
        gathered.append(1)
        return real_batch(self, *a, **k)
    monkeypatch.setattr(data.DeviceCorpus, 'batch', spy)
    ops.deterministic(True)
    try:
        states, counts, logs = {}, {}, {}
        for name, on, maxbytes in (('host', False, None), ('device', True, None), ('fallback', True, 1000)):
            wd = tmp_path / name
            wd.mkdir()
            monkeypatch.chdir(wd)
            run = importlib.reload(run)
            run.cfg.id_valid_start = 22; run.cfg.id_valid_nb = 1; run.cfg.id_test_nb = 1
            run.cfg.train_min_nbepochs = 1; run.cfg.train_cancel_nodecepochs = 10
            run.cfg.train_nbepochs_scalewdata = False
            run.cfg.train_batch_size = 2; run.cfg.arch_hiddenwidth = 8; run.cfg.arch_gen_nbcnnlayers = 2
            run.cfg.train_batch_lengthmax = 60
            run.cfg.train_max_nbepochs = 2
            run.cfg.train_wgan_hipgraph = False
            run.cfg.train_data_on_device = on
            run.cfg.train_data_on_device_maxbytes = maxbytes
            if not os.path.exists(run.cfg.fileids):
                run.synthesize_corpus(nfiles=24, minlen=90, maxlen=140)
            np.random.seed(123); torch.manual_seed(123)
            del gathered[:]
            capsys.readouterr()
            run.training(cont=False)
            logs[name] = capsys.readouterr().out
            counts[name] = len(gathered)
            st = 'model-trainingstate-last.h5'
            with open(st + '.model.cfgextras.pkl', 'rb') as f:
                _, extras, rng = pickle.load(f)
            states[name] = {k: dict(np.load(st + k)) for k in PARTS}
            states[name]['extras'], states[name]['rng'] = extras, rng
    finally:
        ops.deterministic(False)
    assert counts == {'host': 0, 'device': 22, 'fallback': 0}              # 11 batches an epoch, each one gather
    assert 'resident on the device' in logs['device'] and 'host loader' not in logs['device'] + logs['host']
    assert logs['fallback'].count('are allowed: batches come from the host loader') == 1 and ' 1000 bytes are allowed' in logs['fallback']
    a = states['host']
    for name in ('device', 'fallback'):
        b = states[name]
        assert a['extras']['generator_updates'] == b['extras']['generator_updates'] >= 4
        assert tdc.same_state(a['rng'], b['rng'])                           # the numpy generator: the same draws were made
        for k in COSTS:
            assert len(a['extras']['costs'][k]) == 2 and np.array_equal(np.asarray(b['extras']['costs'][k]), np.asarray(a['extras']['costs'][k])), (name, k)
        for part in PARTS:
            assert sorted(a[part]) == sorted(b[part])
            for k in a[part]:
                assert np.array_equal(b[part][k], a[part][k]), (name, part, k)
