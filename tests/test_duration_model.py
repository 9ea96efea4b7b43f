"""Duration modelling end to end: vocoders.DurationFeatures, modeltts_common.DurationModel (trained by the unchanged OptimizerTTS,
plain and with 'randshiftpad'), DurationModel.generate_durations, and the stages of run.py -- phone_labels_from_state_labels,
durations_extraction, contexts_from_durations -- on the five fixture utterances of tests/golden/labels with the hand-written
question set.  Two epochs on four utterances: nothing here claims that the model converges, only that every stage runs on the
device, hands the next one what it expects, and that the way back (durations -> context rows) uses the stored statistics."""
import os

import numpy as np
import pytest

import percivaltts_amd
from percivaltts_amd import data, modeltts_common, optimizertts, vocoders
from percivaltts_amd.external.merlin import label_normalisation as ln

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = os.path.join(ROOT, 'tests', 'golden', 'labels')
FIDS = ['arctic_a0002', 'arctic_a0004', 'arctic_a0005', 'arctic_a0006', 'arctic_a0008']
QFILE = os.path.join(G, 'questions-handwritten.hed')
Q, W = 37, 37 + 9                       # question columns; the width of the aligned context rows ('full')
STATE_LABS = os.path.join(G, 'label_state_align', '*.lab')


# ---------------------------------------------------------------------------------------------------------------------------
# CPU
# ---------------------------------------------------------------------------------------------------------------------------
def test_duration_features_is_a_vocoder_without_streams():
    voc = vocoders.DurationFeatures(0.005)
    assert isinstance(voc, vocoders.Vocoder) and voc.shift == 0.005 and voc.mlpg_wins is None
    assert voc.featuressizeraw() == voc.featuressize() == 5 and vocoders.DurationFeatures(0.01, nstates=1).featuressizeraw() == 1
    assert (voc.f0size(), voc.specsize(), voc.noisesize(), voc.vuvsize()) == (0, 0, 0, 0)
    assert not hasattr(voc, 'synthesis_device') and not hasattr(voc, 'decompress_spectrum')
    for bad in (0, 2.5, -1):
        with pytest.raises(ValueError):
            vocoders.DurationFeatures(0.005, nstates=bad)
    voc.objmeasures_clear()
    ref = np.array([[1, 2, 3, 4, 5], [2, 2, 2, 2, 2], [1, 1, 1, 1, 1]], dtype=np.float32)
    gen = ref + np.array([[1, 0, 0, 0, 0], [0, 0, -2, 0, 0], [0, 0, 0, 0, 3]], dtype=np.float32)
    voc.objmeasures_add(gen, ref)
    voc.objmeasures_add(ref, ref)
    stats = voc.objmeasures_stats()
    assert set(stats) == {'DUR_STATE[frames]', 'DUR_PHONE[ms]', 'DUR_PHONE[corr]'}
    np.testing.assert_allclose(stats['DUR_STATE[frames]'], 0.5 * np.sqrt(14.0 / 15.0), rtol=1e-12)       # the second utterance adds 0
    np.testing.assert_allclose(stats['DUR_PHONE[ms]'], 0.5 * np.sqrt(14.0 / 3.0) * 5.0, rtol=1e-12)
    np.testing.assert_allclose(stats['DUR_PHONE[corr]'], 0.5 * (np.corrcoef([16, 8, 8], [15, 10, 5])[0, 1] + 1.0), rtol=1e-9)
    with pytest.raises(ValueError):
        voc.objmeasures_add(gen[:, :4], ref[:, :4])
    voc.objmeasures_clear()
    voc.objmeasures_add(np.ones((3, 5)), np.ones((3, 5)))                   # constant durations: no correlation to speak of
    assert set(voc.objmeasures_stats()) == {'DUR_STATE[frames]', 'DUR_PHONE[ms]'}


def test_phone_labels_from_state_labels(tmp_path, monkeypatch):
    monkeypatch.setenv('PERCIVAL_CORPUS', str(tmp_path / 'corpus'))
    import percivaltts_amd.run as run
    out = str(tmp_path / 'phone' / '*.lab')
    run.phone_labels_from_state_labels(STATE_LABS, FIDS, out)
    for fid in FIDS:                    # the committed phone-aligned fixtures were derived from the state-aligned ones by this rule
        with open(out.replace('*', fid)) as f, open(os.path.join(G, 'label_phone_align', fid + '.lab')) as g:
            assert f.read() == g.read(), fid
    bad = tmp_path / 'bad' / 'x.lab'
    bad.parent.mkdir()
    with open(STATE_LABS.replace('*', FIDS[2])) as f:
        bad.write_text(''.join(f.readlines()[:-1]))
    with pytest.raises(ValueError):
        run.phone_labels_from_state_labels(str(tmp_path / 'bad' / '*.lab'), ['x'], out)
    assert callable(run.build_duration_model) and callable(run.training_durations) and callable(run.durations_extraction)
    with pytest.raises(ValueError):
        run.generate(dur_fparams='model-dur.h5')                            # the labels to expand are not named


# ---------------------------------------------------------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def corpus(tmp_path_factory):
    """Both corpora of the five fixture utterances, written once: the duration model's (durations_extraction) and the acoustic
    model's aligned inputs (contexts_extraction), whose stored min / max the way back normalises with."""
    d = str(tmp_path_factory.mktemp('durcorpus'))
    import percivaltts_amd.run as run
    paths = dict(root=d, phonelab=d + '/lab_phone/*.lab', durin=d + '/dur_in/*.lab:(-1,{})'.format(Q), durout=d + '/dur_out/*.dur:(-1,5)',
                 durw=d + '/dur_w/*.w:(-1,1)', inpath=d + '/lab_norm/*.lab:(-1,{})'.format(W))
    paths['res'] = run.durations_extraction(STATE_LABS, FIDS, QFILE, paths['phonelab'], d + '/dur_in_bin/*.lab', d + '/dur_raw/*.dur',
                                            paths['durw'], paths['durin'], paths['durout'], id_valid_start=4)
    run.contexts_extraction(STATE_LABS, FIDS, QFILE, d + '/lab_bin/*.lab', d + '/lab_w/*.w:(-1,1)', paths['inpath'], lab_type='state',
                            id_valid_start=4)
    paths['run'] = run
    return paths


@pytest.mark.gpu
def test_durations_extraction_writes_inputs_targets_and_weights(corpus):
    d = corpus['root']
    n = ln.HTSLabelNormalisation(QFILE)
    X, Y, Wt = data.load(corpus['durin'], FIDS), data.load(corpus['durout'], FIDS), data.load(corpus['durw'], FIDS)
    mean, std = (np.fromfile(d + '/dur_out/' + f, dtype=np.float32) for f in ('mean4norm.dat', 'std4norm.dat'))
    assert mean.shape == std.shape == (5,) and (std > 0).all()
    mins, maxs = (np.fromfile(d + '/dur_in/' + f, dtype=np.float32) for f in ('min4norm.dat', 'max4norm.dat'))
    assert mins.shape == maxs.shape == (Q,)
    live = maxs > mins
    assert 25 < live.sum() < Q
    assert corpus['res']['in']['size'] == Q and corpus['res']['out']['size'] == 5
    for fid, x, y, w in zip(FIDS, X, Y, Wt):
        dur = n.extract_dur_features(os.path.join(G, 'label_state_align', fid + '.lab'))
        P = len(dur)
        assert x.shape == (P, Q) and y.shape == (P, 5) and w.shape == (P, 1) and (w == 1.0).all()
        assert np.abs(x[:, live]).max() <= 1.0                               # min-max to [-1, 1] wherever the column varies
        assert np.array_equal(np.fromfile(d + '/dur_raw/{}.dur'.format(fid), dtype=np.float32).reshape(-1, 5), dur)
        np.testing.assert_allclose(y * std + mean, dur, rtol=0, atol=1e-4)
    stacked = np.vstack(Y[:4])
    np.testing.assert_allclose(stacked.mean(axis=0), 0.0, atol=1e-4)               # the statistics are the first four files'


@pytest.mark.gpu
@pytest.mark.parametrize('padtype', ['randshift', 'randshiftpad'])
def test_train_generate_and_expand(corpus, padtype, tmp_path, monkeypatch):
    run, d = corpus['run'], corpus['root']
    monkeypatch.chdir(tmp_path)
    np.random.seed(3); __import__('torch').manual_seed(3)
    cfg = percivaltts_amd.configuration()
    cfg.arch_hiddenwidth = 32
    cfg.train_batch_size = 2
    cfg.train_min_nbepochs = 1; cfg.train_max_nbepochs = 2; cfg.train_cancel_nodecepochs = 10
    cfg.train_nbepochs_scalewdata = False
    cfg.train_batch_padtype = padtype
    cfg.train_batch_lengthmax = 30                                          # phones: a0005 (17) and a0008 (24) are shorter, the others longer
    if padtype == 'randshiftpad': cfg.train_batch_length = 30
    cfg.train_log_plot = False
    mod = modeltts_common.DurationModel(Q, cfg, layertypes=['FC', 'BLSTM'], nstates=5)
    assert isinstance(mod.vocoder, vocoders.DurationFeatures) and mod.vocoder.featuressize() == 5
    costs, seen = [], []
    plain = optimizertts.OptimizerTTS.train_on_batch

    def spy(self, batchid, X, Y, lengths=None):
        seen.append((tuple(X.shape), tuple(Y.shape), None if lengths is None else np.asarray(lengths).copy()))
        costs.append(plain(self, batchid, X, Y, lengths=lengths))
        return costs[-1]
    monkeypatch.setattr(optimizertts.OptimizerTTS, 'train_on_batch', spy)
    opti = optimizertts.OptimizerTTS(cfg, mod)
    opti.train(corpus['durin'], corpus['durout'], corpus['durw'], FIDS[:4], FIDS[4:], 'model-dur.h5')
    assert len(costs) == 4 and np.isfinite(costs).all()                     # two epochs of two batches
    assert all(x[2] == Q and y[2] == 5 and x[:2] == y[:2] for x, y, _ in seen)
    if padtype == 'randshiftpad':
        ns = np.concatenate([n for _, _, n in seen])
        assert all(x[1] == 30 for x, _, _ in seen) and ns.max() == 30 and 1 <= ns.min() < 30
    else:
        assert all(n is None for _, _, n in seen)

    durdir = str(tmp_path / 'gen-dur')
    stats = mod.generate_durations(corpus['durin'], corpus['durout'], FIDS, durdir, batch_size=3)
    assert set(stats) >= {'DUR_STATE[frames]', 'DUR_PHONE[ms]'} and all(np.isfinite(v) for v in stats.values())
    durs = []
    for fid in FIDS:
        dur = np.fromfile(os.path.join(durdir, fid + '.dur'), dtype=np.float32).reshape(-1, 5)
        with open(os.path.join(G, 'label_phone_align', fid + '.lab')) as f:
            assert len(dur) == len(f.readlines())
        assert (dur == np.rint(dur)).all() and dur.min() >= 1
        durs.append(dur)
    assert mod.generate_durations(corpus['durin'], corpus['durout'], FIDS[:1], durdir, do_objmeas=False) is None

    # the way back: labels without times + the predicted durations -> context rows, normalised with the STORED statistics
    out = str(tmp_path / 'gen-lab' / '*.lab')
    nbrows = run.contexts_from_durations(corpus['phonelab'], FIDS, QFILE, durdir + '/*.dur', corpus['inpath'], out, batch_size=3)
    assert nbrows == [int(x.sum()) for x in durs]
    rows = data.load(out + ':(-1,{})'.format(W), FIDS)
    aligned = data.load(corpus['inpath'], FIDS)
    raw = ln.HTSLabelNormalisation(QFILE)
    mins, maxs = (np.fromfile(d + '/lab_norm/' + f, dtype=np.float32) for f in ('min4norm.dat', 'max4norm.dat'))
    live = maxs > mins
    for fid, x, a, dur in zip(FIDS, rows, aligned, durs):
        assert x.shape == (int(dur.sum()), W) and a.shape[1] == W and np.isfinite(x).all()
        path = str(tmp_path / (fid + '.dur'))
        dur.tofile(path)
        un = raw.extract_linguistic_features(os.path.join(G, 'label_phone_align', fid + '.lab'), dur_file_name=path)
        want = (((un - mins) / np.where(live, maxs - mins, 1).astype(np.float32)) - np.float32(0.5)) * np.float32(2.0)
        assert np.array_equal(x[:, live], want[:, live])                    # numpy's operation order in fp32, as compose_normalise states
    # one stored maximum changed: the output changes in that column, and the statistics files are not rewritten
    col = Q + 2                                                             # the state's frame count
    before = open(d + '/lab_norm/max4norm.dat', 'rb').read()
    changed = maxs.copy(); changed[col] *= 2.0
    try:
        changed.tofile(d + '/lab_norm/max4norm.dat')
        out2 = str(tmp_path / 'gen-lab2' / '*.lab')
        run.contexts_from_durations(corpus['phonelab'], FIDS[:2], QFILE, durdir + '/*.dur', corpus['inpath'], out2)
        assert open(d + '/lab_norm/max4norm.dat', 'rb').read() == changed.tobytes()
        for x, x2 in zip(rows, data.load(out2 + ':(-1,{})'.format(W), FIDS[:2])):
            same = np.ones(W, bool); same[col] = False
            assert np.array_equal(x[:, same], x2[:, same]) and not np.array_equal(x[:, col], x2[:, col])
    finally:
        with open(d + '/lab_norm/max4norm.dat', 'wb') as f: f.write(before)
    # the acoustic model takes the rows as it takes the aligned ones
    voc = vocoders.VocoderPML(16000, 0.005, 12, 4)
    cfg.arch_hiddenwidth = 8
    acoustic = modeltts_common.Generic(W, voc, layertypes=['FC', 'FC'], cfgarch=cfg)
    y = acoustic.predict(rows[2][None])
    assert y.shape == (1, rows[2].shape[0], voc.featuressize()) and np.isfinite(y).all()


@pytest.mark.gpu
def test_run_generates_from_labels_without_times(tmp_path, monkeypatch):
    """The run.py stages in a row on the five fixture utterances with the shipped question set (425 context columns, what the
    script's model reads): both corpora, one epoch of the acoustic model (least squares, the shrunk configuration of
    tests/test_run_synthetic.py, random targets of the aligned lengths) and one of the duration model, then
    generate(dur_fparams=...): the test utterance's phone labels go through predicted durations to context rows, parameters and
    a waveform whose lengths are the predicted durations'."""
    import importlib
    import wave
    monkeypatch.setenv('PERCIVAL_CORPUS', str(tmp_path / 'corpus'))
    monkeypatch.chdir(tmp_path)
    import percivaltts_amd.run as run
    run = importlib.reload(run)
    run.errtype = 'LSE'
    run.cfg.id_valid_start = 3; run.cfg.id_valid_nb = 1; run.cfg.id_test_nb = 1
    run.cfg.train_min_nbepochs = 1; run.cfg.train_max_nbepochs = 1; run.cfg.train_cancel_nodecepochs = 3
    run.cfg.train_nbepochs_scalewdata = False
    run.cfg.train_batch_size = 1; run.cfg.arch_hiddenwidth = 4; run.cfg.arch_gen_nbcnnlayers = 1
    run.cfg.train_batch_lengthmax = 60
    cp, qfile = run.cp, os.path.join(G, 'questions-radio_dnn_416.hed')
    os.makedirs(cp)
    with open(run.cfg.fileids, 'w') as f: f.write('\n'.join(FIDS) + '\n')
    res = run.contexts_extraction(STATE_LABS, FIDS, qfile, cp + 'label_state_align_bin425/*.lab', run.cfg.wpath, run.cfg.inpath,
                                  lab_type='state', id_valid_start=3)
    assert res['size'] == run.ctxsize
    rng = np.random.RandomState(1)
    os.makedirs(os.path.dirname(run.cfg.outpath))
    for fid, x in zip(FIDS, data.load(run.cfg.inpath, FIDS)):
        y = rng.randn(x.shape[0], run.out_size).astype(np.float32)
        y[:, 1 + run.vocoder.specsize():] = rng.rand(x.shape[0], run.vocoder.noisesize())
        y.tofile(run.cfg.outpath.split(':')[0].replace('*', fid))
    np.zeros(run.out_size, dtype=np.float32).tofile(os.path.join(os.path.dirname(run.cfg.outpath), 'mean4norm.dat'))
    np.ones(run.out_size, dtype=np.float32).tofile(os.path.join(os.path.dirname(run.cfg.outpath), 'std4norm.dat'))
    phonelabs = cp + 'label_phone_align/*.lab'
    run.durations_extraction(STATE_LABS, FIDS, qfile, phonelabs, cp + 'label_phone_bin416/*.lab', cp + 'label_state_align_dur5/*.dur',
                             run.cfg.dur_wpath, run.cfg.dur_inpath, run.cfg.dur_outpath, id_valid_start=3)
    run.training()
    run.training_durations()
    assert os.path.exists('model.h5.weights.npz') and os.path.exists('model-dur.h5.weights.npz')
    with pytest.raises(ValueError):
        run.generate(dur_fparams=run.cfg.dur_fparams_fullset)
    run.generate(dur_fparams=run.cfg.dur_fparams_fullset, lab_path=phonelabs, lab_questions=qfile)
    fid = FIDS[4]
    dur = np.fromfile('model-gen-dur/{}.dur'.format(fid), dtype=np.float32).reshape(-1, 5)
    T = int(dur.sum())
    assert dur.shape == (24, 5) and dur.min() >= 1 and (dur == np.rint(dur)).all()
    lab = np.fromfile('model-gen-lab/{}.lab'.format(fid), dtype=np.float32).reshape(-1, run.ctxsize)
    cmp_ = np.fromfile('model-gen/{}.cmp'.format(fid), dtype=np.float32).reshape(-1, run.out_size)
    par = np.fromfile('model-demo-params/{}.cmp'.format(fid), dtype=np.float32).reshape(-1, run.vocoder.featuressizeraw())
    assert lab.shape[0] == cmp_.shape[0] == par.shape[0] == T and np.isfinite(lab).all() and np.isfinite(cmp_).all()
    w = wave.open('model-demo-snd/{}.wav'.format(fid))
    try:
        assert w.getframerate() == 16000 and abs(w.getnframes() - T * 80) <= 400      # 5 ms frames at 16 kHz
    finally:
        w.close()
