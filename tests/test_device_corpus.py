"""Host side of the device-resident training set (data.DeviceCorpus, ops.batch_windows): the window plan against data.batching,
the packed rows against croplen + croplen_weight, window_length against batch_window_length, the memory limit and the host
validation of the gather's tables.  Nothing here launches a kernel; every comparison is exact."""
import os

import numpy as np
import pytest
import torch

from percivaltts_amd import data, ops

CROPMODES = ('begend', 'begendbigger', 'all')
PADTYPES = ('randshift', 'padright')
CTX, OUT = 7, 5
LENS = [420, 381, 455, 400, 392, 470]


def make_files(root, ctx=CTX, out=OUT, lens=LENS, seed=3):
    """Tiny files in the corpus layout: weight tracks with silence at both ends, an inner gap shorter than croplen_weight's
    cropsize (150 frames) and one longer; the X / Y / W files of an utterance differ in length by a frame."""
    rng = np.random.RandomState(seed)
    root = str(root)
    fids = ['u{}'.format(k) for k in range(len(lens))]
    for sub, dim in (('lab', ctx), ('cmp', out), ('w', 1)):
        os.makedirs(os.path.join(root, sub))
        for k, (fid, n) in enumerate(zip(fids, lens)):
            extra = {'lab': k % 2, 'cmp': (k + 1) % 2, 'w': 1 if k % 3 == 0 else 0}[sub]
            arr = rng.rand(n + extra, dim).astype(np.float32)
            if sub == 'w':
                arr[:] = 1.0
                arr[:4 + k] = 0.0                       # leading silence
                arr[n - 3 - k:] = 0.0                   # trailing silence
                arr[30:40 + k] = 0.2                    # a short pause: only 'all' drops it
                arr[100:260 + 3 * k] = 0.1              # a pause longer than cropsize: 'begendbigger' drops it too
            arr.tofile(os.path.join(root, sub, fid + '.' + sub))
    indir = os.path.join(root, 'lab', '*.lab') + ':(-1,{})'.format(ctx)
    outdir = os.path.join(root, 'cmp', '*.cmp') + ':(-1,{})'.format(out)
    wdir = os.path.join(root, 'w', '*.w') + ':(-1,1)'
    return indir, outdir, wdir, fids


def same_state(a, b):
    return a[0] == b[0] and np.array_equal(a[1], b[1]) and a[2:] == b[2:]


# ---- the plan against batching, on index arrays --------------------------------------------------------------------------
IDX_LENS = list(range(3, 12))                                # utterance u has 3 + u frames


def index_corpus():
    xs = [np.arange(n, dtype=np.float32)[:, None] for n in IDX_LENS]
    return xs, data.DeviceCorpus.from_utterances(xs, xs, xs, device='cpu')


def rows_of_plan(T, shift, n):
    want = np.zeros((len(n), T, 1), dtype=np.float32)
    for b in range(len(n)):
        want[b, :n[b], 0] = np.arange(shift[b], shift[b] + n[b])
    return want


def ids_for(padtype, T):
    ids = [8, 0, 4, 4, 2, 7, 1, 3, 5, 6]                     # every utterance, one of them twice, not in order
    if padtype == 'randshift' and T is not None:
        ids = [u for u in ids if IDX_LENS[u] >= T]           # (a shorter one raises: test_plan_refuses_...)
    return ids


@pytest.mark.parametrize('padtype', PADTYPES)
@pytest.mark.parametrize('length,lengthmax', [(None, None), (None, 5), (7, None), (7, 5)])
def test_plan_chooses_the_windows_of_batching(padtype, length, lengthmax):
    xs, corpus = index_corpus()
    T_explicit = None if length is None else (length if lengthmax is None else min(length, lengthmax))
    ids = ids_for(padtype, T_explicit)
    if length == 7 and lengthmax is None:
        assert 4 in ids                                      # the utterance of exactly T frames: a single possible shift
        if padtype == 'padright':
            assert min(IDX_LENS[u] for u in ids) < 7         # utterances shorter than T
    sel = [xs[u] for u in ids]
    u01 = np.random.RandomState(9).random_sample(len(ids))
    u01[0], u01[1] = 0.0, np.nextafter(1, 0)
    for rand in (None, u01):
        np.random.seed(21)
        [want], _ = data.batching([sel], length=length, lengthmax=lengthmax, padtype=padtype, rand=rand)
        after_host = np.random.get_state()
        np.random.seed(21)
        T, utt, shift, n = corpus.plan(ids, length, lengthmax, padtype, rand=rand)
        assert same_state(np.random.get_state(), after_host)
        assert T == want.shape[1] == corpus.window_length(ids, length, lengthmax, padtype)
        assert utt.dtype == shift.dtype == n.dtype == np.int32 and list(utt) == ids
        assert np.array_equal(n, [min(IDX_LENS[u], T) for u in ids])
        assert (shift >= 0).all() and (shift + n <= np.array([IDX_LENS[u] for u in ids])).all()
        assert np.array_equal(rows_of_plan(T, shift, n), want)
        if padtype == 'padright':
            assert not shift.any()
    if padtype == 'randshift':
        np.random.seed(21)
        before = np.random.get_state()
        corpus.plan(ids, length, lengthmax, padtype, rand=u01)          # explicit uniforms: nothing is drawn
        assert same_state(np.random.get_state(), before)


@pytest.mark.parametrize('rand', [False, True])
def test_plan_refuses_a_window_longer_than_an_utterance(rand):
    xs, corpus = index_corpus()
    ids = [8, 6, 1, 7]                                       # 11, 9, 4 and 10 frames against length 7
    u01 = np.full(len(ids), 0.5) if rand else None
    np.random.seed(4)
    with pytest.raises(Exception) as host:
        data.batching([[xs[u] for u in ids]], length=7, padtype='randshift', rand=u01)
    after_host = np.random.get_state()
    np.random.seed(4)
    with pytest.raises(host.type):
        corpus.plan(ids, 7, None, 'randshift', rand=u01)
    assert host.type is ValueError and same_state(np.random.get_state(), after_host)      # two rows were drawn before the short one
    assert corpus.plan(ids, 7, None, 'padright')[0] == 7                                  # 'padright' pads it instead


# ---- packing, lengths, limits -----------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def files(tmp_path_factory):
    return make_files(tmp_path_factory.mktemp('corpus'))


def cropped(files, cropmode):
    indir, outdir, wdir, fids = files
    X, Y, W = data.load(indir, fids), data.load(outdir, fids), data.load(wdir, fids)
    X, Y, W = data.croplen([X, Y, W])
    [X, Y], W = data.croplen_weight([X, Y], W, cropmode=cropmode)
    return X, Y, W


@pytest.mark.parametrize('cropmode', CROPMODES)
def test_packed_rows_are_the_cropped_utterances(files, cropmode):
    indir, outdir, wdir, fids = files
    X, Y, W = cropped(files, cropmode)
    corpus = data.DeviceCorpus(indir, outdir, wdir, fids, cropmode=cropmode, device='cpu')
    assert len(corpus) == len(fids) and list(corpus.lens) == [x.shape[0] for x in X]
    assert list(corpus.row_off) == [0] + list(np.cumsum([x.shape[0] for x in X]))
    for got, want, dim in ((corpus.X, X, CTX), (corpus.Y, Y, OUT), (corpus.W, W, 1)):
        assert got.dtype == torch.float32 and got.is_contiguous() and tuple(got.shape) == (sum(corpus.lens), dim)
        assert np.array_equal(got.numpy(), np.concatenate(want, axis=0))
    assert corpus.raw_out_frames == [y.shape[0] for y in data.load(outdir, fids)]
    assert corpus.nbytes == 4 * int(sum(corpus.lens)) * (CTX + OUT + 1)
    lens = {cm: [x.shape[0] for x in cropped(files, cm)[0]] for cm in CROPMODES}
    assert all(a > b > c for a, b, c in zip(lens['begend'], lens['begendbigger'], lens['all'])), lens      # each gap matters


@pytest.mark.parametrize('cropmode', CROPMODES)
@pytest.mark.parametrize('padtype', PADTYPES)
def test_window_length_is_batch_window_length(files, cropmode, padtype):
    indir, outdir, wdir, fids = files
    corpus = data.DeviceCorpus(indir, outdir, wdir, fids, cropmode=cropmode, device='cpu')
    for ids in (fids, fids[1:4], [fids[5], fids[2]]):
        for length, lengthmax in ((None, None), (None, 120), (None, 10 ** 6), (90, None), (90, 60)):
            want = data.batch_window_length(indir, outdir, wdir, ids, length=length, lengthmax=lengthmax, maskpadtype=padtype, cropmode=cropmode)
            assert corpus.window_length(ids, length, lengthmax, padtype) == want
            assert corpus.window_length([fids.index(f) for f in ids], length, lengthmax, padtype) == want       # indices name the same utterances


def test_a_corpus_over_the_limit_raises_before_any_upload(files, monkeypatch):
    indir, outdir, wdir, fids = files

    def no_upload(*a, **k):
        raise AssertionError('upload attempted')
    monkeypatch.setattr(data, 'upload', no_upload)
    with pytest.raises(data.DeviceCorpusTooLarge) as e:
        data.DeviceCorpus(indir, outdir, wdir, fids, device='cpu', maxbytes=1)
    assert e.value.maxbytes == 1 and e.value.needed == 4 * sum(x.shape[0] for x in cropped(files, 'begend')[0]) * (CTX + OUT + 1)
    assert isinstance(e.value, ValueError)


# ---- ops.batch_windows: the tables are checked on the host ----------------------------------------------------------------
def tables(utt=(0, 1), shift=(0, 2), n=(4, 3), dtype=torch.int32):
    return [torch.tensor(v, dtype=dtype) for v in (utt, shift, n)]


def test_batch_windows_refuses_bad_tables_without_a_launch(monkeypatch):
    def no_launch(*a, **k):
        raise AssertionError('launched')
    monkeypatch.setattr(ops, 'call', no_launch)
    src = torch.zeros(10, 3)
    row_off = torch.tensor([0, 4, 10])                       # utterances of 4 and 6 frames
    T = 4
    with pytest.raises(ValueError, match='ends behind its utterance'):
        ops.batch_windows([src], row_off, *tables(shift=(1, 2)), T=T)            # 1 + 4 > 4
    with pytest.raises(ValueError, match='ends behind its utterance'):
        ops.batch_windows([src], row_off, *tables(shift=(0, 6), n=(4, 1)), T=T)  # a shift past the utterance's end
    with pytest.raises(ValueError, match='n > T'):
        ops.batch_windows([src], row_off, *tables(utt=(1, 1), n=(5, 3)), T=T)
    with pytest.raises(ValueError, match='negative'):
        ops.batch_windows([src], row_off, *tables(shift=(-1, 2), n=(3, 3)), T=T)
    with pytest.raises(ValueError, match='outside'):
        ops.batch_windows([src], row_off, *tables(utt=(0, 2)), T=T)
    with pytest.raises(ValueError, match='contiguous float32'):
        ops.batch_windows([torch.zeros(10, 6)[:, ::2]], row_off, *tables(), T=T)
    with pytest.raises(ValueError, match='contiguous float32'):
        ops.batch_windows([src.double()], row_off, *tables(), T=T)
    with pytest.raises(ValueError, match='int32'):
        ops.batch_windows([src], row_off, *tables(dtype=torch.int64), T=T)
    with pytest.raises(ValueError, match='int64'):
        ops.batch_windows([src], row_off.to(torch.int32), *tables(), T=T)
    with pytest.raises(ValueError, match='packed rows'):
        ops.batch_windows([src, torch.zeros(9, 2)], row_off, *tables(), T=T)     # streams of different row counts
    with pytest.raises(ValueError, match='streams'):
        ops.batch_windows([src] * 4, row_off, *tables(), T=T)
    # good tables, host tensors: there is no CPU path
    from percivaltts_amd._hip import HipLibraryError
    with pytest.raises(HipLibraryError):
        ops.batch_windows([src], row_off, *tables(), T=T)
    corpus = data.DeviceCorpus.from_utterances([np.zeros((4, 3), np.float32)], [np.zeros((4, 2), np.float32)], [np.ones((4, 1), np.float32)], device='cpu')
    with pytest.raises(HipLibraryError):
        corpus.batch([0], lengthmax=3)
