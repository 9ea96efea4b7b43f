"""padtype 'randshiftpad' (masked training): the window is the given length, or the LONGEST cropped sample capped by lengthmax; a
longer sample gives a random window, a shorter one all its frames and zeros behind them; every row takes exactly one
np.random.randint(0, max(len - T, 0) + 1) draw in row order (or rand[b]), so the generator's state after a batch depends on the
batch size alone.  load_inoutset(outlengths=True) returns the real frames per row, DeviceCorpus.plan makes the same choice from the
same generator, and BatchPrefetcher hands the positions named in host_items through on the host.  Unset, nothing changes."""
import os

import numpy as np
import pytest
import torch

from percivaltts_amd import data

LENS = [37, 9, 52, 20, 21]          # cropped lengths after the three leading silent frames: 33, 5, 48, 16, 17 ('begend' drops one more)


def utterances(lens=LENS, seed=0):
    rng = np.random.RandomState(seed)
    return [rng.rand(n, 3).astype(np.float32) + 1.0 for n in lens], [rng.rand(n, 2).astype(np.float32) + 1.0 for n in lens]


def draws(lens, T):
    """the shifts batching must choose: one randint per row, in row order"""
    return [np.random.randint(0, max(n - T, 0) + 1) for n in lens]


def test_windows_lengths_and_one_draw_per_row():
    X, Y = utterances()
    for length, lengthmax, T in ((None, 20, 20), (None, None, 52), (12, None, 12), (30, 25, 25)):
        np.random.seed(5)
        [Xb, Yb], M = data.batching([list(X), list(Y)], length=length, lengthmax=lengthmax, padtype='randshiftpad', outmask=True)
        after = np.random.randint(0, 1 << 30)
        np.random.seed(5)
        shifts = draws(LENS, T)
        assert after == np.random.randint(0, 1 << 30), 'not one draw per row'
        assert Xb.shape == (len(LENS), T, 3) and Yb.shape == (len(LENS), T, 2) and Xb.dtype == np.float32
        for b, (n, s) in enumerate(zip(LENS, shifts)):
            k = min(n, T)
            np.testing.assert_array_equal(Xb[b, :k], X[b][s:s + k])
            np.testing.assert_array_equal(Yb[b, :k], Y[b][s:s + k])
            assert not Xb[b, k:].any() and not Yb[b, k:].any()
            assert M[b].sum() == k and M[b, :k].all()
    # rows longer than the window do move (padright always gives their first frames)
    np.random.seed(5)
    assert any(s > 0 for s, n in zip(draws(LENS, 20), LENS) if n > 20)


def test_rand_replaces_the_draws():
    X, Y = utterances()
    u = np.array([0.0, 0.7, 0.999999, 0.5, 0.25])
    state = np.random.get_state()[1].copy()
    [Xb], _ = data.batching([list(X)], lengthmax=20, padtype='randshiftpad', rand=u)
    np.testing.assert_array_equal(np.random.get_state()[1], state)                 # no draw
    for b, n in enumerate(LENS):
        ns = max(n - 20, 0) + 1
        s = min(int(u[b] * ns), ns - 1)
        np.testing.assert_array_equal(Xb[b, :min(n, 20)], X[b][s:s + min(n, 20)])


def _files(tmp_path):
    rng = np.random.RandomState(1)
    fids = ['u{}'.format(i) for i in range(len(LENS))]
    for sub, dim in (('lab', 7), ('cmp', 5), ('w', 1)):
        os.makedirs(str(tmp_path / sub))
        for fid, n in zip(fids, LENS):
            arr = rng.rand(n, dim).astype(np.float32) + 1.0
            if sub == 'w':
                arr[:] = 1.0
                arr[:3] = 0.0
            arr.tofile(str(tmp_path / sub / (fid + '.' + sub)))
    return (fids, str(tmp_path / 'lab' / '*.lab') + ':(-1,7)', str(tmp_path / 'cmp' / '*.cmp') + ':(-1,5)',
            str(tmp_path / 'w' / '*.w') + ':(-1,1)')


def test_load_inoutset_returns_the_lengths_when_asked(tmp_path):
    fids, indir, outdir, wdir = _files(tmp_path)
    kept = [n - 4 for n in LENS]                          # 'begend': first to last frame above the threshold, the last one excluded
    np.random.seed(3)
    out = data.load_inoutset(indir, outdir, wdir, fids, lengthmax=20, maskpadtype='randshiftpad', cropmode='begend', outlengths=True)
    assert len(out) == 4
    X, Y, W, n = out
    assert X.shape == (5, 20, 7) and Y.shape == (5, 20, 5) and W.shape == (5, 20, 1)
    assert n.dtype == np.int32 and n.tolist() == [min(k, 20) for k in kept]
    for b, k in enumerate(n):
        assert (X[b, :k] >= 1.0).all() and not X[b, k:].any() and not Y[b, k:].any()
    assert data.batch_window_length(indir, outdir, wdir, fids, lengthmax=20, maskpadtype='randshiftpad', cropmode='begend') == 20
    assert data.batch_window_length(indir, outdir, wdir, fids, maskpadtype='randshiftpad', cropmode='begend') == max(kept)
    # unset, three values as ever -- with any padtype
    np.random.seed(3)
    again = data.load_inoutset(indir, outdir, wdir, fids, lengthmax=20, maskpadtype='randshiftpad', cropmode='begend')
    assert len(again) == 3
    np.testing.assert_array_equal(again[0], X)
    assert len(data.load_inoutset(indir, outdir, wdir, fids, lengthmax=3, maskpadtype='randshift', cropmode='begend')) == 3
    # the lengths of the other padtypes are the same min(len, T)
    n2 = data.load_inoutset(indir, outdir, wdir, fids, maskpadtype='padright', cropmode='begend', outlengths=True)[3]
    assert n2.tolist() == kept
    with pytest.raises(ValueError):
        data.load_inoutset(indir, outdir, wdir, fids, inouttimesync=False, outlengths=True)


def test_device_corpus_plans_what_batching_draws(tmp_path):
    fids, indir, outdir, wdir = _files(tmp_path)
    corpus = data.DeviceCorpus(indir, outdir, wdir, fids, cropmode='begend', device='cpu')
    ids = [3, 0, 2, 1]
    for length, lengthmax in ((None, 20), (None, None), (12, None)):
        np.random.seed(9)
        X, Y, W, n = data.load_inoutset(indir, outdir, wdir, [fids[i] for i in ids], length=length, lengthmax=lengthmax,
                                        maskpadtype='randshiftpad', cropmode='begend', outlengths=True)
        after = np.random.randint(0, 1 << 30)
        np.random.seed(9)
        T, utt, shift, pn = corpus.plan(ids, length, lengthmax, 'randshiftpad')
        assert after == np.random.randint(0, 1 << 30)
        assert T == X.shape[1] == corpus.window_length(ids, length, lengthmax, 'randshiftpad')
        assert pn.tolist() == n.tolist() and utt.tolist() == ids
        packed = corpus.X.numpy()
        for b in range(len(ids)):
            lo = int(corpus.row_off[utt[b]]) + int(shift[b])
            np.testing.assert_array_equal(packed[lo:lo + pn[b]], X[b, :pn[b]])
    u = np.array([0.3, 0.9, 0.0, 0.6])
    Xr = data.load_inoutset(indir, outdir, wdir, [fids[i] for i in ids], lengthmax=20, maskpadtype='randshiftpad', cropmode='begend', rand=u)[0]
    T, utt, shift, pn = corpus.plan(ids, None, 20, 'randshiftpad', rand=u)
    for b in range(len(ids)):
        lo = int(corpus.row_off[utt[b]]) + int(shift[b])
        np.testing.assert_array_equal(corpus.X.numpy()[lo:lo + pn[b]], Xr[b, :pn[b]])


def test_prefetcher_hands_the_lengths_through_on_the_host():
    n = np.array([4, 2, 1], dtype=np.int32)
    batches = [(np.ones((3, 4, 2), dtype=np.float32) * i, np.zeros((3, 4, 1)), n + 0) for i in range(3)]
    pf = data.BatchPrefetcher(lambda i: batches[i], 3, host_items=(2,))
    try:
        got = list(pf)
    finally:
        pf.close()
    assert len(got) == 3
    for i, (X, Y, k) in enumerate(got):
        assert isinstance(k, np.ndarray) and k.dtype == np.int32 and k.tolist() == [4, 2, 1]
        assert tuple(X.shape) == (3, 4, 2) and float(X[0, 0, 0]) == float(i)
    # not named, an integer array becomes a float32 tensor as ever
    pf = data.BatchPrefetcher(lambda i: batches[i], 1)
    try:
        (X, Y, k), = list(pf)
    finally:
        pf.close()
    assert torch.is_tensor(k) and k.dtype == torch.float32 and k.tolist() == [4.0, 2.0, 1.0]
