"""Duration side of the label front end: ptts_labels_segments (csrc/labels.hip, ops.labels_segments) and, in
percivaltts_amd/external/merlin/label_normalisation.py, the duration targets (prepare_dur_data / extract_dur_features), the
phone-level inputs (HTSDurationLabelNormalisation) and the context rows built from durations (extract_durational_features, the
duration files of extract_linguistic_features / perform_normalisation, normalise_with_durations).

What is pinned against the REAL reference: tests/golden/durations/*.npz are what the reference's own extract_dur_features and
HTSDurationLabelNormalisation gave for two of the committed label files (tests/golden/durations/make_durations_golden.py).  What
has no reference run (the reference's duration-file paths stop with a TypeError under numpy 2) takes the round-trip definition:
durations extracted from an aligned file, fed back with labels that carry no times, give that file's own context rows, bit for
bit -- and those rows are pinned against the reference by tests/test_labels.py.  The segment kernel itself is checked against a
numpy restatement written here, with exact integer equality.
"""
import ctypes
import functools
import os
import re

import numpy as np
import pytest

from percivaltts_amd import _hip, compose, ops
from percivaltts_amd.external.merlin import label_normalisation as ln

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = os.path.join(ROOT, 'tests', 'golden', 'labels')
GD = os.path.join(ROOT, 'tests', 'golden', 'durations')
FIDS = ['arctic_a0005', 'arctic_a0008']                 # the two utterances of the fixtures
PHONES = {'arctic_a0005': 17, 'arctic_a0008': 24, 'arctic_a0002': 42}
FRAMES = {'arctic_a0005': 293, 'arctic_a0008': 453, 'arctic_a0002': 747}
QFILES = {'radio416': os.path.join(G, 'questions-radio_dnn_416.hed'), 'handwritten': os.path.join(G, 'questions-handwritten.hed')}
COMBINATIONS = [('state_align', 'numerical', 'state', 'phoneme'), ('state_align', 'numerical', 'phoneme', 'phoneme'),
                ('state_align', 'binary', 'state', 'frame'), ('state_align', 'binary', 'phoneme', 'frame'),
                ('phone_align', 'numerical', 'phoneme', 'phoneme'), ('phone_align', 'binary', 'phoneme', 'frame')]


def lab(fid, align='state_align'):
    return os.path.join(G, 'label_' + align, fid + '.lab')


@functools.lru_cache(maxsize=None)
def golden(name):
    with np.load(os.path.join(GD, name + '.npz')) as z:
        out = {k: z[k] for k in z.files}
    for a in out.values(): a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def normaliser(qname, feats='full'):
    return ln.HTSLabelNormalisation(QFILES[qname], add_frame_features=True, subphone_feats=feats)


def bare_labels(fid, directory, align='phone_align'):
    """The labels of a fixture file without their times, one per line."""
    path = os.path.join(str(directory), '{}_{}_bare.lab'.format(fid, align))
    with open(lab(fid, align)) as f, open(path, 'w') as g:
        g.writelines(line.split()[-1] + '\n' for line in f if line.strip())
    return path


# ---------------------------------------------------------------------------------------------------------------------------
# CPU: the host side
# ---------------------------------------------------------------------------------------------------------------------------
def test_duration_targets_equal_the_reference(tmp_path):
    """extract_dur_features is host work (a few integers per label line): the six combinations against the reference's output."""
    n, want = normaliser('handwritten'), golden('dur_features')
    assert len(want) == len(FIDS) * len(COMBINATIONS)
    for fid in FIDS:
        for align, ft, us, fs in COMBINATIONS:
            got = n.extract_dur_features(lab(fid, align), None, align, ft, us, fs)
            w = want['{}/{}/{}_{}_{}'.format(fid, align, ft, us, fs)]
            assert got.dtype == np.float32 and got.shape == w.shape and np.array_equal(got, w), (fid, align, ft, us, fs)
    a5 = want['arctic_a0005/state_align/numerical_state_phoneme']
    assert a5.shape == (17, 5) and a5.sum() == 293 and a5[0].tolist() == [1, 1, 25, 3, 8]
    assert want['arctic_a0005/state_align/binary_state_frame'].sum() == 85 and want['arctic_a0005/phone_align/binary_phoneme_frame'].sum() == 17
    # the defaults: numerical state durations per phone; phone_align means unit_size 'phoneme'; binary means one row per frame
    assert np.array_equal(n.extract_dur_features(lab(FIDS[0])), a5)
    assert np.array_equal(n.extract_dur_features(lab(FIDS[0], 'phone_align'), label_type='phone_align'), a5.sum(axis=1, keepdims=True))
    assert np.array_equal(n.extract_dur_features(lab(FIDS[0]), feature_type='binary'), want['arctic_a0005/state_align/binary_state_frame'])
    # prepare_dur_data writes headerless float32 and turns unit_size into 'phoneme' for phone-aligned labels
    outs = [str(tmp_path / (fid + '.dur')) for fid in FIDS]
    n.prepare_dur_data([lab(fid) for fid in FIDS], outs)
    for fid, o in zip(FIDS, outs):
        assert np.array_equal(np.fromfile(o, dtype=np.float32).reshape(-1, 5), want[fid + '/state_align/numerical_state_phoneme'])
    n.prepare_dur_data([lab(fid, 'phone_align') for fid in FIDS], outs, label_type='phone_align', unit_size='state')
    for fid, o in zip(FIDS, outs):
        assert np.array_equal(np.fromfile(o, dtype=np.float32).reshape(-1, 1), want[fid + '/phone_align/numerical_phoneme_phoneme'])


def test_duration_refusals(tmp_path):
    n = normaliser('handwritten')
    for align, combo in (('state_align', ('numerical', 'state', 'frame')), ('state_align', ('numerical', 'syllable', 'syllable')),
                         ('state_align', ('numerical', 'word', 'word')), ('state_align', ('numerical', 'phoneme', 'MLU')),
                         ('state_align', ('binary', 'state', 'phoneme')), ('state_align', ('ternary', 'state', 'frame')),
                         ('phone_align', ('numerical', 'state', 'phoneme')), ('phone_align', ('binary', 'state', 'frame')),
                         ('phone_align', ('numerical', 'phoneme', 'frame'))):
        with pytest.raises(ValueError, match=re.escape(str(combo))):
            n.extract_dur_features(lab(FIDS[0], align), None, align, *combo)
    with pytest.raises(ValueError):
        n.extract_dur_features(lab(FIDS[0]), label_type='word_align')
    with pytest.raises(ValueError):
        n.prepare_dur_data([lab(FIDS[0])], [])
    with pytest.raises(ValueError):
        n.prepare_dur_data([lab(FIDS[0])], [str(tmp_path / 'x.dur')], feature_type='ternary')
    p = tmp_path / 'zero.lab'                       # the state [4] has no frame: 'binary' has no last frame to mark
    times = [(0, 50000), (50000, 100000), (100000, 100000), (100000, 150000), (150000, 200000)]
    p.write_text(''.join('{} {} x^x-sil+w=ih[{}]\n'.format(a, b, k + 2) for k, (a, b) in enumerate(times)))
    assert n.extract_dur_features(str(p)).tolist() == [[1, 1, 0, 1, 1]]
    with pytest.raises(ValueError):
        n.extract_dur_features(str(p), feature_type='binary')
    p = tmp_path / 'order.lab'                      # five lines, but not [2] .. [6]
    p.write_text(''.join('{} {} x^x-sil+w=ih[{}]\n'.format(50000 * k, 50000 * (k + 1), (2, 3, 3, 5, 6)[k]) for k in range(5)))
    with pytest.raises(ValueError):
        n.extract_dur_features(str(p))
    # context rows from durations: refusals that need no device
    with pytest.raises(ValueError):
        normaliser('handwritten', 'minimal_frame').extract_durational_features(dur_data=np.ones((3, 5), np.float32))
    with pytest.raises(ValueError):
        n.extract_durational_features()
    with pytest.raises(ValueError):
        n.extract_durational_features(dur_data=np.ones((3, 1), np.float32))         # 'full' takes [P,5]
    with pytest.raises(ValueError):
        normaliser('handwritten', 'coarse_coding').extract_durational_features(dur_data=np.ones((3, 5), np.float32))
    d = tmp_path / 'a.dur'
    np.ones((16, 5), np.float32).tofile(str(d))     # 16 phones of durations, 17 in the label file
    with pytest.raises(ValueError, match='17'):
        n.extract_linguistic_features(lab(FIDS[0]), dur_file_name=str(d))
    np.ones(7, np.float32).tofile(str(d))
    with pytest.raises(ValueError):
        n.extract_linguistic_features(lab(FIDS[0]), dur_file_name=str(d))
    with pytest.raises(ValueError):                 # as with times: 'full' needs states
        n.extract_linguistic_features(lab(FIDS[0], 'phone_align'), label_type='phone_align', dur_file_name=str(d))
    with pytest.raises(ValueError):
        n.perform_normalisation([lab(FIDS[0])], [str(tmp_path / 'o')], dur_file_list=[])
    dn = ln.HTSDurationLabelNormalisation(QFILES['handwritten'])
    assert (dn.dimension, dn.dict_size, dn.frame_feature_size) == (37, 37, 9)
    with pytest.raises(ValueError):
        dn.extract_linguistic_features(lab(FIDS[0]), dur_file_name=str(d))
    with pytest.raises(ValueError):
        dn.extract_durational_features(dur_data=np.ones((3, 5), np.float32))
    with pytest.raises(ValueError):
        dn.extract_linguistic_features(lab(FIDS[0]), label_type='word_align')


def test_phone_labels_without_times(tmp_path):
    want = ln.parse_label_file(lab(FIDS[0]), 'state_align')[0]
    assert len(want) == 17
    assert ln.parse_phone_labels(lab(FIDS[0]), 'state_align') == want                           # the [2] line of each five, suffix stripped
    assert ln.parse_phone_labels(lab(FIDS[0], 'phone_align'), 'phone_align') == want
    assert ln.parse_phone_labels(bare_labels(FIDS[0], tmp_path), 'phone_align') == want         # no times at all
    assert ln.parse_phone_labels(bare_labels(FIDS[0], tmp_path), 'state_align') == want         # bare labels count as phones
    states = ln.parse_phone_labels(bare_labels(FIDS[0], tmp_path, 'state_align'), 'state_align')
    assert states == want
    assert len(ln.parse_phone_labels(lab(FIDS[0]), 'phone_align')) == 85 and ln.parse_phone_labels(lab(FIDS[0]), 'phone_align')[0].endswith(b'[2]')
    with pytest.raises(ValueError):
        ln.parse_phone_labels(lab(FIDS[0]), 'word_align')


def test_no_device_no_fallback(monkeypatch, tmp_path):
    import torch
    monkeypatch.setattr(torch.cuda, 'is_available', lambda: False)
    d = tmp_path / 'a.dur'
    normaliser('handwritten').prepare_dur_data([lab(FIDS[0])], [str(d)])                    # host work: no device needed
    with pytest.raises(_hip.HipLibraryError):
        normaliser('handwritten').extract_linguistic_features(lab(FIDS[0]), dur_file_name=str(d))
    with pytest.raises(_hip.HipLibraryError):
        normaliser('handwritten').extract_durational_features(dur_file_name=str(d))
    with pytest.raises(_hip.HipLibraryError):
        ln.HTSDurationLabelNormalisation(QFILES['handwritten']).extract_linguistic_features(lab(FIDS[0]))
    with pytest.raises(_hip.HipLibraryError):
        normaliser('handwritten').normalise_with_durations([lab(FIDS[0])], torch.ones(17, 5))
    with pytest.raises(_hip.HipLibraryError):
        ops.labels_segments(torch.ones(3, 5), torch.tensor([0, 3], dtype=torch.int32), 1, 100)


def test_segments_entry_point_rejects_bad_arguments():
    """The library loads without a device; PTTS_EINVAL before any launch, the message naming the entry point."""
    assert 'ptts_labels_segments' in _hip.SIGNATURES
    lib = _hip.lib()
    p = ctypes.c_void_p(256)

    def segments(dur=p, off=p, P=10, D=5, U=2, lo=1, hi=1000, seg=p, rows=p, status=p):
        return lib.ptts_labels_segments(dur, off, P, D, U, lo, hi, seg, rows, status, None)
    for kw in (dict(dur=None), dict(off=None), dict(seg=None), dict(rows=None), dict(status=None), dict(P=-1), dict(D=0), dict(D=2), dict(D=4),
               dict(D=6), dict(U=0), dict(U=-1), dict(lo=-1), dict(lo=1001), dict(hi=ops.LABELS_SEG_MAX_FRAMES + 1),
               dict(P=1 << 20, hi=1 << 12), dict(P=1 << 30, D=1, hi=2), dict(seg=ctypes.c_void_p(264))):
        assert segments(**kw) == -1, kw
        assert 'labels_segments' in _hip.last_error(), kw
    assert '2^31' in (segments(P=1 << 20, hi=1 << 12), _hip.last_error())[1]
    with open(os.path.join(ROOT, 'include', 'percival_hip.h')) as f:
        header = f.read()
    assert '#define PTTS_LABELS_SEG_STATES      {}\n'.format(ops.LABELS_SEG_STATES) in header
    assert '#define PTTS_LABELS_SEG_CLAMPED     {}\n'.format(ops.LABELS_SEG_CLAMPED) in header
    assert '#define PTTS_LABELS_SEG_MAX_FRAMES  {}\n'.format(ops.LABELS_SEG_MAX_FRAMES) in header


# ---------------------------------------------------------------------------------------------------------------------------
# GPU: the segment kernel against a numpy restatement
# ---------------------------------------------------------------------------------------------------------------------------
def segments_in_numpy(dur, unit_off, lo, hi):
    """The rule of include/percival_hip.h in numpy and Python loops (a restatement): seg [P*D,8], rows [U+1], status [U]."""
    P, D = dur.shape
    with np.errstate(invalid='ignore'):
        r = np.rint(dur.astype(np.float32))             # ties to even
        over = r > hi
        n = np.where(np.isnan(r) | (r < lo), lo, np.where(over, hi, r)).astype(np.int64)
    U = len(unit_off) - 1
    seg, rows, status = np.zeros((P * D, 8), np.int64), np.zeros(U + 1, np.int64), np.zeros(U, np.int64)
    row = 0
    for u in range(U):
        rows[u] = row
        for p in range(unit_off[u], unit_off[u + 1]):
            base = 0
            for k in range(D):
                seg[p * D + k] = [p, row, n[p, k], k + 1 if D > 1 else 0, D - k if D > 1 else 0, n[p].sum(), base, 0]
                row += n[p, k]
                base += n[p, k]
            status[u] |= int(over[p].any())
    rows[U] = row
    return seg.astype(np.int32), rows.astype(np.int32), status.astype(np.int32)


def device_segments(dur, unit_off, lo, hi):
    import torch
    dev = compose._device()
    seg, rows, status = ops.labels_segments(torch.from_numpy(np.array(dur, dtype=np.float32)).to(dev),
                                            torch.from_numpy(np.asarray(unit_off, dtype=np.int32)).to(dev), lo, hi)
    assert seg.dtype == rows.dtype == status.dtype == torch.int32
    return seg.cpu().numpy(), rows.cpu().numpy(), status.cpu().numpy()


SPECIAL = [0.49, 0.5, 1.5, 2.5, -3.0, float('nan'), 0.0, 3.5, 0.51, float('inf'), float('-inf'), 49.5, 50.49]
MAX_FRAMES = 50


@functools.lru_cache(maxsize=None)
def segment_durations(D):
    """Utterances of 1, 7 and 300 phones (300 x 5 values cross the scan tile of 1024); the special values sit in the second
    utterance and at both sides of the tile boundary of the third, which also holds the one value above MAX_FRAMES."""
    rng = np.random.RandomState(11 + D)
    dur = rng.uniform(0.0, 12.0, size=(308, D)).astype(np.float32)
    flat = dur.reshape(-1)
    flat[1 * D:1 * D + len(SPECIAL)] = SPECIAL
    if D == 5:
        flat[8 * D + 1018:8 * D + 1018 + len(SPECIAL)] = SPECIAL[::-1]
    flat[(8 + 150) * D] = 50.51                     # rounds to 51 > MAX_FRAMES
    dur.setflags(write=False)
    return dur


@pytest.mark.gpu
@pytest.mark.parametrize('min_frames', [0, 1])
@pytest.mark.parametrize('D', [5, 1])
def test_segments_equal_the_numpy_restatement(D, min_frames):
    dur, off = segment_durations(D), [0, 1, 8, 308]
    want = segments_in_numpy(dur, off, min_frames, MAX_FRAMES)
    got = device_segments(dur, off, min_frames, MAX_FRAMES)
    for g, w, name in zip(got, want, ('seg', 'rows', 'status')):
        assert g.shape == w.shape and np.array_equal(g, w), (name, np.argwhere(g != w)[:5].tolist())
    seg, rows, status = got
    # 50.51 sits in the third utterance; the special values (inf among them) fill phones 1-3 with D = 5 and phones 1-13 with D = 1
    assert status.tolist() == [0, ops.LABELS_SEG_CLAMPED if D == 5 else 0, ops.LABELS_SEG_CLAMPED]
    assert rows[-1] == seg[:, 2].sum() and (np.diff(seg[:, 1]) == seg[:-1, 2]).all() and (seg[:, 2] >= min_frames).all()
    assert seg[:, 2].max() == MAX_FRAMES
    # the rounding itself, spelled out: ties to even, NaN and negatives to min_frames
    k = 1 * D
    assert seg[k:k + 9, 2].tolist() == [max(v, min_frames) for v in (0, 0, 2, 2, 0, 0, 0, 4, 1)]
    assert seg[k + 9:k + 13, 2].tolist() == [50, min_frames, 50, 50]
    # a lone utterance (U = 1) gives the rows of that utterance in the batch, from row 0
    one = device_segments(dur[8:], [0, 300], min_frames, MAX_FRAMES)
    w1 = segments_in_numpy(dur[8:], [0, 300], min_frames, MAX_FRAMES)
    assert all(np.array_equal(g, w) for g, w in zip(one, w1))
    assert np.array_equal(one[0][:, 2:], seg[8 * D:, 2:]) and one[1].tolist() == [0, rows[3] - rows[2]]


@pytest.mark.gpu
def test_segments_without_phones_and_many_utterances():
    seg, rows, status = device_segments(np.zeros((0, 5), np.float32), [0, 0, 0], 1, 100)
    assert seg.shape == (0, 8) and rows.tolist() == [0, 0, 0] and status.tolist() == [0, 0]
    # more utterances than one scan tile of the offsets (1024), some of them empty
    rng = np.random.RandomState(5)
    counts = rng.randint(0, 4, size=1500)
    off = np.concatenate([[0], np.cumsum(counts)])
    dur = rng.uniform(0, 6, size=(int(off[-1]), 1)).astype(np.float32)
    got, want = device_segments(dur, off, 1, 100), segments_in_numpy(dur, off, 1, 100)
    assert all(np.array_equal(g, w) for g, w in zip(got, want))
    import torch
    with pytest.raises(ValueError):
        ops.labels_segments(torch.ones(3, 4, device='cuda'), torch.tensor([0, 3], dtype=torch.int32, device='cuda'), 1, 100)
    with pytest.raises(ValueError):
        ops.labels_segments(torch.ones(3, 5, device='cuda'), torch.tensor([0, 3], dtype=torch.int32, device='cuda'), 2, 1)
    with pytest.raises(ValueError):
        ops.labels_segments(torch.ones(1 << 20, 5, device='cuda'), torch.tensor([0, 1 << 20], dtype=torch.int32, device='cuda'), 1, 1 << 12)


# ---------------------------------------------------------------------------------------------------------------------------
# GPU: the normaliser
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize('qname', ['handwritten', 'radio416'])
def test_duration_inputs_equal_the_reference(qname, tmp_path):
    """One row per line, the question columns alone, on state-aligned, phone-aligned and timing-less files; ptts_labels_match
    and nothing else."""
    dn = ln.HTSDurationLabelNormalisation(QFILES[qname])
    want = golden(qname + '_duration_inputs')
    for fid in FIDS:
        files = {'state_align': lab(fid), 'phone_align': lab(fid, 'phone_align'), 'bare': bare_labels(fid, tmp_path)}
        for key, path in files.items():
            with _hip.KernelTimer() as kt:
                got = dn.extract_linguistic_features(path)
            assert [r[0] for r in kt.records] == ['ptts_labels_match']
            w = want['{}/{}'.format(fid, key)]
            assert got.dtype == np.float32 and got.shape == w.shape == (PHONES[fid] * (5 if key == 'state_align' else 1), dn.dict_size)
            assert np.array_equal(got, w), (fid, key)
    outs = [str(tmp_path / (fid + '.bin')) for fid in FIDS]
    dn.perform_normalisation([lab(fid, 'phone_align') for fid in FIDS], outs)
    for fid, o in zip(FIDS, outs):
        assert open(o, 'rb').read() == want[fid + '/phone_align'].tobytes()


@pytest.mark.gpu
@pytest.mark.parametrize('feats,align', [('full', 'state_align'), ('minimal_frame', 'state_align'), ('state_only', 'state_align'),
                                         ('none', 'state_align'), ('minimal_phoneme', 'phone_align'), ('coarse_coding', 'phone_align'),
                                         ('none', 'phone_align')])
def test_round_trip_through_durations(feats, align, tmp_path):
    """Durations extracted from an aligned file, fed back with labels that carry no times, give that file's own rows."""
    n = normaliser('handwritten', feats)
    for fid in FIDS:
        want = n.extract_linguistic_features(lab(fid, align), label_type=align)
        dur = str(tmp_path / (fid + '.dur'))
        n.prepare_dur_data([lab(fid, align)], [dur], label_type=align)
        got = n.extract_linguistic_features(bare_labels(fid, tmp_path), label_type=align, dur_file_name=dur)
        assert got.dtype == np.float32 and got.shape == want.shape == (FRAMES[fid], n.dimension)
        assert np.array_equal(got, want), (fid, np.argwhere(got != want)[:3].tolist())
        # the aligned file itself may stand in for the timing-less one: its times are ignored
        assert np.array_equal(n.extract_linguistic_features(lab(fid, align), label_type=align, dur_file_name=dur), want)
        if feats in ('full', 'coarse_coding'):
            F = n.frame_feature_size
            sub = n.extract_durational_features(dur_file_name=dur)
            assert sub.dtype == np.float32 and sub.shape == (FRAMES[fid], F) and np.array_equal(sub, want[:, -F:])
            assert np.array_equal(n.extract_durational_features(dur_data=np.fromfile(dur, dtype=np.float32).reshape(-1, 5 if feats == 'full' else 1)), sub)
    outs = [str(tmp_path / (fid + '.bin')) for fid in FIDS]
    n.perform_normalisation([bare_labels(fid, tmp_path) for fid in FIDS], outs, label_type=align,
                            dur_file_list=[str(tmp_path / (fid + '.dur')) for fid in FIDS])
    for fid, o in zip(FIDS, outs):
        assert open(o, 'rb').read() == n.extract_linguistic_features(lab(fid, align), label_type=align).tobytes()


@pytest.mark.gpu
def test_device_batch_equals_file_by_file(tmp_path):
    """normalise_with_durations on three utterances: the rows of each, cut at the offsets, are the file-by-file rows; fractional
    durations are rounded by the kernel's rule and lifted to min_frames."""
    import torch
    n = normaliser('radio416')
    fids = ['arctic_a0005', 'arctic_a0002', 'arctic_a0008']
    rng = np.random.RandomState(2)
    durs = [(n.extract_dur_features(lab(fid)) + rng.uniform(-0.6, 0.6, size=(PHONES[fid], 5))).astype(np.float32) for fid in fids]
    durs[1][3] = [0.5, 1.5, 2.5, -1.0, float('nan')]
    labels = [bare_labels(fid, tmp_path) for fid in fids]
    dev = compose._device()
    with _hip.KernelTimer() as kt:
        X, offs = n.normalise_with_durations(labels, torch.from_numpy(np.concatenate(durs)).to(dev), 'state_align', min_frames=1)
    assert [r[0] for r in kt.records] == ['ptts_labels_segments', 'ptts_labels_match', 'ptts_labels_expand']
    assert X.is_cuda and X.dtype == torch.float32 and offs.shape == (4,) and offs[0] == 0 and X.shape == (offs[-1], 425)
    X = X.cpu().numpy()
    for i, fid in enumerate(fids):
        rounded = np.maximum(np.nan_to_num(np.rint(durs[i]), nan=1.0), 1.0).astype(np.float32)
        assert offs[i + 1] - offs[i] == rounded.sum()
        path = str(tmp_path / (fid + '.dur'))
        rounded.tofile(path)
        want = n.extract_linguistic_features(labels[i], dur_file_name=path)
        assert np.array_equal(X[offs[i]:offs[i + 1]], want), fid
    # a list of tensors, one per file, is the same call
    X2, offs2 = n.normalise_with_durations(labels, [torch.from_numpy(d).to(dev) for d in durs], 'state_align', min_frames=1)
    assert np.array_equal(offs2, offs) and np.array_equal(X2.cpu().numpy(), X)
    with pytest.raises(ValueError):
        n.normalise_with_durations(labels, torch.ones(5, 5, device=dev))
    with pytest.raises(ValueError, match='above'):
        n.normalise_with_durations(labels[:1], torch.full((17, 5), 1e6, device=dev))
