"""Label front end: csrc/labels.hip (ops.labels_match / ops.labels_expand), percivaltts_amd/external/merlin/label_normalisation.py
and run.contexts_extraction.

Parity is pinned against the REAL reference here, not a restatement: tests/golden/labels/*.npz are what the reference's own
HTSLabelNormalisation wrote for the committed label files (tests/golden/labels/make_labels_golden.py; five of the reference's ten
test utterances, its shipped question set and a hand-written one that exercises what the shipped set does not).  The comparisons
are np.array_equal: the QS columns are 0/1, the CQS columns small integers, and the frame features ratios of small integers
divided in fp64 and rounded once to fp32, as the reference's fp64 matrix is by numpy.array(data, 'float32').

Two things are NOT reference runs and are named so below: the `re` evaluation of the question semantics written in this file
(test_match_equals_re_*), and 'coarse_coding', whose table the reference computes with matplotlib's removed mlab.normpdf -- its
three coded columns are checked against the formula restated in numpy (test_coarse_coding_*).
"""
import ctypes
import functools
import math
import os
import re

import numpy as np
import pytest

from percivaltts_amd import _hip, compose, data, ops
from percivaltts_amd.external.merlin import label_normalisation as ln

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = os.path.join(ROOT, 'tests', 'golden', 'labels')
FIDS = ['arctic_a0002', 'arctic_a0004', 'arctic_a0005', 'arctic_a0006', 'arctic_a0008']
FRAMES = {'arctic_a0002': 747, 'arctic_a0004': 497, 'arctic_a0005': 293, 'arctic_a0006': 589, 'arctic_a0008': 453}
QFILES = {'radio416': os.path.join(G, 'questions-radio_dnn_416.hed'), 'handwritten': os.path.join(G, 'questions-handwritten.hed')}


def lab(fid, align='state_align'):
    return os.path.join(G, 'label_' + align, fid + '.lab')


@functools.lru_cache(maxsize=None)
def golden(qname, feats, align):
    with np.load(os.path.join(G, '{}_{}_{}.npz'.format(qname, feats, align))) as z:
        out = {fid: z[fid] for fid in FIDS}
    for a in out.values(): a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def normaliser(qname, feats='full'):
    return ln.HTSLabelNormalisation(QFILES[qname], add_frame_features=True, subphone_feats=feats)


@functools.lru_cache(maxsize=None)
def fixture_phone_labels():
    out = []
    for fid in FIDS:
        with open(lab(fid, 'phone_align')) as f:
            out.extend(line.split()[2] for line in f if line.strip())
    return tuple(out)


# ---------------------------------------------------------------------------------------------------------------------------
# CPU: the host side
# ---------------------------------------------------------------------------------------------------------------------------
def test_shipped_question_set_counts():
    n = normaliser('radio416')
    assert (n.questions.n_qs, n.questions.n_cqs) == (373, 43)
    assert sum(len(pats) for _, pats in n.questions.qs) == 916
    assert (n.dict_size, n.frame_feature_size, n.dimension) == (416, 9, 425)
    assert not any(p.wild for p in n.questions.patterns)                # no '?' or inner '*' in the shipped set
    t = n.questions.host_table()
    assert t['qs_first'][0] == 0 and t['qs_first'][-1] == 916 and (np.diff(t['qs_first']) >= 1).all()
    assert t['pat_bytes'].nbytes + 8 * len(t['pat_off']) < 48 << 10     # it is staged in the LDS
    for feats, size in (('minimal_frame', 2), ('state_only', 1), ('none', 0), ('minimal_phoneme', 3), ('coarse_coding', 4)):
        m = normaliser('radio416', feats)
        assert (m.frame_feature_size, m.dimension) == (size, 416 + size)


def test_anchor_flags_of_the_hand_written_set():
    qs = {key.split('\t')[0].strip('"'): pats for key, pats in normaliser('handwritten').questions.qs}
    flags = lambda p: (p.text, p.anchor_start, p.anchor_end, p.wild)
    assert flags(qs['C-Vowel_plain'][0]) == ('-aa+', False, False, False)           # no '*': plain substring search
    assert flags(qs['C-Sil_star'][0]) == ('-sil+', False, False, False)             # '*' at both ends
    assert flags(qs['Start_x'][0]) == ('x^', True, False, False)                    # does not begin with '*'
    assert flags(qs['End_1'][0]) == ('-1', False, True, False)                      # does not end with '*'
    assert flags(qs['Inner_star'][0]) == ('^sil-*=l@', False, False, True)          # inner '*'
    assert flags(qs['Inner_both_anchors'][0]) == ('x^*-1', True, True, True)
    assert flags(qs['Qmark_one'][0]) == ('-?+', False, False, True)
    assert flags(qs['Qmark_plain'][0]) == ('/A:?_0_', False, False, True)           # '?' alone does not anchor
    assert flags(qs['Double_star'][0]) == ('-ih+', False, False, False)             # every outer '*' is stripped
    assert flags(qs['All'][0]) == ('', False, False, False)
    assert flags(qs['LL-x'][0]) == ('x^', True, False, False)                       # an LL- key anchors at the start
    assert flags(qs['LL-consonant'][-1]) == ('z^', True, True, False)
    # the reference tests the line's second space-separated token: behind tabs it runs on into the patterns
    assert [flags(p) for p in qs['Tabbed_key']] == [('LL-', True, False, False), ('x^x-sil', True, False, False)]
    assert [flags(p) for p in qs['Spaced_key']] == [('LL-', False, False, False), ('x^x-sil', False, False, False)]
    cqs = {key.split('\t')[0].strip('"'): (pre, suf, kind) for key, pre, suf, kind in normaliser('handwritten').questions.cqs}
    pre, suf, kind = cqs['Seg_Fw']
    assert (flags(pre), flags(suf), kind) == (('@', False, False, False), ('_', False, False, False), ops.LABELS_CAPTURE_DIGITS)
    pre, suf, kind = cqs['Last_number']
    assert (flags(pre), flags(suf), kind) == (('-', False, False, False), ('', False, True, False), ops.LABELS_CAPTURE_DIGITS)
    pre, suf, kind = cqs['First_number']
    assert (flags(pre), flags(suf)) == (('', True, False, False), ('^', False, False, False))
    pre, suf, kind = cqs['Decimal_end']
    assert (flags(pre), flags(suf), kind) == (('+', False, False, False), ('-1', False, True, False), ops.LABELS_CAPTURE_DECIMAL)
    assert flags(cqs['Qmark_prefix'][0]) == ('/?:', False, False, True)
    meta = normaliser('handwritten').questions.host_table()['pat_meta']
    pats = normaliser('handwritten').questions.patterns
    for m, p in zip(meta, pats):
        assert m & 0xffff == len(p.text)
        assert (bool(m & ops.LABELS_ANCHOR_START), bool(m & ops.LABELS_ANCHOR_END), bool(m & ops.LABELS_WILD)) == (p.anchor_start, p.anchor_end, p.wild)


def test_label_parsing_of_a0005():
    phones, segs = ln.parse_label_file(lab('arctic_a0005'), 'state_align')
    assert segs.shape == (85, 7) and len(phones) == 17
    assert segs[:, 2].sum() == 293
    assert phones[0] == b'x^x-sil+w=ih@x_x/A:0_0_0/B:x-x-x@x-x&x-x#x-x$x-x!x-x;x-x|x/C:1+1+3/D:0_0/E:x+x@x+x&x+x#x+x/F:md_1/G:0_0/H:x=x@1=1|0/I:7=5/J:7+5-1'
    assert segs[:5].tolist() == [[0, 0, 1, 1, 5, 38, 0], [0, 1, 1, 2, 4, 38, 1], [0, 2, 25, 3, 3, 38, 2], [0, 27, 3, 4, 2, 38, 27],
                                 [0, 30, 8, 5, 1, 38, 30]]
    assert (np.diff(segs[:, 1]) == segs[:-1, 2]).all()                              # first rows are the running frame count
    for p in range(17):                                                             # a phone's duration is its five states'
        assert segs[segs[:, 0] == p][:, 2].sum() == segs[segs[:, 0] == p][0, 5]
    pphones, psegs = ln.parse_label_file(lab('arctic_a0005', 'phone_align'), 'phone_align')
    assert list(pphones) == list(phones) and psegs[:, 2].sum() == 293
    assert psegs[0].tolist() == [0, 0, 38, 0, 0, 38, 0]


def test_refusals(tmp_path):
    for feats in ('frame_only', 'uniform_state', 'nonsense'):
        with pytest.raises(ValueError):
            ln.HTSLabelNormalisation(QFILES['handwritten'], subphone_feats=feats)
    with pytest.raises(ValueError):
        ln.HTSLabelNormalisation(QFILES['handwritten'], add_frame_features=False)

    def qfile(text):
        p = tmp_path / 'q.hed'
        p.write_text(text)
        return str(p)
    for text in ('CQS "star_in_prefix" {/A:*_(\\d+)_}\n', 'CQS "star_in_suffix" {_(\\d+)_*/B:x}\n', 'CQS "two" {@(\\d+)_,_(\\d+)/}\n',
                 'CQS "no_capture" {/A:0_}\n', 'CQS "two_captures" {@(\\d+)_(\\d+)}\n', 'XS "what" {*-a+*}\n', 'QS\t"tab_only"\t{*-a+*}\n',
                 'QS "no braces" *-a+*\n', 'QS "non-ascii" {*-é+*}\n', 'ab\n\n'):
        with pytest.raises(ValueError):
            ln.HTSLabelNormalisation(qfile(text))
    assert ln.HTSLabelNormalisation(qfile('QS "a" {*-a+*}\nab{}\n')).dimension == 10       # lines of <= 5 characters are skipped

    n = normaliser('handwritten')
    def labfile(text):
        p = tmp_path / 'x.lab'
        p.write_text(text)
        return str(p)
    five = lambda label: ''.join('{} {} {}[{}]\n'.format(50000 * k, 50000 * (k + 1), label, k + 2) for k in range(5))
    for text in ('x^x-sil+w=ih[2]\n',                                       # no times
                 five('x^x-sil+w')[:-20],                                   # the phone has four state lines
                 five('x^x-sil+w').replace('[2]', '[3]'),                   # does not begin with the first state
                 '100000 50000 x^x-sil+w[2]\n',                             # ends before it starts
                 'a b x^x-sil+w[2]\n',
                 five('x' * 1025)):                                         # longer than the kernel stages
        with pytest.raises(ValueError):
            n.extract_linguistic_features(labfile(text))
    with pytest.raises(ValueError):
        n.extract_linguistic_features(lab('arctic_a0005'), label_type='word_align')
    with pytest.raises(ValueError):                                         # as the reference: 'full' needs states
        n.extract_linguistic_features(lab('arctic_a0005', 'phone_align'), label_type='phone_align')
    with pytest.raises(ValueError):
        normaliser('handwritten', 'minimal_phoneme').extract_linguistic_features(lab('arctic_a0005'))
    with pytest.raises(ValueError):
        n.perform_normalisation([lab('arctic_a0005')], [])


def test_no_device_no_fallback(monkeypatch, tmp_path):
    import torch
    monkeypatch.setattr(torch.cuda, 'is_available', lambda: False)
    with pytest.raises(_hip.HipLibraryError):
        normaliser('handwritten').extract_linguistic_features(lab('arctic_a0005'))
    with pytest.raises(_hip.HipLibraryError):
        ops.labels_expand(torch.zeros(2, 3), torch.zeros(1, 8, dtype=torch.int32), 4, 'full')


def test_header_library_and_documents():
    with open(os.path.join(ROOT, 'include', 'percival_hip.h')) as f:
        header = f.read()
    names = ['ptts_labels_match', 'ptts_labels_expand', 'ptts_labels_feature_count']
    assert os.path.exists(_hip.LIB_PATH), 'libpercival_hip.so not built (run __graft_entry__.build())'
    lib = _hip.lib()
    for n in names:
        assert re.search(r'\bint {}\('.format(n), header) and n in _hip.SIGNATURES and hasattr(lib, n), n
    assert '#define PTTS_LABELS_MAX_LABEL       {}'.format(ops.LABELS_MAX_LABEL) in header
    for name, mode in ops.LABELS_MODES.items():
        assert re.search(r'#define PTTS_LABELS_{}\s+{}\n'.format(name.upper(), mode), header)
        assert lib.ptts_labels_feature_count(mode) == ops.LABELS_FEATURES[name]
    assert lib.ptts_labels_feature_count(6) == -1
    for doc in ('INTEGRATION.md', 'DESIGN.md', 'README.md'):
        with open(os.path.join(ROOT, doc)) as f:
            assert 'labels_match' in f.read(), doc
    with open(os.path.join(ROOT, 'percivaltts_amd', 'csrc', 'Makefile')) as f:
        assert 'labels.hip' in f.read()


def test_entry_points_reject_bad_arguments():
    """PTTS_EINVAL before any launch, the message naming the entry point; no pointer is dereferenced."""
    lib = _hip.lib()
    p = ctypes.c_void_p(256)

    def match(labels=p, off=p, P=3, nbytes=100, maxlen=50, pb=p, npb=10, poff=p, pmeta=p, NP=4, qsf=p, nQS=2, cqs=p, nCQS=1, V=p, st=p):
        return lib.ptts_labels_match(labels, off, P, nbytes, maxlen, pb, npb, poff, pmeta, NP, qsf, nQS, cqs, nCQS, V, st, None)
    for kw in (dict(labels=None), dict(off=None), dict(V=None), dict(st=None), dict(P=0), dict(nbytes=-1), dict(maxlen=ops.LABELS_MAX_LABEL + 1),
               dict(maxlen=-1), dict(nQS=0, nCQS=0), dict(nQS=-1), dict(NP=0), dict(poff=None), dict(pmeta=None), dict(pb=None),
               dict(qsf=None), dict(cqs=None)):
        assert match(**kw) == -1, kw
        assert 'labels_match' in _hip.last_error(), kw
    assert 'exceeds the 1024' in (match(maxlen=1025), _hip.last_error())[1]

    def expand(V=p, seg=p, cc=p, X=p, P=3, Q=5, S=4, T=20, mode=0):
        return lib.ptts_labels_expand(V, seg, cc, X, P, Q, S, T, mode, None)
    for kw in (dict(V=None), dict(seg=None), dict(X=None), dict(P=0), dict(Q=0), dict(S=0), dict(T=0), dict(mode=6), dict(mode=-1),
               dict(mode=5, cc=None), dict(X=ctypes.c_void_p(260)), dict(seg=ctypes.c_void_p(264))):
        assert expand(**kw) == -1, kw
        assert 'labels_expand' in _hip.last_error(), kw


# ---------------------------------------------------------------------------------------------------------------------------
# GPU: against the reference's own output
# ---------------------------------------------------------------------------------------------------------------------------
def assert_equals_golden(qname, feats, align):
    n = normaliser(qname, feats)
    want = golden(qname, feats, align)
    for fid in FIDS:
        got = n.extract_linguistic_features(lab(fid, align), label_type=align)
        assert got.dtype == np.float32 and got.shape == want[fid].shape == (FRAMES[fid], n.dimension), fid
        diff = np.argwhere(got != want[fid])
        assert np.array_equal(got, want[fid]), '{} {} {}: {} elements differ, first at {}'.format(qname, feats, fid, len(diff), diff[:3].tolist())


@pytest.mark.gpu
def test_shipped_set_full_state_alignment_equals_the_reference():
    assert_equals_golden('radio416', 'full', 'state_align')


@pytest.mark.gpu
@pytest.mark.parametrize('feats,align', [('minimal_frame', 'state_align'), ('state_only', 'state_align'), ('none', 'state_align'),
                                         ('minimal_phoneme', 'phone_align'), ('none', 'phone_align')])
def test_shipped_set_other_modes_equal_the_reference(feats, align):
    assert_equals_golden('radio416', feats, align)


@pytest.mark.gpu
@pytest.mark.parametrize('feats,align', [('full', 'state_align'), ('minimal_frame', 'state_align'), ('state_only', 'state_align'),
                                         ('none', 'state_align'), ('minimal_phoneme', 'phone_align'), ('none', 'phone_align')])
def test_hand_written_set_equals_the_reference(feats, align):
    assert_equals_golden('handwritten', feats, align)


# ---- the question semantics in `re`, written here from their description (a restatement, not a reference run) ---------------------
def _piece(text):
    return ''.join('.*' if ch == '*' else '.' if ch == '?' else re.escape(ch) for ch in text)


def re_questions(path):
    """[('QS', [compiled, ...]) | ('CQS', compiled)] of a question file."""
    out = []
    with open(path) as f:
        for line in f.read().split('\n'):
            if len(line) <= 5: continue
            kind, key = line.split(' ')[0], line.split(' ')[1]
            body = line.split('{')[1].split('}')[0].strip()
            def rx(q, ll=False, capture=None):
                start = '\\A' if ll or ('*' in q and not q.startswith('*')) else ''
                end = '\\Z' if '*' in q and not q.endswith('*') else ''
                q = q.strip('*')
                if capture is None: return re.compile(start + _piece(q) + end)
                a, b = q.split(capture)
                return re.compile(start + _piece(a) + ('(\\d+)' if capture == '(\\d+)' else '([\\d.]+)') + _piece(b) + end)
            if kind == 'QS':
                out.append(('QS', [rx(q, ll='LL-' in key) for q in body.split(',')]))
            else:
                out.append(('CQS', rx(body, capture='(\\d+)' if '(\\d+)' in body else '([\\d\\.]+)')))
    return out


def re_evaluate(questions, labels):
    """V [P, Q] float32 with the QS columns first; None in place of a row whose capture float() refuses."""
    ordered = [q for q in questions if q[0] == 'QS'] + [q for q in questions if q[0] == 'CQS']
    rows = []
    for s in labels:
        row = []
        try:
            for kind, c in ordered:
                if kind == 'QS':
                    row.append(1.0 if any(r.search(s) for r in c) else 0.0)
                else:
                    m = c.search(s)
                    row.append(-1.0 if m is None else float(m.group(1)))
        except ValueError:
            row = None
        rows.append(row)
    return rows


def device_match(n, labels):
    import torch
    dev = compose._device()
    enc = [s.encode('ascii') for s in labels]
    off = np.zeros(len(enc) + 1, dtype=np.int32)
    off[1:] = np.cumsum([len(e) for e in enc])
    blob = np.frombuffer(b''.join(enc) or b'\0', dtype=np.uint8).copy()
    V, status = ops.labels_match(torch.from_numpy(blob).to(dev), torch.from_numpy(off).to(dev), max(len(e) for e in enc),
                                 n.questions.device_table(dev))
    return V.cpu().numpy(), status.cpu().numpy()


def random_strings(count, seed=7):
    """Strings over the label alphabet that still hit the questions: real labels with spans cut out, doubled or overwritten, and
    short strings over the characters the questions turn on."""
    rng = np.random.RandomState(seed)
    real = fixture_phone_labels()
    alphabet = sorted(set(''.join(real)) | set('.059'))
    small = list('x^-+=@_/:|&.0159') + ['sil', 'ih', '/A:', '/B:', '/I:', '-1', 'LL-', '+5', '=l@', '5@', '0_']
    out = []
    while len(out) < count:
        if len(out) % 2:
            s = ''.join(small[i] for i in rng.randint(0, len(small), size=rng.randint(0, 24)))
        else:
            s = real[rng.randint(len(real))]
            for _ in range(rng.randint(1, 5)):
                a = rng.randint(0, len(s) + 1); b = min(len(s), a + rng.randint(0, 12)); op = rng.randint(4)
                if op == 0: s = s[:a] + s[b:]
                elif op == 1: s = s[:b] + s[a:b] + s[b:]
                elif op == 2: s = s[:a] + ''.join(alphabet[i] for i in rng.randint(0, len(alphabet), size=b - a)) + s[b:]
                else: s = s[a:] if rng.randint(2) else s[:b]
        out.append(s)
    return out


@pytest.mark.gpu
def test_match_equals_re_on_labels_and_random_strings():
    n = normaliser('handwritten')
    crafted = ['', 'x', '/I:12.5=3', '=0.255@1', '=5.5@', '=55@', '=5@', ':100_', ':10_0_', '12^x', 'x-12', '/B:007-', '+3.5-1', '+3.5-12', 'LL-',
               'x^x-sil', 'ax^x-sil+5-1']
    labels = list(fixture_phone_labels()) + random_strings(200) + crafted
    want = re_evaluate(re_questions(QFILES['handwritten']), labels)
    keep = [i for i, r in enumerate(want) if r is not None]         # a capture float() refuses is test_capture_errors' subject
    assert len(keep) > len(labels) - 20
    labels, want = [labels[i] for i in keep], np.array([want[i] for i in keep], dtype=np.float32)
    got, status = device_match(n, labels)
    bad = np.argwhere(got != want)
    assert np.array_equal(got, want), [(labels[i], int(j), float(got[i, j]), float(want[i, j])) for i, j in bad[:5]]
    assert not status.any()
    nqs = n.questions.n_qs
    ones, pairs = int(want[:, :nqs].sum()), want[:, :nqs].size
    captured = int((want[:, nqs:] != -1).sum())
    print('re alone: {} of {} (label, QS) pairs are 1 ({:.1%}); {} of {} (label, CQS) pairs capture a number'.format(
        ones, pairs, ones / pairs, captured, want[:, nqs:].size))
    assert 0.05 < ones / pairs < 0.95
    per_question = want[:, :nqs].mean(axis=0)
    assert (per_question > 0).sum() >= nqs - 1 and (per_question < 1).sum() >= nqs - 1      # all but 'Never' / 'All' go both ways
    assert captured > 0.05 * want[:, nqs:].size and (want[:, nqs:] == -1).any()
    # the hand-written cases that matter are really there: a decimal, a shortened run, a never-matching CQS
    assert (want[:, nqs:] % 1 != 0).any() and (want[:, -1] == -1).all()


@pytest.mark.gpu
def test_match_table_in_global_memory_many_labels_and_longest_label(tmp_path):
    """A question set too large for the LDS takes the kernel's other path; more labels than workgroups; a 1024-byte label."""
    rng = np.random.RandomState(3)
    real = fixture_phone_labels()
    lines = []
    for q in range(1200):
        pats = []
        for _ in range(4):
            s = real[rng.randint(len(real))]
            a = rng.randint(0, len(s) - 12); t = s[a:a + rng.randint(2, 12)]
            if rng.randint(3) == 0: t = t[:1] + '?' + t[2:]
            if rng.randint(4) == 0: t = t[:len(t) // 2] + '*' + t[len(t) // 2:]
            pats.append(('' if rng.randint(4) == 0 else '*') + t.replace(',', '') + ('' if rng.randint(4) == 0 else '*'))
        lines.append('QS "q{}" {{{}}}'.format(q, ','.join(pats)))
    lines.append('CQS "c" {/A:(\\d+)_}')
    path = str(tmp_path / 'big.hed')
    with open(path, 'w') as f: f.write('\n'.join(lines) + '\n')
    n = ln.HTSLabelNormalisation(path, subphone_feats='none')
    t = n.questions.host_table()
    assert t['pat_bytes'].nbytes + 8 * len(t['pat_off']) > 48 << 10
    labels = [real[i] for i in rng.randint(0, len(real), size=40)]
    longest = (real[0] * 8)[:1024]
    labels.append(longest)
    want = np.array(re_evaluate(re_questions(path), labels), dtype=np.float32)
    got, status = device_match(n, labels)
    assert np.array_equal(got, want) and not status.any()
    assert 0.02 < want[:, :-1].mean() < 0.98
    # 2600 labels: more than the grid of 8 workgroups per CU
    m = normaliser('handwritten')
    many = [real[i % len(real)] for i in range(2600)]
    got, _ = device_match(m, many)
    first, _ = device_match(m, list(real))
    assert np.array_equal(got, first[np.arange(2600) % len(real)])
    with pytest.raises(ValueError):
        device_match(m, ['x' * 1025])


@pytest.mark.gpu
def test_capture_errors_raise(tmp_path):
    n = normaliser('handwritten')
    _, status = device_match(n, ['/I:1.2.3=', 'a/I:7=5', '/B:1234567890123456-', '/B:123456789012345-', '/I:.=', '/I:.5='])
    kinds = [int(s) & 3 for s in status]
    assert kinds == [ops.LABELS_ERR_FORMAT, 0, ops.LABELS_ERR_DIGITS, 0, ops.LABELS_ERR_FORMAT, 0]
    cqs_keys = [k for k, _, _, _ in n.questions.cqs]
    assert 'Decimal' in cqs_keys[(int(status[0]) >> 2) - 1] and 'Syl_stress' in cqs_keys[(int(status[2]) >> 2) - 1]
    got, _ = device_match(n, ['/B:123456789012345-', '/I:.5=', '/I:0.1=', '/I:12.625='])
    col = lambda key: n.questions.n_qs + [i for i, k in enumerate(cqs_keys) if key in k][0]
    assert got[0, col('Syl_stress')] == np.float32(123456789012345.0)
    assert got[1, col('"Decimal"')] == np.float32(0.5) and got[2, col('"Decimal"')] == np.float32(0.1) and got[3, col('"Decimal"')] == 12.625
    p = tmp_path / 'bad.lab'
    p.write_text(''.join('{} {} x^x-sil+w=ih/I:1.2.3=5[{}]\n'.format(50000 * k, 50000 * (k + 1), k + 2) for k in range(5)))
    with pytest.raises(ValueError, match='Decimal'):
        n.extract_linguistic_features(str(p))


# ---- expansion ----------------------------------------------------------------------------------------------------------------
def expand_in_numpy(V, seg, feats, cc=None):
    """The frame loop of the issue, fp64 then one cast (a restatement)."""
    rows = []
    for phone, first, fn, si, sib, pd, base, _ in seg.tolist():
        for i in range(fn):
            f = {'full': [(i + 1) / fn, (fn - i) / fn, fn, si, sib, pd, fn / pd if pd else 0, (pd - i - base) / pd if pd else 0, (base + i + 1) / pd if pd else 0],
                 'minimal_frame': [(i + 1) / fn, si], 'state_only': [si], 'none': [], 'minimal_phoneme': [(i + 1) / fn, (fn - i) / fn, fn]}.get(feats)
            if feats == 'coarse_coding':
                k = int((200 / float(pd)) * (base + i))
                f = [cc[0, 300 + k], cc[1, 200 + k], cc[2, 100 + k], pd]
            rows.append(np.concatenate([V[phone].astype(np.float64), np.array(f, dtype=np.float64)]))
    return np.array(rows).astype(np.float32)


@pytest.mark.gpu
@pytest.mark.parametrize('feats', ['full', 'minimal_frame', 'state_only', 'none', 'minimal_phoneme', 'coarse_coding'])
@pytest.mark.parametrize('Q', [3, 70])
def test_expand_odd_shapes_and_empty_segments(feats, Q):
    """Widths that are no multiple of four, a row count that is no multiple of the 16-row block, segments without frames at the
    start, in the middle and at the end, one long segment that spans blocks."""
    import torch
    dev = compose._device()
    rng = np.random.RandomState(Q)
    frames = [0, 3, 1, 0, 0, 40, 2, 7, 0, 5, 1, 1, 0, 13, 0]
    P = 4
    V = rng.randn(P, Q).astype(np.float32)
    seg, row = [], 0
    for s, fn in enumerate(frames):
        phone, state = s // 4, s % 4 + 1
        mine = [f for t, f in enumerate(frames) if t // 4 == phone]
        seg.append([phone, row, fn, state, 6 - state, sum(mine), sum(mine[:s % 4]), 0])
        row += fn
    seg = np.array(seg, dtype=np.int32)
    if feats in ('minimal_phoneme',): seg[:, 5], seg[:, 6] = seg[:, 2], 0
    cc = ln.coarse_coding_table()
    want = expand_in_numpy(V, seg, feats, cc)
    got = ops.labels_expand(torch.from_numpy(V).to(dev), torch.from_numpy(seg).to(dev), row, feats,
                            torch.from_numpy(cc).to(dev) if feats == 'coarse_coding' else None).cpu().numpy()
    assert got.shape == want.shape == (73, Q + ops.LABELS_FEATURES[feats])
    assert np.array_equal(got, want)


def coarse_coding_expected(fid):
    """The three coded columns and the duration of every frame, from the formula and the reference's indices (a restatement)."""
    sigma, rows = 0.4, []
    table = [np.exp(-(np.linspace(lo, lo + 3.0, 600) - mu) ** 2 / (2 * sigma ** 2)) / (sigma * math.sqrt(2 * math.pi))
             for lo, mu in ((-1.5, 0.0), (-1.0, 0.5), (-0.5, 1.0))]
    with open(lab(fid, 'phone_align')) as f:
        for line in f:
            start, end = (int(v) for v in line.split()[:2])
            dur = int(end / 50000) - int(start / 50000)
            for i in range(dur):
                k = int((200 / float(dur)) * i)
                rows.append([table[0][300 + k], table[1][200 + k], table[2][100 + k], dur])
    return np.array(rows).astype(np.float32)


@pytest.mark.gpu
@pytest.mark.parametrize('align', ['state_align', 'phone_align'])
def test_coarse_coding_is_the_restated_formula(align):
    """NOT a reference run (mlab.normpdf is gone): question columns and duration against the goldens of 'full' /
    'minimal_phoneme', the coded columns against the formula in numpy, equal after the fp32 cast."""
    n = normaliser('radio416', 'coarse_coding')
    ref = golden('radio416', 'full', 'state_align') if align == 'state_align' else golden('radio416', 'minimal_phoneme', 'phone_align')
    durcol = 416 + 5 if align == 'state_align' else 416 + 2
    for fid in FIDS:
        got = n.extract_linguistic_features(lab(fid, align), label_type=align)
        assert got.shape == (FRAMES[fid], 420) and got.dtype == np.float32
        assert np.array_equal(got[:, :416], ref[fid][:, :416])
        assert np.array_equal(got[:, 419], ref[fid][:, durcol])
        want = coarse_coding_expected(fid)
        assert np.array_equal(got[:, 416:], want), fid
    assert 0 < want[:, :3].min() and want[:, :3].max() < 1.0


# ---- batching -----------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_batching_is_invisible(tmp_path, monkeypatch):
    n = normaliser('radio416')
    ins = [lab(fid) for fid in FIDS]

    def run(name, one_by_one=False):
        d = tmp_path / name
        d.mkdir()
        outs = [str(d / (fid + '.lab')) for fid in FIDS]
        with _hip.KernelTimer() as kt:
            if one_by_one:
                for i, o in zip(ins, outs): n.perform_normalisation([i], [o])
            else:
                n.perform_normalisation(ins, outs)
        launches = [r[0] for r in kt.records]
        assert launches.count('ptts_labels_match') == launches.count('ptts_labels_expand') == len(launches) // 2
        return [open(o, 'rb').read() for o in outs], len(launches) // 2

    single, l1 = run('single', one_by_one=True)
    batch, l2 = run('batch')
    again, _ = run('again')
    monkeypatch.setattr(ln, 'CHUNK_BYTES', 1100 * 425 * 4)      # 747 | 497+293 | 589+453 frames
    chunked, l3 = run('chunked')
    assert (l1, l2, l3) == (5, 1, 3)                            # one match and one expand launch per chunk
    assert single == batch == again == chunked
    want = golden('radio416', 'full', 'state_align')
    for fid, b in zip(FIDS, batch):
        assert b == want[fid].tobytes()


# ---- end to end ---------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_contexts_extraction_end_to_end(tmp_path):
    from percivaltts_amd import modeltts_common, run, vocoders
    import percivaltts_amd
    d = str(tmp_path)
    with open(d + '/ids.scp', 'w') as f: f.write('\n'.join(FIDS) + '\n')
    inpath = d + '/lab_norm/*.lab:(-1,425)'
    res = run.contexts_extraction(os.path.join(G, 'label_state_align', '*.lab'), d + '/ids.scp', QFILES['radio416'], d + '/lab_bin/*.lab',
                                  d + '/lab_w/*.w:(-1,1)', inpath, lab_type='state', id_valid_start=5)
    assert res['size'] == 425 and res['nbframes'] == sum(FRAMES.values())
    want = golden('radio416', 'full', 'state_align')
    X = data.load(inpath, FIDS)
    W = data.load(d + '/lab_w/*.w:(-1,1)', FIDS)
    allrows = np.vstack([want[fid] for fid in FIDS])
    live = allrows.max(axis=0) > allrows.min(axis=0)
    assert 300 < live.sum() < 425
    for fid, x, w in zip(FIDS, X, W):
        assert x.shape == (FRAMES[fid], 425) and x.dtype == np.float32 and w.shape == (FRAMES[fid], 1)
        assert np.array_equal(np.fromfile(d + '/lab_bin/{}.lab'.format(fid), dtype=np.float32).reshape(-1, 425), want[fid])
        assert np.abs(x[:, live]).max() <= 1.0                  # min-max to [-1, 1] wherever the column varies
        assert w[0, 0] == 0.0 and w.max() == 1.0                # the files begin with 'sil'
    stacked = np.vstack(X)
    assert (stacked[:, live].min(axis=0) == -1.0).all() and (stacked[:, live].max(axis=0) == 1.0).all()
    cfg = percivaltts_amd.configuration()
    cfg.arch_hiddenwidth = 8; cfg.train_batch_size = 2
    cfg.arch_ctx_nbcnnlayers = 1; cfg.arch_ctx_winlen = 5
    cfg.arch_gen_nbcnnlayers = 2; cfg.arch_gen_nbfilters = 2; cfg.arch_gen_winlen = 3; cfg.arch_spec_freqlen = 3
    voc = vocoders.VocoderPML(16000, 0.005, 12, 4)
    mod = modeltts_common.Generic(425, voc, layertypes=['FC', 'FC'], cfgarch=cfg)
    y = mod.predict(X[2][None])
    assert y.shape == (1, FRAMES[FIDS[2]], voc.featuressize()) and np.isfinite(y).all()
