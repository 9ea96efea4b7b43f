"""Forced alignment by flat-start Viterbi training (csrc/align.hip, ops.align_viterbi / align_accumulate / align_update /
forced_align_train, label_normalisation.write_state_labels, run.labels_alignment; the definition is the build's own, DESIGN.md
section 3).

The restatement lives here, in fp64 numpy: the emissions with a loop over the columns in index order, the recurrence with the tie
rule (staying wins; the advance replaces it only if strictly greater), the backtrack, accumulate, update and the training loop.

The GPU tolerance of the scores is derived, not tuned.  Both sides are fp64.  With t = x_d - mu_d an emission carries four
roundings per column (the difference, the square, the product with w, the sum), then g and the halving, and the path sum one per
frame; every partial sum is bounded by m(t,n) = 0.5 (sum_d t^2 w + |g|).  With M = sum of m along the restatement's path and
eps = (4 D + T + 4) 2^-52:  (a) |score_dev - score_ref| <= eps M;  (b) the device dur is valid (every dur >= 1, sum dur = T);
(c) the device path's score under the restatement's emissions is >= score_ref - eps M (a near-tie may legitimately be resolved the
other way).  Where every emission is a small multiple of 1/2 (the exact cases) nothing rounds and dur is asserted EQUAL.

The training loop is compared in two ways.  The trajectory -- dur after every iteration, the number of iterations, the changed
frames -- is asserted EQUAL to the restatement's own loop, on a seed for which the restatement shows that no decision along any
chosen path was closer than 1e-6 (fp64 error is near 1e-10 there).  The scores are compared by bound (a), and for that the
restatement is given the model the device aligned with in that iteration (forced_align_train's trace): the device's statistics are
summed in another order than the restatement's, and s2 / count - mu mu cancels, so the two loops' models differ by more than one
emission's roundings although their decisions do not; accumulate and update have their own bounds in their own test."""
import ctypes
import functools
import itertools
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden', 'labels')
U = 2.0 ** -52
S = 5
FLAGS = {'EMPTY': 1, 'TOO_LONG': 2, 'TOO_SHORT': 4, 'NOT_FINITE': 8, 'BAD_OFFSETS': 16, 'BAD_GAUSS': 32}


# ---- the restatement ----------------------------------------------------------------------------------------------------------
def ref_emissions(X, c0, c1, gauss, mu, w, g):
    """e(t,n) = -0.5 (sum_d ((x_d - mu_d) (x_d - mu_d)) w_d + g), fp64, the columns added in index order; also m(t,n)."""
    x = np.asarray(X)[:, c0:c1].astype(np.float64)
    gauss = np.asarray(gauss)
    acc = np.zeros((x.shape[0], gauss.size), dtype=np.float64)
    for d in range(c1 - c0):
        t = x[:, d][:, None] - mu[gauss, d][None, :]
        acc = acc + (t * t) * w[gauss, d][None, :]
    return -0.5 * (acc + g[gauss][None, :]), 0.5 * (acc + np.abs(g[gauss])[None, :])


def ref_viterbi(E):
    """-> (dur, state, score, the smallest difference of two reachable predecessors along the chosen path)."""
    T, N = E.shape
    V = np.full(N, -np.inf)
    V[0] = E[0, 0]
    hist = np.empty((T, N))
    hist[0] = V
    take = np.zeros((T, N), dtype=bool)
    for t in range(1, T):
        adv = np.concatenate([[-np.inf], V[:-1]])
        take[t] = adv > V                                   # staying wins a tie; -inf (unreachable) is never greater
        V = E[t] + np.where(take[t], adv, V)
        hist[t] = V
    state = np.zeros(T, dtype=np.int32)
    n, margin = N - 1, np.inf
    for t in range(T - 1, -1, -1):
        state[t] = n
        if t > 0:
            if n > 0 and np.isfinite(hist[t - 1, n]) and np.isfinite(hist[t - 1, n - 1]):
                margin = min(margin, abs(hist[t - 1, n] - hist[t - 1, n - 1]))
            if take[t, n]:
                n -= 1
    assert n == 0
    return np.bincount(state, minlength=N).astype(np.int32), state, float(V[N - 1]), margin


def path_score(E, dur):
    """The emissions along the path `dur`, added frame by frame."""
    state = np.repeat(np.arange(len(dur)), dur)
    total = 0.0
    for t in range(E.shape[0]):
        total = total + E[t, state[t]]
    return total


def dur_is_valid(dur, T):
    return (np.asarray(dur) >= 1).all() and int(np.sum(dur)) == T


def uniform_dur(T, N):
    n = np.arange(N, dtype=np.int64)
    return ((n + 1) * T // N - n * T // N).astype(np.int32)


def ref_accumulate(Xs, chains, durs, Q, c0, c1, sums=None):
    D = c1 - c0
    count, s1, s2 = sums if sums is not None else (np.zeros(Q, np.int64), np.zeros((Q, D)), np.zeros((Q, D)))
    absum = np.zeros((Q, D)), np.zeros((Q, D))              # sum |terms|, for the bound
    for X, chain, dur in zip(Xs, chains, durs):
        x = X[:, c0:c1].astype(np.float64)
        at = 0
        for q, d in zip(chain, dur):
            for row in x[at:at + d]:
                s1[q] = s1[q] + row
                s2[q] = s2[q] + row * row
                absum[0][q] += np.abs(row)
                absum[1][q] += row * row
            count[q] += d
            at += d
    return (count, s1, s2), absum


def ref_update(count, s1, s2, floor, mu, w, g, min_count):
    mu, w, g = mu.copy(), w.copy(), g.copy()
    kept, floored = np.zeros(len(count), np.int32), np.zeros(len(count), np.int32)
    for q in range(len(count)):
        if count[q] < min_count:
            kept[q] = 1
            continue
        m = s1[q] / count[q]
        var = s2[q] / count[q] - m * m
        floored[q] = int((~(var >= floor)).sum())
        var = np.where(var >= floor, var, floor)
        total = 0.0
        for d in range(len(var)):
            total = total + np.log(var[d])
        mu[q], w[q], g[q] = m, 1.0 / var, total
    return mu, w, g, kept, floored


def ref_floor(Xs, c0, c1, var_floor):
    x = np.concatenate(Xs)[:, c0:c1].astype(np.float64)
    return var_floor * ((x - x.mean(axis=0)) ** 2).mean(axis=0)


def ref_train(Xs, chains, Q, c0, c1, n_iter=20, var_floor=0.01, min_count=2):
    """-> (model, [durs per iteration], history, the smallest decision margin of all iterations)."""
    D = c1 - c0
    floor = ref_floor(Xs, c0, c1, var_floor)
    mu, w, g = np.zeros((Q, D)), np.ones((Q, D)), np.zeros(Q)
    durs = [uniform_dur(X.shape[0], len(c)) for X, c in zip(Xs, chains)]
    sums, _ = ref_accumulate(Xs, chains, durs, Q, c0, c1)
    mu, w, g, kept, floored = ref_update(*sums, floor, mu, w, g, min_count)
    traj, history, margin = [durs], [(float('nan'), sum(X.shape[0] for X in Xs), int(kept.sum()), int(floored.sum()))], np.inf
    prev = [np.repeat(np.arange(len(d)), d) for d in durs]
    for _ in range(n_iter):
        res = [ref_viterbi(ref_emissions(X, c0, c1, c, mu, w, g)[0]) for X, c in zip(Xs, chains)]
        total = 0.0
        for r in res:
            total = total + r[2]
        margin = min([margin] + [r[3] for r in res])
        changed = int(sum((r[1] != p).sum() for r, p in zip(res, prev)))
        durs, prev = [r[0] for r in res], [r[1] for r in res]
        if changed:
            sums, _ = ref_accumulate(Xs, chains, durs, Q, c0, c1)
            mu, w, g, kept, floored = ref_update(*sums, floor, mu, w, g, min_count)
        traj.append(durs)
        history.append((total, changed, int(kept.sum()), int(floored.sum())))
        if changed == 0:
            break
    return (mu, w, g), traj, history, margin


def compositions(T, N):
    """Every way to write T as N positive parts."""
    for cuts in itertools.combinations(range(1, T), N - 1):
        yield np.diff((0,) + cuts + (T,))


# ---- CPU: the restatement against brute force ---------------------------------------------------------------------------------
@pytest.mark.parametrize('T,N', [(5, 5), (6, 5), (9, 5), (8, 3), (7, 1)])
def test_restatement_against_brute_force(T, N):
    rng = np.random.RandomState(100 * T + N)
    E = rng.randn(T, N)
    dur, state, score, _ = ref_viterbi(E)
    best = max(path_score(E, c) for c in compositions(T, N))
    assert abs(score - best) <= 1e-12 * max(1.0, abs(best))
    assert dur_is_valid(dur, T) and (np.repeat(np.arange(N), dur) == state).all()
    assert abs(path_score(E, dur) - score) <= 1e-12 * max(1.0, abs(score))


@pytest.mark.parametrize('T,N', [(5, 5), (6, 5), (9, 5), (8, 3), (7, 1)])
def test_restatement_tie_rule_against_brute_force(T, N):
    """Integer emissions: many paths share the best score.  "Staying wins" picks, walking back from the end, the path that is in the
    highest state as late as it can be: of the best compositions the one with the largest dur[N-1], then dur[N-2], and so on."""
    tied = 0
    for seed in range(6):
        E = np.random.RandomState(1000 * seed + 10 * T + N).randint(-2, 1, size=(T, N)).astype(np.float64)
        dur, _, score, _ = ref_viterbi(E)
        scored = [(path_score(E, c), tuple(c[::-1])) for c in compositions(T, N)]
        best = max(s for s, _ in scored)
        winners = [c for s, c in scored if s == best]
        assert score == best and tuple(dur[::-1]) == max(winners)
        tied += len(winners) > 1
    assert tied > 0 or T == N or N == 1                      # the cases have ties: the rule alone decides there
    dur, _, score, _ = ref_viterbi(np.zeros((T, N)))
    assert dur.tolist() == [1] * (N - 1) + [T - N + 1] and score == 0.0


def test_header_declares_and_library_exports_the_symbols():
    from percivaltts_amd import _hip
    with open(os.path.join(ROOT, 'include', 'percival_hip.h')) as f:
        header = f.read()
    names = ('ptts_align_max_states', 'ptts_align_workspace_bytes', 'ptts_align_viterbi_batch', 'ptts_align_accumulate',
             'ptts_align_update')
    assert 'int ptts_align_max_states(void);' in header
    assert 'size_t ptts_align_workspace_bytes(long long cells, int B, long long t_total);' in header
    for n in names:
        assert n in _hip.SIGNATURES
    assert {n: _hip._define('PTTS_ALIGN_' + n) for n in FLAGS} == FLAGS
    assert [_hip._define('PTTS_ALIGN_PHASE_' + n) for n in ('EMISSIONS', 'TIME_LOOP', 'BACKTRACK', 'ALL')] == [1, 2, 4, 7]
    assert os.path.exists(_hip.LIB_PATH), 'libpercival_hip.so is not built'
    lib = ctypes.CDLL(_hip.LIB_PATH)
    for n in names:
        assert hasattr(lib, n)
    l = _hip.lib()
    assert l.ptts_align_max_states() >= 2048
    assert l.ptts_align_workspace_bytes(1000, 3, 50) >= 1000 * 8 + 50 * 64 // 8
    assert l.ptts_align_workspace_bytes(-1, 3, 50) == 0 and l.ptts_align_workspace_bytes(10, 70000, 50) == 0


def test_ops_checks_without_a_device():
    from percivaltts_amd import ops
    assert ops.align_check(8, [10, 4, 0], [5, 5, 3], 20, (1, 7)) == (1, 7, [50, 0, 0])
    for bad in (dict(Dx=0), dict(cols=(3, 3)), dict(cols=(0, 9)), dict(Q=0), dict(frame_lengths=[10]), dict(state_lengths=[-1, 2, 3])):
        kw = dict(Dx=8, frame_lengths=[10, 4, 0], state_lengths=[5, 5, 3], Q=20, cols=None)
        kw.update(bad)
        with pytest.raises(ValueError):
            ops.align_check(**kw)
    occ, off = ops.align_occurrences(np.array([2, 0, 2, 1, 0]), 4)
    assert occ.tolist() == [1, 4, 3, 0, 2] and off.tolist() == [0, 2, 3, 5, 5] and occ.dtype == np.int32 and off.dtype == np.int64
    with pytest.raises(ValueError):
        ops.align_occurrences(np.array([0, 4]), 4)
    with pytest.raises(ValueError, match='utterance 1: PTTS_ALIGN_TOO_SHORT'):
        ops.align_status('x', np.array([0, 4, 0], dtype=np.int32))
    with pytest.raises(ValueError, match='b.lab: PTTS_ALIGN_NOT_FINITE'):
        ops.align_status('x', np.array([0, 8], dtype=np.int32), names=['a.lab', 'b.lab'])


# ---- CPU: the host side -------------------------------------------------------------------------------------------------------
def _golden_phone_labels():
    from percivaltts_amd.external.merlin import label_normalisation as ln
    return ln.parse_phone_labels(os.path.join(GOLDEN, 'label_state_align', 'arctic_a0005.lab'))


def test_centre_phone():
    from percivaltts_amd.external.merlin import label_normalisation as ln
    phones = _golden_phone_labels()
    assert [ln.centre_phone(p) for p in phones[:5]] == ['sil', 'w', 'ih', 'l', 'w']
    assert ln.centre_phone(phones[1].decode('ascii')) == 'w'
    assert ln.centre_phone('x^x-sil+h=e@1_1') == 'sil' and ln.centre_phone('h^e-l+sil=x@3_1[4]') == 'l'
    assert ln.centre_phone('a~b-pau+c=d:rest', r'([^\~]+)\~([^-]+)-([^\+]+)\+([^=]+)=([^:]+):(.+)') == 'pau'
    with open(os.path.join(GOLDEN, 'label_phone_align', 'arctic_a0002.lab')) as f:
        assert all(ln.centre_phone(line.split()[2]) for line in f)
    with pytest.raises(ValueError, match='f.lab:7.*no centre phone'):
        ln.centre_phone('sil', where='f.lab:7')


def test_write_state_labels_round_trip(tmp_path):
    from percivaltts_amd import run
    from percivaltts_amd.external.merlin import label_normalisation as ln
    phones = _golden_phone_labels()[:6]
    dur = np.random.RandomState(3).randint(1, 9, size=(6, 5))
    dur[0] = 1
    dur[2, 3] = 3000
    dur[5, 4] = 1
    path = str(tmp_path / 'a.lab')
    ln.write_state_labels(path, phones, dur)
    got_phones, segs = ln.parse_label_file(path, 'state_align')
    assert got_phones == phones and segs.shape == (30, 7)
    assert (segs[:, 2].reshape(6, 5) == dur).all() and (segs[:, 3].reshape(6, 5) == np.arange(1, 6)).all()
    assert (segs[:, 1] == np.concatenate([[0], np.cumsum(dur.reshape(-1))[:-1]])).all()
    feats = ln.dur_features(path, 'state_align', 'numerical', 'state', 'phoneme')
    assert feats.dtype == np.float32 and (feats == dur).all()
    with open(path) as f:
        first = f.readline().split()
    assert first[:2] == ['0', '50000'] and first[2].endswith('[2]')
    # the flat [5 P] form and str labels write the same file
    ln.write_state_labels(str(tmp_path / 'b.lab'), [p.decode('ascii') for p in phones], dur.reshape(-1).astype(np.int32))
    assert (tmp_path / 'b.lab').read_text() == (tmp_path / 'a.lab').read_text()
    # per phone: what phone_labels_from_state_labels makes of the state file
    ln.write_phone_labels(str(tmp_path / 'p.lab'), phones, dur)
    run.phone_labels_from_state_labels(str(tmp_path / '*.lab'), ['a'], str(tmp_path / 'phone' / '*.lab'))
    assert (tmp_path / 'p.lab').read_text() == (tmp_path / 'phone' / 'a.lab').read_text()
    ln.write_phone_labels(str(tmp_path / 'q.lab'), phones, dur.sum(axis=1))
    assert (tmp_path / 'q.lab').read_text() == (tmp_path / 'p.lab').read_text()
    assert ln.parse_phone_labels(path) == phones and ln.parse_phone_label_lines(path)[1] == list(range(1, 31, 5))


def test_label_writer_refusals(tmp_path):
    from percivaltts_amd.external.merlin import label_normalisation as ln
    phones = _golden_phone_labels()[:2]
    path = str(tmp_path / 'a.lab')
    with pytest.raises(ValueError, match='shift'):
        ln.write_state_labels(path, phones, np.ones((2, 5), int), shift=0.01)
    with pytest.raises(ValueError, match='shift'):
        ln.write_phone_labels(path, phones, np.ones(2, int), shift=0.004)
    with pytest.raises(ValueError):
        ln.write_state_labels(path, phones, np.ones((2, 4), int))
    with pytest.raises(ValueError):
        ln.write_state_labels(path, phones, np.ones((2, 5)))                 # frames are integers
    with pytest.raises(ValueError):
        ln.write_state_labels(path, phones, -np.ones((2, 5), int))
    assert not os.path.exists(path)


def test_labels_alignment_refuses_before_the_device(tmp_path):
    """A label the expression does not match names file and line; the shift; a feature path without a shape."""
    from percivaltts_amd import run
    (tmp_path / 'a.lab').write_text('x^x-sil+w=ih@x_x[2]\nx^x-sil+w=ih@x_x[3]\n\nnot_a_full_context_label\n')
    with pytest.raises(ValueError, match=r'a\.lab:4.*no centre phone'):
        run.labels_alignment(str(tmp_path / '*.lab'), ['a'], str(tmp_path / '*.cmp:(-1,6)'), str(tmp_path / 'out' / '*.lab'))
    with pytest.raises(ValueError, match='shift'):
        run.labels_alignment(str(tmp_path / '*.lab'), ['a'], str(tmp_path / '*.cmp:(-1,6)'), str(tmp_path / 'out' / '*.lab'), shift=0.01)
    with pytest.raises(ValueError, match='shape'):
        run.labels_alignment(str(tmp_path / '*.lab'), ['a'], str(tmp_path / '*.cmp'), str(tmp_path / 'out' / '*.lab'))
    assert not (tmp_path / 'out').exists()


# ---- GPU ----------------------------------------------------------------------------------------------------------------------
def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _align(utts, mu, w, g, cols=None, **kw):
    """utts: [(X [T,Dx] fp32, chain)] -> the AlignResult of one batched call."""
    from percivaltts_amd import ops
    X = np.concatenate([x for x, _ in utts]).astype(np.float32)
    gauss = np.concatenate([np.asarray(c) for _, c in utts]).astype(np.int32)
    return ops.align_viterbi(_dev(X), [x.shape[0] for x, _ in utts], _dev(gauss), [len(c) for _, c in utts], _dev(mu), _dev(w), _dev(g),
                             cols=cols, **kw)


def _split(res):
    dur, state, score = res.dur.cpu().numpy(), res.state.cpu().numpy(), res.score.cpu().numpy()
    so, fo = res.state_offsets.off, res.frame_offsets.off
    return [(dur[so[b]:so[b + 1]], state[fo[b]:fo[b + 1]], score[b]) for b in range(len(score))]


EXACT_Q, EXACT_D = 7, 3


def _exact_model():
    rng = np.random.RandomState(11)
    return rng.randint(-4, 5, size=(EXACT_Q, EXACT_D)).astype(np.float64), np.ones((EXACT_Q, EXACT_D)), np.zeros(EXACT_Q)


def _exact_utterance(k, T, N):
    """Integer features |x| <= 8: kind 0 random with a random chain, 1 all zero on a chain of one Gaussian (every emission ties),
    2 random with every Gaussian repeated in adjacent states (the neighbours tie in every frame)."""
    rng = np.random.RandomState(7000 + k)
    kind = k % 3
    if kind == 1:
        return np.zeros((T, EXACT_D), np.float32), np.full(N, 3, np.int32), kind
    chain = rng.randint(0, EXACT_Q, size=N) if kind == 0 else np.repeat(rng.randint(0, EXACT_Q, size=(N + 1) // 2), 2)[:N]
    return rng.randint(-8, 9, size=(T, EXACT_D)).astype(np.float32), chain.astype(np.int32), kind


@pytest.mark.gpu
@pytest.mark.parametrize('N', [1, 5, 63, 64, 65, 256, 257, 640, 'max'])
def test_exact_cases(N):
    from percivaltts_amd import ops
    N = ops.align_max_states() if N == 'max' else N
    mu, w, g = _exact_model()
    shapes = [(N, N), (N + 1, N), (2 * N + 3, N)] + ([(3000, 5), (3000, 5), (3000, 5)] if N == 5 else [])
    utts, kinds = [], []
    for k, (T, n) in enumerate(shapes):
        X, chain, kind = _exact_utterance(k + (1 if N % 2 else 0) + N, T, n)
        utts.append((X, chain)); kinds.append(kind)
    if N == 5:
        assert sorted(kinds[3:]) == [0, 1, 2]
    X0 = np.zeros((2 * N + 3, EXACT_D), np.float32)
    utts.append((X0, np.full(N, 3, np.int32))); kinds.append(1)              # the all-zero case at every N
    got = _split(_align(utts, mu, w, g))
    for b, ((X, chain), kind) in enumerate(zip(utts, kinds)):
        E, _ = ref_emissions(X, 0, EXACT_D, chain, mu, w, g)
        assert (E * 2 == np.round(E * 2)).all()                               # multiples of 1/2: nothing rounds
        dur, state, score, _ = ref_viterbi(E)
        np.testing.assert_array_equal(got[b][0], dur, err_msg='utterance {} kind {}'.format(b, kind))
        np.testing.assert_array_equal(got[b][1], state, err_msg='utterance {} kind {}'.format(b, kind))
        assert got[b][2] == score, b
        if kind == 1:
            assert got[b][0].tolist() == [1] * (len(chain) - 1) + [X.shape[0] - len(chain) + 1]


def _raw_viterbi(X, foff, t_total, gauss, soff, n_total, model, Q, B, cells, cols, sizes):
    """ptts_align_viterbi_batch through the C ABI with sentinel-filled outputs of `sizes` = (states, frames) entries."""
    import torch
    from percivaltts_amd import _hip
    dev = X.device
    dur = torch.full((sizes[0],), -7, dtype=torch.int32, device=dev)
    state = torch.full((sizes[1],), -7, dtype=torch.int32, device=dev)
    score = torch.full((B + 8,), -7.0, dtype=torch.float64, device=dev)
    info = torch.full((B + 8,), -7, dtype=torch.int32, device=dev)
    nws = _hip.lib().ptts_align_workspace_bytes(cells, B, t_total)
    ws = torch.empty(nws, dtype=torch.uint8, device=dev)
    _hip.call('ptts_align_viterbi_batch', _hip.ptr(X), _hip.ptr(foff), t_total, X.shape[1], cols[0], cols[1], _hip.ptr(gauss), _hip.ptr(soff),
              n_total, *(_hip.ptr(t) for t in model), Q, B, cells, _hip.ptr(dur), _hip.ptr(state), _hip.ptr(score), _hip.ptr(info), 7,
              _hip.ptr(ws), nws, _hip.stream())
    return tuple(t.cpu().numpy() for t in (dur, state, score, info))


FLAG_CASES = ['too_short', 'no_frames', 'too_long', 'nan', 'bad_gauss', 'offsets_reversed', 'offsets_past_totals']


@pytest.mark.gpu
@pytest.mark.parametrize('case', FLAG_CASES)
def test_flags_and_neighbours(case):
    """The flagged utterance sits in the middle of a batch of five.  Offsets [B+1] are shared boundaries, so an END past the total
    is also the next utterance's START: 'offsets_reversed' flags the middle one alone (its end lies before its start, the
    utterances' rows stay disjoint), 'offsets_past_totals' passes totals five short of the last offset, which flags the last."""
    import torch
    from percivaltts_amd import _hip, ops
    _hip.clear_status()
    cap = ops.align_max_states()
    rng = np.random.RandomState(31)
    Q, Dx, cols = 9, 5, (1, 4)
    D = cols[1] - cols[0]
    mu, w, g = rng.randn(Q, D), 0.5 + rng.rand(Q, D), rng.randn(Q)
    TN = [(12, 5), (70, 66), (9, 4), (30, 30), (200, 130)]
    flagged, want = 2, None
    if case == 'too_short':
        TN[2], want = (6, 7), FLAGS['TOO_SHORT']
    elif case == 'no_frames':
        TN[2], want = (0, 4), FLAGS['EMPTY']
    elif case == 'too_long':
        TN[2], want = (cap + 1, cap + 1), FLAGS['TOO_LONG']
    utts = [(rng.randn(T, Dx).astype(np.float32), rng.randint(0, Q, size=N).astype(np.int32)) for T, N in TN]
    if case == 'nan':
        utts[2][0][5, 2], want = np.nan, FLAGS['NOT_FINITE']
        utts[1][0][3, 0] = utts[3][0][3, 4] = np.nan                          # outside the alignment columns: not read
    elif case == 'bad_gauss':
        utts[2][1][3], want = Q, FLAGS['BAD_GAUSS']
    order = list(range(5))
    if case == 'offsets_reversed':
        order, want = [3, 4, 0, 1], FLAGS['BAD_OFFSETS']                      # rows: utterances 3, 4, then 0, 1; the middle one has none
    present = order if case == 'offsets_reversed' else list(range(5))
    X = _dev(np.concatenate([utts[b][0] for b in present]))
    gauss = _dev(np.concatenate([utts[b][1] for b in present]))
    fstart, sstart, fa, sa = {}, {}, 0, 0
    for b in present:
        fstart[b], sstart[b] = fa, sa
        fa += utts[b][0].shape[0]; sa += len(utts[b][1])
    t_total, n_total = fa, sa
    if case == 'offsets_reversed':                          # boundaries: 0 | 1 | (the flagged one: from the end of 1 back to the start of 3) | 3 | 4
        foff = [fstart[0], fstart[1], fstart[1] + TN[1][0], fstart[3], fstart[4], fstart[4] + TN[4][0]]
        soff = [sstart[0], sstart[1], sstart[1] + TN[1][1], sstart[3], sstart[4], sstart[4] + TN[4][1]]
        assert foff[3] < foff[2] and soff[3] < soff[2]
    else:
        foff = [fstart[b] for b in range(5)] + [t_total]
        soff = [sstart[b] for b in range(5)] + [n_total]
    if case == 'offsets_past_totals':
        t_total, n_total, flagged, want = t_total - 5, n_total - 5, 4, FLAGS['BAD_OFFSETS']
    good = [b for b in range(5) if b != flagged]
    cells = sum(TN[b][0] * TN[b][1] for b in good)
    dur, state, score, info = _raw_viterbi(X, _dev(np.asarray(foff, np.int64)), t_total, gauss, _dev(np.asarray(soff, np.int64)), n_total,
                                           (_dev(mu), _dev(w), _dev(g)), Q, 5, cells, cols, (sa + 16, fa + 16))
    assert info[:5].tolist() == [want if b == flagged else 0 for b in range(5)]
    assert (info[5:] == -7).all() and (score[5:] == -7.0).all() and (dur[sa:] == -7).all() and (state[fa:] == -7).all()
    assert np.isnan(score[flagged])
    written_s, written_f = np.zeros(sa + 16, bool), np.zeros(fa + 16, bool)
    for b in good:                                          # byte-equal to the utterance alone
        solo = _split(_align([utts[b]], mu, w, g, cols=cols))[0]
        ss, fs = slice(soff[b], soff[b] + TN[b][1]), slice(foff[b], foff[b] + TN[b][0])
        assert dur[ss].tobytes() == solo[0].tobytes() and state[fs].tobytes() == solo[1].tobytes(), b
        assert score[b:b + 1].tobytes() == np.float64(solo[2]).tobytes(), b
        assert dur_is_valid(dur[ss], TN[b][0])
        written_s[ss] = written_f[fs] = True
    if want != FLAGS['BAD_OFFSETS']:                        # its slots are known: dur zeros, state -1
        ss, fs = slice(soff[2], soff[2] + TN[2][1]), slice(foff[2], foff[2] + TN[2][0])
        assert (dur[ss] == 0).all() and (state[fs] == -1).all()
        written_s[ss] = written_f[fs] = True
    assert (dur[~written_s] == -7).all() and (state[~written_f] == -7).all()       # nothing else is written
    _hip.check_status()                                     # the device status word is clean
    if case in ('too_short', 'no_frames', 'too_long', 'nan', 'bad_gauss'):      # the wrapper: the bits come back, or the ValueError
        res = _align(utts, mu, w, g, cols=cols, info=torch.zeros(5, dtype=torch.int32, device=X.device))
        assert res.info.cpu().numpy().tolist() == info[:5].tolist()
        assert res.dur.cpu().numpy().tobytes() == dur[:sa].tobytes() and res.state.cpu().numpy().tobytes() == state[:fa].tobytes()
        with pytest.raises(ValueError, match='utterance 2: PTTS_ALIGN_'):
            _align(utts, mu, w, g, cols=cols)


@pytest.mark.gpu
def test_argument_errors_launch_nothing():
    import torch
    from percivaltts_amd import _hip, ops
    rng = np.random.RandomState(2)
    X, gauss = _dev(rng.randn(10, 4).astype(np.float32)), _dev(np.zeros(3, np.int32))
    mu, w, g = _dev(np.zeros((2, 4))), _dev(np.ones((2, 4))), _dev(np.zeros(2))
    off = _dev(np.asarray([0, 10], np.int64)); soff = _dev(np.asarray([0, 3], np.int64))
    out = [torch.zeros(16, dtype=torch.int32, device=X.device) for _ in range(3)] + [torch.zeros(4, dtype=torch.float64, device=X.device)]
    l, p = _hip.lib(), _hip.ptr
    nws = l.ptts_align_workspace_bytes(30, 1, 10)
    ws = torch.empty(nws, dtype=torch.uint8, device=X.device)

    def rc(Dx=4, c0=0, c1=4, Q=2, B=1, phases=7, nws=nws):
        return l.ptts_align_viterbi_batch(p(X), p(off), 10, Dx, c0, c1, p(gauss), p(soff), 3, p(mu), p(w), p(g), Q, B, 30, p(out[0]), p(out[1]),
                                          p(out[3]), p(out[2]), phases, p(ws), nws, _hip.stream())
    EINVAL, EWORKSPACE = -1, -3                                                 # PTTS_EINVAL, PTTS_EWORKSPACE
    assert rc() == 0 and rc(B=0) == 0
    assert [rc(Dx=0), rc(c0=2, c1=2), rc(c1=5), rc(Q=0), rc(B=-1), rc(B=70000), rc(phases=0), rc(phases=8)] == [EINVAL] * 8
    assert rc(nws=nws - 1) == EWORKSPACE
    with pytest.raises(ValueError, match='no backward'):
        ops.align_viterbi(X.clone().requires_grad_(True), [10], gauss, [3], mu, w, g)
    with pytest.raises(ValueError, match='columns'):
        ops.align_viterbi(X, [10], gauss, [3], mu, w, g, cols=(0, 3))
    with pytest.raises(ValueError):
        ops.align_viterbi(X, [9], gauss, [3], mu, w, g)


def _fp_case(D, seed):
    """B = 3 with unequal T and N, Dx > D, c0 > 0; the frames are drawn around the chain's means so that the path is a path."""
    rng = np.random.RandomState(seed)
    Q, c0 = 11, 2
    Dx = c0 + D + 3
    mu, var = rng.randn(Q, D) * 2, 0.5 + 1.5 * rng.rand(Q, D)
    g = np.zeros(Q)
    for d in range(D):
        g = g + np.log(var[:, d])
    utts = []
    for T, N in ((40, 7), (150, 70), (260, 129)):
        chain = rng.randint(0, Q, size=N)
        dur = np.ones(N, int)
        for n in rng.randint(0, N, size=T - N):
            dur[n] += 1
        X = rng.randn(T, Dx)
        X[:, c0:c0 + D] = mu[np.repeat(chain, dur)] + rng.randn(T, D) * np.sqrt(var[np.repeat(chain, dur)])
        utts.append((X.astype(np.float32), chain.astype(np.int32)))
    return utts, (mu, 1.0 / var, g), (c0, c0 + D)


def check_against_restatement(got, utts, model, cols):
    D = cols[1] - cols[0]
    for b, ((X, chain), (dur, state, score)) in enumerate(zip(utts, got)):
        T = X.shape[0]
        E, m = ref_emissions(X, cols[0], cols[1], chain, *model)
        rdur, rstate, rscore, margin = ref_viterbi(E)
        M = float(m[np.arange(T), rstate].sum())
        eps = (4 * D + T + 4) * U
        valid = dur_is_valid(dur, T)
        under = path_score(E, dur) if valid else float('nan')
        print('utterance {} {}x{} D={}: score dev {!r} ref {!r} diff {:.3e} bound {:.3e}; path under ref {:.3e} below; same path {}; '
              'margin {:.3e}'.format(b, T, len(chain), D, score, rscore, abs(score - rscore), eps * M, rscore - under,
                                     bool(valid and (dur == rdur).all()), margin))
        assert abs(score - rscore) <= eps * M, b                                              # (a)
        assert valid and (np.repeat(np.arange(len(chain)), dur) == state).all(), b             # (b)
        assert under >= rscore - eps * M, b                                                   # (c)


@pytest.mark.gpu
@pytest.mark.parametrize('D', [1, 7, 64, 65])
def test_random_cases_against_restatement(D):
    utts, model, cols = _fp_case(D, 50 + D)
    res = _align(utts, *model, cols=cols)
    assert str(res.dur.dtype) == str(res.state.dtype) == str(res.info.dtype) == 'torch.int32' and str(res.score.dtype) == 'torch.float64'
    check_against_restatement(_split(res), utts, model, cols)
    again = _align(utts, *model, cols=cols)                                     # the same input gives the same bytes
    for a, b in ((res.dur, again.dur), (res.state, again.state), (res.score, again.score)):
        assert a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes()
    nostate = _align(utts, *model, cols=cols, want_state=False)
    assert nostate.state is None and nostate.dur.cpu().numpy().tobytes() == res.dur.cpu().numpy().tobytes()


@pytest.mark.gpu
def test_batch_split_over_the_workspace_budget():
    from percivaltts_amd import _hip
    utts, model, cols = _fp_case(7, 57)
    whole = _align(utts, *model, cols=cols)
    with _hip.KernelTimer() as kt:
        parts = _align(utts, *model, cols=cols, workspace_bytes=1 << 16)
    assert len(kt.durations_ms()) == 3                                          # one utterance a call
    for a, b in ((whole.dur, parts.dur), (whole.state, parts.state), (whole.score, parts.score), (whole.info, parts.info)):
        assert a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes()


@pytest.mark.gpu
def test_accumulate_and_update():
    import torch
    from percivaltts_amd import ops
    rng = np.random.RandomState(8)
    Q, Dx, cols, min_count = 9, 70, (3, 69), 3
    D = cols[1] - cols[0]
    chains = [rng.randint(0, Q - 2, size=N) for N in (6, 40, 1)]                 # Gaussians Q-2 and Q-1 never occur
    chains[1][5] = Q - 2                                                         # ... Q-2 once, with two frames: below min_count
    durs = [rng.randint(1, 6, size=len(c)) for c in chains]
    durs[1][5] = 2
    chains[2][0], durs[2][0] = Q - 3, 300                                         # one long state
    Xs = [(3.0 + 2.0 * rng.randn(int(d.sum()), Dx)).astype(np.float32) for d in durs]
    for X, c, d in zip(Xs, chains, durs):                                        # Gaussian 0 is constant in column 0: its variance takes the floor
        X[np.repeat(c, d) == 0, cols[0]] = 1.5
    assert any((c == 0).sum() for c in chains)
    X, gauss = _dev(np.concatenate(Xs)), _dev(np.concatenate(chains).astype(np.int32))
    dur = _dev(np.concatenate(durs).astype(np.int32))
    fl, sl = [x.shape[0] for x in Xs], [len(c) for c in chains]
    occ, occ_off = (_dev(a) for a in ops.align_occurrences(np.concatenate(chains), Q))
    (rcount, rs1, rs2), (a1, a2) = ref_accumulate(Xs, chains, durs, Q, *cols)
    count, s1, s2 = ops.align_accumulate(X, fl, gauss, sl, dur, occ, occ_off, Q, cols)
    assert str(count.dtype) == 'torch.int64' and (count.cpu().numpy() == rcount).all() and rcount[Q - 1] == 0 and rcount[Q - 2] == 2
    err1, err2 = np.abs(s1.cpu().numpy() - rs1), np.abs(s2.cpu().numpy() - rs2)
    bound1, bound2 = rcount[:, None] * U * a1, rcount[:, None] * U * a2          # n_q 2^-52 sum |terms| (both sides: n_q - 1 roundings each)
    print('accumulate: largest error over its bound: s1 {:.3f} s2 {:.3f}'.format((err1 / np.maximum(bound1, 1e-300)).max(),
                                                                                 (err2 / np.maximum(bound2, 1e-300)).max()))
    assert (err1 <= bound1).all() and (err2 <= bound2).all()
    # the same call on fresh zeroed arrays: identical bytes
    again = ops.align_accumulate(X, fl, gauss, sl, dur, occ, occ_off, Q, cols)
    for a, b in zip((count, s1, s2), again):
        assert a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes()
    # a second call adds to the first: the corpus in two calls (per utterance tables) against both utterance sets' restatement
    sums = None
    for part in ([0], [1, 2]):
        pc = [chains[b] for b in part]
        pocc, poff = (_dev(a) for a in ops.align_occurrences(np.concatenate(pc), Q))
        sums = ops.align_accumulate(_dev(np.concatenate([Xs[b] for b in part])), [fl[b] for b in part], _dev(np.concatenate(pc).astype(np.int32)),
                                    [sl[b] for b in part], _dev(np.concatenate([durs[b] for b in part]).astype(np.int32)), pocc, poff, Q, cols,
                                    sums=sums)
    assert (sums[0].cpu().numpy() == rcount).all()
    assert (np.abs(sums[1].cpu().numpy() - rs1) <= bound1).all() and (np.abs(sums[2].cpu().numpy() - rs2) <= bound2).all()
    # a Gaussian without frames is untouched: sentinels survive
    sent = (torch.full((Q,), 5, dtype=torch.int64, device=X.device), torch.full((Q, D), 0.25, dtype=torch.float64, device=X.device),
            torch.full((Q, D), 0.75, dtype=torch.float64, device=X.device))
    ops.align_accumulate(X, fl, gauss, sl, dur, occ, occ_off, Q, cols, sums=sent)
    assert sent[0][Q - 1].item() == 5 and (sent[1][Q - 1] == 0.25).all().item() and (sent[2][Q - 1] == 0.75).all().item()
    assert sent[0][0].item() == 5 + rcount[0]
    # a flagged utterance's zeros add nothing
    zero = ops.align_accumulate(X, fl, gauss, sl, torch.zeros_like(dur), occ, occ_off, Q, cols)
    assert all((t == 0).all().item() for t in zero)
    # update: the floor branch (Gaussian 0, column 0) and the min_count branch (Gaussians Q-2, Q-1) are both taken
    floor = ref_floor(Xs, cols[0], cols[1], 0.01)
    mu0, w0, g0 = rng.randn(Q, D), 0.5 + rng.rand(Q, D), rng.randn(Q)
    rmu, rw, rg, rkept, rfloored = ref_update(rcount, s1.cpu().numpy(), s2.cpu().numpy(), floor, mu0, w0, g0, min_count)
    assert rkept.tolist() == [0] * (Q - 2) + [1, 1] and rfloored[0] >= 1 and rfloored[1:].sum() == 0
    mu, w, g = _dev(mu0), _dev(w0), _dev(g0)
    kept, floored = ops.align_update(count, s1, s2, _dev(floor), mu, w, g, min_count)
    assert (kept.cpu().numpy() == rkept).all() and (floored.cpu().numpy() == rfloored).all()
    mu, w, g = mu.cpu().numpy(), w.cpu().numpy(), g.cpu().numpy()
    assert mu[Q - 2:].tobytes() == mu0[Q - 2:].tobytes() and w[Q - 2:].tobytes() == w0[Q - 2:].tobytes() and g[Q - 2:].tobytes() == g0[Q - 2:].tobytes()
    # the same statistics, the same operations: one division, one product and one difference each; the log is the library's
    assert mu.tobytes() == rmu.tobytes()
    assert (np.abs(w / rw - 1.0) <= 4 * U).all() and w[0, 0] == 1.0 / floor[0]
    glim = (4 + D) * U * np.abs(np.log(1.0 / rw)).sum(axis=1)                      # at most 4 ulp per logarithm, D - 1 partial sums
    print('update: g largest error over its bound {:.3f}'.format((np.abs(g - rg) / glim)[:Q - 2].max()))
    assert (np.abs(g - rg) <= glim).all()


# ---- the loop -----------------------------------------------------------------------------------------------------------------
LOOP_SEED = 3
LOOP_MODELS = ['sil', 'w', 'ih', 'l']
LOOP_COLS, LOOP_DX = (1, 7), 8


@functools.lru_cache(maxsize=None)
def loop_corpus(seed=LOOP_SEED):
    """12 utterances, 4 models x 5 states, D = 6 (columns 1 .. 6 of 8), 6 phones each, true state durations 1 .. 6, integer means in
    [-8, 8], Gaussian noise of sigma 1 -> (Xs, chains, phone model indices per utterance)."""
    rng = np.random.RandomState(seed)
    Q, D = len(LOOP_MODELS) * S, LOOP_COLS[1] - LOOP_COLS[0]
    means = rng.randint(-8, 9, size=(Q, D)).astype(np.float64)
    Xs, chains, phones = [], [], []
    for u in range(12):
        ph = rng.randint(0, len(LOOP_MODELS), size=6)
        ph[u % 6] = u % len(LOOP_MODELS)                                        # every model occurs
        chain = (ph[:, None] * S + np.arange(S)[None, :]).reshape(-1)
        dur = rng.randint(1, 7, size=chain.size)
        X = rng.randn(int(dur.sum()), LOOP_DX)
        X[:, LOOP_COLS[0]:LOOP_COLS[1]] += means[np.repeat(chain, dur)]
        Xs.append(X.astype(np.float32)); chains.append(chain); phones.append(ph)
    return Xs, chains, phones


@functools.lru_cache(maxsize=None)
def loop_reference():
    Xs, chains, _ = loop_corpus()
    return ref_train(Xs, chains, len(LOOP_MODELS) * S, *LOOP_COLS)


def test_loop_precondition_on_the_restatement():
    """Asserted on the restatement alone: no decision along a chosen path closer than 1e-6, the loop converges, the total score never
    decreases.  (Flat-start Viterbi training stops in local optima: the true boundaries are not asserted.)"""
    _, traj, history, margin = loop_reference()
    print('loop: {} iterations, margin {:.3e}, history {}'.format(len(history), margin, history))
    assert margin >= 1e-6
    assert 2 < len(history) <= 21 and history[-1][1] == 0 and all(h[1] > 0 for h in history[:-1])
    totals = [h[0] for h in history[1:]]
    assert all(b >= a for a, b in zip(totals, totals[1:]))
    assert all(dur_is_valid(d, X.shape[0]) for durs in traj for d, X in zip(durs, loop_corpus()[0]))


def _score_bound(Xs, chains, durs, model, cols):
    """sum over the utterances of eps M (item (a) of the module docstring) along the paths `durs`, and the scores under `model`."""
    bound, scores = 0.0, []
    for X, chain, dur in zip(Xs, chains, durs):
        E, m = ref_emissions(X, cols[0], cols[1], chain, *model)
        state = np.repeat(np.arange(len(dur)), dur)
        bound += (4 * (cols[1] - cols[0]) + X.shape[0] + 4) * U * float(m[np.arange(X.shape[0]), state].sum())
        scores.append(ref_viterbi(E)[2])
    return bound, scores


@pytest.mark.gpu
def test_training_loop_equals_the_restatement():
    from percivaltts_amd import ops
    Xs, chains, _ = loop_corpus()
    _, traj, history, _ = loop_reference()
    Q = len(LOOP_MODELS) * S
    trace = []
    model, dur, hist = ops.forced_align_train(_dev(np.concatenate(Xs)), [x.shape[0] for x in Xs], chains, Q, *LOOP_COLS, trace=trace,
                                              workspace_bytes=1 << 18)             # several chunks of utterances
    print('device history {}'.format(hist))
    print('restatement    {}'.format(history))
    assert len(hist) == len(history) == len(trace)
    off = np.concatenate([[0], np.cumsum([len(c) for c in chains])])
    for it, (ref_durs, entry) in enumerate(zip(traj, trace)):
        for b, rd in enumerate(ref_durs):
            np.testing.assert_array_equal(entry[0][off[b]:off[b + 1]], rd, err_msg='iteration {} utterance {}'.format(it, b))
    np.testing.assert_array_equal(dur.cpu().numpy(), np.concatenate(traj[-1]))
    assert [h[1:] for h in hist] == [h[1:] for h in history]                     # changed frames, kept Gaussians, floored variances
    assert np.isnan(hist[0][0])
    slack = []
    for it in range(1, len(hist)):                                              # the totals, by (a), under the model the device aligned with
        _, scores, mu, w, g = trace[it]
        bound, rscores = _score_bound(Xs, chains, traj[it], (mu, w, g), LOOP_COLS)
        total = 0.0
        for v in rscores:
            total = total + v
        bound += len(Xs) * U * sum(abs(v) for v in rscores)                      # the sum over the utterances
        print('iteration {}: total dev {!r} ref (device model) {!r} ref (own loop) {!r} diff {:.3e} bound {:.3e}'.format(
            it, hist[it][0], total, history[it][0], abs(hist[it][0] - total), bound))
        assert abs(hist[it][0] - total) <= bound
        slack.append(bound)
    for a, b, s in zip(hist[1:], hist[2:], slack[1:]):                           # non-decreasing, within the bound
        assert b[0] >= a[0] - s
    # the model: what the restatement's update makes of the last segmentation, to the accuracy of the statistics: a sum of
    # n_q < 100 terms is good to n_q 2^-52 = 2e-14 relative, and s2 / count - mu mu loses a factor (mu^2 + var) / var <= 65 / 0.26
    # (means within 8, noise of variance 1, the floor 0.01 x the columns' variance of about 26): 6e-12
    rmu, rw, rg = loop_reference()[0]
    mu, var = model.host()
    assert np.abs(mu - rmu).max() <= 1e-12 and np.abs(var * rw - 1.0).max() <= 1e-9
    # align only, with the stored model: the final alignment again
    m2, dur2, hist2 = ops.forced_align_train(_dev(np.concatenate(Xs)), [x.shape[0] for x in Xs], chains, Q, *LOOP_COLS, n_iter=0,
                                             model=ops.AlignModel.from_host(mu, var, 'cuda'))
    assert len(hist2) == 1 and dur2.cpu().numpy().tobytes() == dur.cpu().numpy().tobytes()
    with pytest.raises(ValueError, match='utterance 1: PTTS_ALIGN_TOO_SHORT'):
        ops.forced_align_train(_dev(np.concatenate(Xs[:2])), [Xs[0].shape[0] + Xs[1].shape[0] - 3, 3], chains[:2], Q, *LOOP_COLS)


LABEL_TAIL = '/A:0_0_0/B:1-1-3@1-1&1-7#1-5$1-3!0-1;0-1|ih/C:1+1+2/D:0_0/E:md+1@1+5&1+4#0+1/F:content_1/G:0_0/H:7=5@1=1|L-L%/I:0=0/J:7+5-1'


def _write_loop_corpus(tmp_path):
    """Untimed full-context labels (one phone per line, in the golden files' shape) and the feature files of loop_corpus."""
    Xs, _, phones = loop_corpus()
    fids = ['utt{:02d}'.format(u) for u in range(len(Xs))]
    os.makedirs(str(tmp_path / 'lab')); os.makedirs(str(tmp_path / 'cmp'))
    for fid, X, ph in zip(fids, Xs, phones):
        names = ['x', 'x'] + [LOOP_MODELS[p] for p in ph] + ['x', 'x']
        with open(str(tmp_path / 'lab' / (fid + '.lab')), 'w') as f:
            for i in range(len(ph)):
                f.write('{}^{}-{}+{}={}@{}_{}{}\n'.format(names[i], names[i + 1], names[i + 2], names[i + 3], names[i + 4], i + 1,
                                                          len(ph) - i, LABEL_TAIL))
        X.tofile(str(tmp_path / 'cmp' / (fid + '.cmp')))
    return fids


@pytest.mark.gpu
def test_labels_alignment_end_to_end(tmp_path):
    from percivaltts_amd import run
    from percivaltts_amd.external.merlin import label_normalisation as ln
    Xs, chains, phones = loop_corpus()
    _, traj, history, _ = loop_reference()
    fids = _write_loop_corpus(tmp_path)
    lab, cmp_, out = str(tmp_path / 'lab' / '*.lab'), str(tmp_path / 'cmp' / '*.cmp:(-1,{})'.format(LOOP_DX)), str(tmp_path / 'aligned' / '*.lab')
    model_file = str(tmp_path / 'models' / 'mono.npz')
    hist = run.labels_alignment(lab, fids, cmp_, out, cols=LOOP_COLS, model_out=model_file)
    assert [h[1:] for h in hist] == [h[1:] for h in history]
    for b, fid in enumerate(fids):
        got_phones, segs = ln.parse_label_file(out.replace('*', fid), 'state_align')
        assert got_phones == ln.parse_phone_labels(lab.replace('*', fid)) and len(got_phones) == 6
        np.testing.assert_array_equal(segs[:, 2], traj[-1][b], err_msg=fid)
        assert ln.dur_features(out.replace('*', fid), 'state_align', 'numerical', 'state', 'phoneme').shape == (6, 5)
    with np.load(model_file) as z:
        assert [str(n) for n in z['names']] == sorted(LOOP_MODELS) and z['mu'].shape == z['var'].shape == (20, 6) and (z['var'] > 0).all()
    # the label front end takes the files as they are (the handwritten question set fits these label strings)
    norm = ln.HTSLabelNormalisation(os.path.join(GOLDEN, 'questions-handwritten.hed'), add_frame_features=True, subphone_feats='full')
    os.makedirs(str(tmp_path / 'bin'))
    norm.perform_normalisation([out.replace('*', fid) for fid in fids[:3]], [str(tmp_path / 'bin' / (fid + '.lab')) for fid in fids[:3]],
                               label_type='state_align')
    for fid, X in zip(fids[:3], Xs):
        assert os.path.getsize(str(tmp_path / 'bin' / (fid + '.lab'))) == X.shape[0] * norm.dimension * 4
    # a second run with the stored model and n_iter=0 reproduces the final alignment; phone-level output is the state file's per phone
    out2 = str(tmp_path / 'again' / '*.lab')
    hist2 = run.labels_alignment(out, fids, cmp_, out2, cols=LOOP_COLS, n_iter=0, model_in=model_file)     # timed input: the times are ignored
    assert len(hist2) == 1
    out3 = str(tmp_path / 'phone' / '*.lab')
    run.labels_alignment(lab, fids, cmp_, out3, cols=LOOP_COLS, n_iter=0, model_in=model_file, lab_type='phone')
    run.phone_labels_from_state_labels(out, fids, str(tmp_path / 'phone_ref' / '*.lab'))
    for fid in fids:
        with open(out.replace('*', fid)) as a, open(out2.replace('*', fid)) as b:
            assert a.read() == b.read()
        with open(out3.replace('*', fid)) as a, open(str(tmp_path / 'phone_ref' / (fid + '.lab'))) as b:
            assert a.read() == b.read()
    # an utterance that cannot be aligned names its file and its flag; a phone without a stored model names the file
    short = np.zeros((20, LOOP_DX), np.float32)
    short.tofile(str(tmp_path / 'cmp' / 'utt03.cmp'))
    with pytest.raises(ValueError, match=r'utt03\.lab: PTTS_ALIGN_TOO_SHORT'):
        run.labels_alignment(lab, fids, cmp_, str(tmp_path / 'x' / '*.lab'), cols=LOOP_COLS)
    Xs[3].tofile(str(tmp_path / 'cmp' / 'utt03.cmp'))
    with open(str(tmp_path / 'lab' / 'utt04.lab')) as f:
        text = f.read()
    with open(str(tmp_path / 'lab' / 'utt04.lab'), 'w') as f:
        f.write(text.replace('-{}+'.format(LOOP_MODELS[phones[4][0]]), '-zz+', 1))
    with pytest.raises(ValueError, match=r"utt04\.lab: the phone 'zz' has no model"):
        run.labels_alignment(lab, fids, cmp_, str(tmp_path / 'x' / '*.lab'), cols=LOOP_COLS, n_iter=0, model_in=model_file)
