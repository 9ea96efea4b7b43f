"""Waveform analysis over a batch of utterances (ops.wave_peak, ops.f0_track_device, the *_batch forms of the seven analysis ops,
VocoderPML / VocoderWORLDAnalysisDevice.analysis_device_batch, run.features_extraction(batch_size=)): a batch gives every utterance,
byte for byte, what the per-utterance path gives that utterance alone, in one launch per kernel.

Equality, not a tolerance: a frame is computed by the same device function from the same samples and rows, and ptts_f0_track repeats
ops.f0_track's fp64 operations one by one.  The one value that is not the single path's bit for bit is the waveform's peak (a
fixed-order fp64 sum against torch's): it is held to 1e-12 relative, far above the error of an fp64 mean over a few 10^5 fp32
samples (about N 2^-53 relative to the largest sample), and the estimated path is compared through ops.f0_candidates' own gpeak
argument.  One comparison against the fp64 restatements of tests/test_analysis.py and tests/test_worldanalysis.py, with their
bounds, ties the batched kernels to the definition as well."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_analysis as ta                                      # noqa: E402
import test_f0 as tf                                            # noqa: E402
import test_f0_refine as tr                                     # noqa: E402
import test_pulsesynth as ps                                    # noqa: E402
import test_pulsetable as tt                                    # noqa: E402  (the two shapes of the batched synthesis)
import test_worldanalysis as wa                                 # noqa: E402

SHIFT = ps.SHIFT
F0_MIN, F0_MAX = 100.0, 400.0
A, B = tt.A, tt.B                                               # shape A: fs 8000, dftlen 512; shape B: fs 32000, dftlen 4096
NB = 5
ESTIMATED = (0, 2, 3, 4)                                        # the utterances of batch A whose estimated track has a voiced frame
_batches = {}


def _dev(a, dtype=torch.float32):
    return torch.tensor(np.asarray(a), dtype=dtype).cuda().contiguous()


def frame_count(N, fs):
    T = 0
    while tf.rnd(T * SHIFT * fs) <= N:
        T += 1
    return T


def batch(name):
    """Shape A: five utterances of unequal length cut or joined from the signals of tests/test_f0.py (signal A: a noise stretch
    and a silent tail), tests/test_analysis.py and tests/test_f0_refine.py, with a given track each: unvoiced runs at the start, in
    the middle and at the end, values below f0_min and above f0_max, one utterance of a single frame, one whose track is longer
    than its waveform allows.  Shape B: two short utterances."""
    if name not in _batches:
        if name == 'A':
            fs = A['fs']
            sa, an = tf.case('A'), ta.case('A')
            fm, exact = tr.fm_signal(fs, 30)
            wavs = [sa['wav'], an['wav'][:10], an['wav'], np.concatenate([fm, sa['wav'][:1500]]), sa['wav'][900:2700]]
            f0s = [sa['64']['f0'].astype(np.float32), np.array([200.0], dtype=np.float32)]
            t2 = np.concatenate([an['f0'], np.full(7, 180.0, dtype=np.float32)])         # 47 frames for 40: cropped
            t2[:3] = 0.0
            t2[10], t2[11] = 90.0, 450.0
            f0s.append(t2)
            T3 = frame_count(len(wavs[3]), fs)
            t3 = (170.0 + 60.0 * np.sin(np.arange(T3) / 7.0)).astype(np.float32)
            t3[:len(exact)] = exact.astype(np.float32)
            t3[35:41] = 0.0
            f0s.append(t3)
            T4 = frame_count(len(wavs[4]), fs)
            t4 = np.full(T4, 150.0, dtype=np.float32)
            t4[-6:] = 0.0
            f0s.append(t4)
        else:
            fs = B['fs']
            w0, e0 = tr.fm_signal(fs, 14, seed=29)
            w1, e1 = tr.fm_signal(fs, 10, seed=3)
            wavs, f0s = [w0, w1[:-100]], [e0.astype(np.float32), e1.astype(np.float32)]
            f0s[1][0] = 0.0
        wavs = [np.ascontiguousarray(w, dtype=np.float32) for w in wavs]
        for a in wavs + f0s:
            a.setflags(write=False)
        _batches[name] = (A if name == 'A' else B, wavs, f0s)
    return _batches[name]


def packed(arrays, dtype=np.float32):
    return _dev(np.concatenate([np.asarray(a, dtype=dtype) for a in arrays]), dtype=torch.float64 if dtype == np.float64 else torch.float32)


def host_tracks(shape, wavs, f0s):
    from percivaltts_amd import ops
    return [ops.f0_track(f, F0_MIN, F0_MAX, shape['fs'], SHIFT, shape['L'], wavlen=len(w)) for w, f in zip(wavs, f0s)]


def split(t, lengths):
    return [x.cpu().numpy() for x in t.split(list(lengths))]


# ---------------------------------------------------------------------------------------------------------------------------
# 7: refusals that need no device
# ---------------------------------------------------------------------------------------------------------------------------
def vocoder(kind, shape=None, spec_type='fwbnd'):
    from percivaltts_amd import vocoders
    shape = A if shape is None else shape
    if kind == 'PML':
        return vocoders.VocoderPML(shape['fs'], SHIFT, 9, 9, dftlen=shape['L'], spec_type=spec_type)
    return vocoders.VocoderWORLDAnalysisDevice(shape['fs'], SHIFT, 9, 4, dftlen=shape['L'], spec_type=spec_type)


@pytest.mark.parametrize('kind', ['PML', 'WORLD'])
def test_refusals_without_a_device(kind, tmp_path, monkeypatch):
    voc = vocoder(kind)
    wav, f0 = np.zeros(400), np.full(11, 150.0)
    with pytest.raises(ValueError, match='mixture'):
        voc.analysis_device_batch([wav, wav], [f0, None], F0_MIN, F0_MAX)
    with pytest.raises(ValueError, match='mixture'):
        voc.analysis_device_batch([wav, wav], [f0], F0_MIN, F0_MAX)
    with pytest.raises(ValueError, match='no utterance'):
        voc.analysis_device_batch([], None, F0_MIN, F0_MAX)
    bad = wav.copy()
    bad[7] = np.inf
    for f0s in (None, [f0, f0, f0]):
        with pytest.raises(ValueError, match='utterance 1: wav is not a finite'):
            voc.analysis_device_batch([wav, bad, wav], f0s, F0_MIN, F0_MAX)
    with pytest.raises(ValueError, match='utterance 1'):
        voc.analysis_device_batch([wav, wav], [f0, np.zeros((2, 5))], F0_MIN, F0_MAX)       # a track of the wrong rank
    with pytest.raises(ValueError, match='utterance 0'):
        voc.analysis_device_batch([wav], [np.zeros(0)], F0_MIN, F0_MAX)
    with pytest.raises(ValueError):
        voc.analysis_device_batch([wav], [f0], F0_MIN, 5000.0)                              # the checks of the single path
    import importlib
    monkeypatch.setenv('PERCIVAL_CORPUS', str(tmp_path / 'corpus'))
    monkeypatch.chdir(tmp_path)
    import percivaltts_amd.run as run
    run = importlib.reload(run)
    for k in (0, -1, 1.5):
        with pytest.raises(ValueError, match='batch_size'):
            run.features_extraction(None, fids=['a'], batch_size=k)


def test_interface_without_a_device():
    import inspect
    from percivaltts_amd import _hip, ops, ops_offline
    for name in ('wave_peak', 'f0_track_device', 'f0_candidates_batch', 'f0_viterbi_batch', 'f0_estimate_batch', 'f0_refine_batch',
                 'frame_harmonics_batch', 'phase_coherence_batch', 'world_envelope_batch', 'world_aperiodicity_batch'):
        assert getattr(ops, name) is getattr(ops_offline, name) and name in ops_offline.__all__
    assert list(inspect.signature(ops.f0_track_device).parameters)[:8] == ['f0', 'frame_lengths', 'wav_lengths', 'f0_min', 'f0_max', 'fs',
                                                                           'shift', 'dftlen']
    assert list(inspect.signature(ops.wave_peak).parameters)[:2] == ['wav', 'wav_lengths']
    for name in ('ptts_wave_peak', 'ptts_f0_track', 'ptts_f0_candidates_batch', 'ptts_f0_viterbi_batch', 'ptts_f0_refine_batch',
                 'ptts_frame_harmonics_batch', 'ptts_phase_coherence_batch', 'ptts_world_envelope_batch', 'ptts_world_aperiodicity_batch'):
        assert name in _hip.SIGNATURES
    assert [_hip._define('PTTS_ANALYSIS_' + n) for n in ('BAD_WAV', 'BAD_F0', 'NO_VOICED')] == [1, 2, 4]
    with pytest.raises(ValueError):
        ops.packed_offsets([], 'cpu')
    with pytest.raises(ValueError):
        ops.packed_offsets([3, -1], 'cpu')


# ---------------------------------------------------------------------------------------------------------------------------
# 1: the track
# ---------------------------------------------------------------------------------------------------------------------------
def tracks_of_every_kind():
    """(f0, the samples of its waveform at shape A) pairs: leading, trailing and interior unvoiced runs, values outside [f0_min,
    f0_max] on both sides (among them the float32 neighbours of the bounds from outside), a single voiced frame, a single frame,
    a cropped track, one longer than the workgroup has lanes (several frames a lane) and one that is not float32-representable."""
    rng = np.random.RandomState(5)
    _, wavs, f0s = batch('A')
    out = [(f.astype(np.float64), len(w)) for w, f in zip(wavs, f0s)]
    one = np.zeros(23)
    one[9] = 222.2
    out.append((one, 40 * 22))
    lo, hi = np.float32(F0_MIN), np.float32(F0_MAX)
    edge = np.array([0.0, 99.99999, np.nextafter(lo, np.float32(0)), lo, np.nextafter(hi, np.float32(1e9)), 400.00001, 1e-30, 5000.0, 0.0, 0.0, 250.0, 0.0])
    out.append((edge, 40 * 11))
    longt = 100.0 + 300.0 * rng.rand(1500)
    longt[rng.rand(1500) < 0.6] = 0.0
    longt[:5] = 0.0
    longt[700:1100] = 0.0                                       # a run that spans many lanes
    longt[-300:] = 0.0
    out.append((longt, 40 * 1499))
    out.append((np.array([0.0, 100.0 + 1e-9, 0.0, 0.0, 399.0 + 1e-7 / 3, 0.0]), 40 * 3))         # cropped to four frames
    return out


@pytest.mark.gpu
@pytest.mark.parametrize('F0_MIN,F0_MAX', [(100.0, 400.0), (100.1, 399.95)])
@pytest.mark.parametrize('dtype', [np.float32, np.float64])
def test_f0_track_device_equals_the_host(dtype, F0_MIN, F0_MAX, capsys):
    """The second pair of bounds is not float32-representable: float32(100.1) lies below 100.1 and float32(399.95) above 399.95, so
    a clipped value takes the one-ulp correction on either side."""
    from percivaltts_amd import ops
    assert (float(np.float32(F0_MIN)) < F0_MIN and float(np.float32(F0_MAX)) > F0_MAX) == (F0_MIN != 100.0)
    cases = [(f.astype(dtype), N) for f, N in tracks_of_every_kind()]
    want = []
    for f, N in cases:
        want.append(ops.f0_track(f, F0_MIN, F0_MAX, A['fs'], SHIFT, A['L'], wavlen=N))
    host_lines = capsys.readouterr().out
    track, vuv, oo = ops.f0_track_device(packed([f for f, _ in cases], dtype), [len(f) for f, _ in cases], [N for _, N in cases], F0_MIN,
                                         F0_MAX, A['fs'], SHIFT, A['L'])
    assert capsys.readouterr().out == host_lines and host_lines.count('are cropped') == 2
    assert track.dtype == vuv.dtype == torch.float32 and oo.lengths == [len(w) for w in want] and oo.lengths[2] == 40
    got, gv = split(track, oo.lengths), split(vuv, oo.lengths)
    for b, (f, _) in enumerate(cases):
        np.testing.assert_array_equal(got[b], want[b], err_msg='utterance {}'.format(b))
        np.testing.assert_array_equal(gv[b], (f[:len(want[b])] > 0).astype(np.float32))
        assert (got[b].astype(np.float64) >= F0_MIN).all() and (got[b].astype(np.float64) <= F0_MAX).all()
    # a batch of one equals the same utterance inside the batch
    for b in (0, 2, 7):
        f, N = cases[b]
        alone, _, _ = ops.f0_track_device(packed([f], dtype), [len(f)], [N], F0_MIN, F0_MAX, A['fs'], SHIFT, A['L'])
        np.testing.assert_array_equal(alone.cpu().numpy(), got[b])


@pytest.mark.gpu
def test_f0_track_device_status():
    from percivaltts_amd import ops
    ok = np.full(6, 150.0)
    args = (F0_MIN, F0_MAX, A['fs'], SHIFT, A['L'])
    with pytest.raises(ValueError, match='utterance 2: ops.f0_track: no voiced frame'):
        ops.f0_track_device(packed([ok, ok, np.zeros(6)], np.float64), [6, 6, 6], [400, 400, 400], *args)
    bad = ok.copy()
    bad[3] = np.nan
    with pytest.raises(ValueError, match='utterance 1: ops.f0_track: f0 has to be'):
        ops.f0_track_device(packed([ok, bad, np.zeros(6)], np.float64), [6, 6, 6], [400, 400, 400], *args)
    info = torch.zeros(3, dtype=torch.int32).cuda()
    track, _, oo = ops.f0_track_device(packed([ok, -ok, ok]), [6, 6, 6], [400, 400, 400], *args, info=info)     # deferred: no read-back
    assert info.cpu().tolist() == [0, 4, 0] and (track.cpu().numpy().reshape(3, 6)[1] == 0).all()              # no rows for the refused one


# ---------------------------------------------------------------------------------------------------------------------------
# 2: the peak
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_wave_peak():
    from percivaltts_amd import ops
    _, wavs, _ = batch('A')
    rng = np.random.RandomState(3)
    wavs = list(wavs) + [np.zeros(0, dtype=np.float32), (0.3 + 0.1 * rng.randn(70001)).astype(np.float32), np.array([0.25], dtype=np.float32)]
    lengths = [len(w) for w in wavs]
    got = ops.wave_peak(packed(wavs), lengths)
    assert got.dtype == torch.float64 and tuple(got.shape) == (len(wavs),)
    again = ops.wave_peak(packed(wavs), lengths)
    assert got.cpu().numpy().tobytes() == again.cpu().numpy().tobytes()
    got = got.cpu().numpy()
    for b, w in enumerate(wavs):
        print('utterance {}: gpeak {!r}, numpy {!r}'.format(b, got[b], tf.global_peak(w)))
        np.testing.assert_allclose(got[b], tf.global_peak(w), rtol=1e-12, atol=0)
    assert got[5] == 0.0 and got[7] == 0.0 and got[0] > 0
    bad = wavs[2].copy()
    bad[100] = np.nan
    with pytest.raises(ValueError, match='utterance 1: wav is not a finite'):
        ops.wave_peak(packed([wavs[0], bad]), [len(wavs[0]), len(bad)])


# ---------------------------------------------------------------------------------------------------------------------------
# 3: each batched op equals its single op
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize('name', ['A', 'B'])
def test_f0_ops_equal_the_single_ops(name):
    from percivaltts_amd import ops
    shape, wavs, f0s = batch(name)
    fs, L = shape['fs'], shape['L']
    wav, wl = packed(wavs), [len(w) for w in wavs]
    fl = [frame_count(n, fs) for n in wl]
    assert fl == [ops.f0_frame_count(n, SHIFT, fs) for n in wl]
    gpeak = ops.wave_peak(wav, wl)
    out = ops.f0_candidates_batch(wav, wl, fl, SHIFT, fs, L, F0_MIN, F0_MAX, gpeak, want_r=True)
    f0, path = ops.f0_viterbi_batch(out[0], out[1], out[2], fl, SHIFT, want_path=True)
    est, fo, gp = ops.f0_estimate_batch(wav, wl, SHIFT, fs, L, F0_MIN, F0_MAX, want_gpeak=True)
    assert fo.lengths == fl and gp.cpu().numpy().tobytes() == gpeak.cpu().numpy().tobytes()
    np.testing.assert_array_equal(est.cpu().numpy(), f0.cpu().numpy())
    got = [split(t, fl) for t in out] + [split(f0, fl), split(path, fl)]
    voiced = 0
    for b, w in enumerate(wavs):
        single = ops.f0_candidates(_dev(w), fl[b], SHIFT, fs, L, F0_MIN, F0_MAX, float(gpeak[b].item()), want_r=True)
        for k, what in enumerate(('freq', 'strength', 'n', 'lag', 'r')):
            np.testing.assert_array_equal(got[k][b], single[k].cpu().numpy(), err_msg='{} of utterance {}'.format(what, b))
        sf0, spath = ops.f0_viterbi(single[0], single[1], single[2], SHIFT, want_path=True)
        np.testing.assert_array_equal(got[5][b], sf0.cpu().numpy(), err_msg='f0 of utterance {}'.format(b))
        np.testing.assert_array_equal(got[6][b], spath.cpu().numpy())
        # the single path measures the peak with torch: the same voicing pattern, the voiced values within 1e-6
        own = ops.f0_estimate(w, SHIFT, fs, L, F0_MIN, F0_MAX)
        np.testing.assert_array_equal(got[5][b] > 0, own > 0)
        np.testing.assert_allclose(got[5][b], own, rtol=1e-6)
        voiced += int((own > 0).sum())
    assert voiced > 50 if name == 'A' else voiced > 5
    # the refinement, of the given tracks (their own lengths: the frames beyond a waveform are kept as they are)
    tl = [len(f) for f in f0s]
    ref, status = ops.f0_refine_batch(wav, wl, packed(f0s), tl, SHIFT, fs, F0_MIN, F0_MAX, want_status=True)
    seen = set()
    for b, (w, f) in enumerate(zip(wavs, f0s)):
        o, s = ops.f0_refine(w, f, SHIFT, fs, F0_MIN, F0_MAX, want_status=True)
        np.testing.assert_array_equal(split(ref, tl)[b], o, err_msg='refined track of utterance {}'.format(b))
        np.testing.assert_array_equal(split(status, tl)[b], s)
        seen |= set(s.tolist())
    assert seen >= ({0, 1, 2} if name == 'A' else {0, 1})


@pytest.mark.gpu
@pytest.mark.parametrize('name', ['A', 'B'])
def test_frame_ops_equal_the_single_ops(name):
    from percivaltts_amd import ops
    shape, wavs, f0s = batch(name)
    fs, L = shape['fs'], shape['L']
    tracks = host_tracks(shape, wavs, f0s)
    wav, wl, fl = packed(wavs), [len(w) for w in wavs], [len(t) for t in tracks]
    f0 = packed(tracks)
    vuv = packed([(np.asarray(f)[:len(t)] > 0).astype(np.float32) for f, t in zip(f0s, tracks)])
    rate = torch.where(vuv > 0, f0, torch.full_like(f0, ops.WORLD_UNVOICED_RATE))
    hcap = ops.analysis_check(L, fs, SHIFT, F0_MIN, F0_MAX)
    lspec, u = ops.frame_harmonics_batch(wav, wl, f0, fl, SHIFT, fs, L, hcap, log=True)
    R, nm = ops.phase_coherence_batch(u, f0, fl, SHIFT, fs, L, NB)
    env = ops.world_envelope_batch(wav, wl, rate, fl, SHIFT, fs, L, log=True)
    aper = ops.world_aperiodicity_batch(wav, wl, f0, vuv, fl, SHIFT, fs, L, NB)
    got = {k: split(t, fl) for k, t in (('lspec', lspec), ('u', u), ('R', R), ('nm', nm), ('env', env), ('aper', aper))}
    for b, w in enumerate(wavs):
        wb, fb = _dev(w), _dev(tracks[b])
        vb = _dev((np.asarray(f0s[b])[:fl[b]] > 0).astype(np.float32))
        rb = torch.where(vb > 0, fb, torch.full_like(fb, ops.WORLD_UNVOICED_RATE))
        sl, su = ops.frame_harmonics(wb, fb, SHIFT, fs, L, hcap, log=True)
        sR, snm = ops.phase_coherence(su, fb, SHIFT, fs, L, NB)
        want = dict(lspec=sl, u=su, R=sR, nm=snm, env=ops.world_envelope(wb, rb, SHIFT, fs, L, log=True),
                    aper=ops.world_aperiodicity(wb, fb, vb, SHIFT, fs, L, NB))
        for k in want:
            np.testing.assert_array_equal(got[k][b], want[k].cpu().numpy(), err_msg='{} of utterance {}'.format(k, b))
            assert np.isfinite(got[k][b]).all()
    assert (aper.cpu().numpy() < -1.0).any()
    if name == 'A':
        # the coherence at an utterance's ends: utterance 2 has neighbours on both sides (utterance 1 is a single frame, utterance
        # 3 follows).  Its first and last J = 2 frames equal the single op's (above) and differ from what the whole packing gives
        # as ONE utterance, where their neighbourhoods reach into the neighbours' rows: the check above is not vacuous.
        whole, _ = ops.phase_coherence(u, f0, SHIFT, fs, L, NB)
        lo, hi = sum(fl[:2]), sum(fl[:3])
        for i in (lo, lo + 1, hi - 2, hi - 1):
            J = max(2, int(np.floor(1.0 / (float(f0[i].item()) * SHIFT) + 0.5)))
            assert J == 2 and not np.array_equal(R[i].cpu().numpy(), whole[i].cpu().numpy()), i
        np.testing.assert_array_equal(R[lo + 4:hi - 4].cpu().numpy(), whole[lo + 4:hi - 4].cpu().numpy())


# ---------------------------------------------------------------------------------------------------------------------------
# 4: one tie to the definition
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_a_batch_of_one_against_the_restatements():
    from percivaltts_amd import ops
    c = ta.case('A')
    lspec, u = ops.frame_harmonics_batch(_dev(c['wav']), [len(c['wav'])], _dev(c['f0']), [c['T']], SHIFT, c['fs'], c['L'], c['hcap'], log=True)
    ta.check(lspec.cpu().numpy(), c['lspec64'], c['lspec32'], 'frame_harmonics_batch ln SPEC, one utterance')
    ta.check(u.cpu().numpy(), c['u64'], c['u32'], 'frame_harmonics_batch phasors, one utterance')
    w = wa.case('A')
    env = ops.world_envelope_batch(_dev(w['wav']), [len(w['wav'])], _dev(w['rate']), [w['T']], SHIFT, w['fs'], w['L'], log=True)
    wa.check(env.cpu().numpy(), w['lspec64'], w['lspec32'], 'world_envelope_batch ln SPEC, one utterance')


# ---------------------------------------------------------------------------------------------------------------------------
# 5: the vocoders
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize('refine', [False, True])
@pytest.mark.parametrize('spec_type', ['fwbnd', 'mcep'])
@pytest.mark.parametrize('kind', ['PML', 'WORLD'])
def test_analysis_device_batch_equals_the_loop(kind, spec_type, refine):
    shape, wavs, f0s = batch('A')
    voc = vocoder(kind, shape, spec_type)
    with voc.f0_refine_as(refine):
        want = [voc.analysis_device(w, f, F0_MIN, F0_MAX) for w, f in zip(wavs, f0s)]
        got = voc.analysis_device_batch(wavs, f0s, F0_MIN, F0_MAX)
        assert len(got) == len(want) and [g.shape[0] for g in got] == [120, 1, 40, len(f0s[3]), len(f0s[4])]
        for b, (g, w) in enumerate(zip(got, want)):
            assert g.dtype == np.float32 and g.shape == w.shape == (w.shape[0], voc.featuressizeraw()) and np.isfinite(g).all()
            np.testing.assert_array_equal(g, w, err_msg='utterance {}'.format(b))
        # float64 tracks, as a caller may give them
        for g, w in zip(voc.analysis_device_batch(wavs[2:4], [f.astype(np.float64) + 1e-9 for f in f0s[2:4]], F0_MIN, F0_MAX),
                        [voc.analysis_device(w, f.astype(np.float64) + 1e-9, F0_MIN, F0_MAX) for w, f in zip(wavs[2:4], f0s[2:4])]):
            np.testing.assert_array_equal(g, w)
        # the tracks estimated: against the single path given the batch's own track, and against the single path's own estimate
        # (without the utterance of ten samples: its one frame is unvoiced, which both paths refuse)
        wavs = [wavs[b] for b in ESTIMATED]
        got, est = voc.analysis_device_batch(wavs, None, F0_MIN, F0_MAX, want_f0=True)
        for b, (g, f, w) in enumerate(zip(got, est, wavs)):
            assert f.dtype == np.float32 and f.shape == (g.shape[0],)
            np.testing.assert_array_equal(g, voc.analysis_device(w, f, F0_MIN, F0_MAX), err_msg='utterance {}'.format(b))
            own = voc.f0_estimate_device(w, F0_MIN, F0_MAX)
            np.testing.assert_array_equal(f > 0, own > 0)
            np.testing.assert_allclose(f, own, rtol=1e-6)
        assert (est[0] > 0).sum() > 50 and (est[0] == 0).sum() > 20


@pytest.mark.gpu
@pytest.mark.parametrize('kind', ['PML', 'WORLD'])
def test_analysis_device_batch_at_shape_b(kind):
    shape, wavs, f0s = batch('B')
    voc = vocoder(kind, shape)
    with voc.f0_refine_as(True):
        want = [voc.analysis_device(w, f, F0_MIN, F0_MAX) for w, f in zip(wavs, f0s)]
        for g, w in zip(voc.analysis_device_batch(wavs, f0s, F0_MIN, F0_MAX), want):
            np.testing.assert_array_equal(g, w)
        got, est = voc.analysis_device_batch(wavs, None, F0_MIN, F0_MAX, want_f0=True)
        for g, f, w in zip(got, est, wavs):
            np.testing.assert_array_equal(g, voc.analysis_device(w, f, F0_MIN, F0_MAX))


@pytest.mark.gpu
@pytest.mark.parametrize('kind', ['PML', 'WORLD'])
def test_an_utterance_without_a_voiced_frame_refuses_the_batch(kind):
    shape, wavs, f0s = batch('A')
    voc = vocoder(kind, shape)
    with pytest.raises(ValueError, match='utterance 2: ops.f0_track: no voiced frame'):
        voc.analysis_device_batch(wavs[2:5], [f0s[2], f0s[3], np.zeros_like(f0s[4])], F0_MIN, F0_MAX)
    with pytest.raises(ValueError, match='ops.f0_track: no voiced frame'):                # the wording of the single path
        voc.analysis_device(wavs[4], np.zeros_like(f0s[4]), F0_MIN, F0_MAX)
    with pytest.raises(ValueError, match='utterance 1: ops.f0_track: no voiced frame'):    # silence, the track estimated
        voc.analysis_device_batch([wavs[2], np.zeros(500), wavs[4]], None, F0_MIN, F0_MAX)


# ---------------------------------------------------------------------------------------------------------------------------
# 6: one launch per kernel and batch
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize('kind', ['PML', 'WORLD'])
def test_one_launch_per_kernel_and_batch(kind):
    from percivaltts_amd import _hip
    shape, wavs, f0s = batch('A')
    voc = vocoder(kind, shape)
    frames = (['ptts_frame_harmonics_batch', 'ptts_phase_coherence_batch'] if kind == 'PML'
              else ['ptts_world_envelope_batch', 'ptts_world_aperiodicity_batch'])
    with voc.f0_refine_as(True):
        own = [wavs[b] for b in ESTIMATED] + [wavs[0][:777]]
        assert len(own) == len(wavs) == 5
        voc.analysis_device_batch(own, None, F0_MIN, F0_MAX)            # the tables of the band axis are built at a first call
        with _hip.KernelTimer() as kt:
            voc.analysis_device_batch(own, None, F0_MIN, F0_MAX)
        names = [r[0] for r in kt.records]
        assert sorted(names) == sorted(['ptts_wave_peak', 'ptts_f0_candidates_batch', 'ptts_f0_viterbi_batch', 'ptts_f0_refine_batch',
                                        'ptts_f0_track', 'ptts_fwbnd_compress'] + frames), names
        with _hip.KernelTimer() as kt:
            voc.analysis_device_batch(wavs, f0s, F0_MIN, F0_MAX)
        names = [r[0] for r in kt.records]
        assert sorted(names) == sorted(['ptts_f0_refine_batch', 'ptts_f0_track', 'ptts_fwbnd_compress'] + frames), names


# ---------------------------------------------------------------------------------------------------------------------------
# 8: features_extraction writes the same files for every batch_size
# ---------------------------------------------------------------------------------------------------------------------------
def _files(root):
    out = {}
    for d, _, names in os.walk(root):
        for n in names:
            with open(os.path.join(d, n), 'rb') as f:
                out[os.path.relpath(os.path.join(d, n), root)] = f.read()
    return out


@pytest.mark.gpu
@pytest.mark.parametrize('kind', ['PML', 'WORLD'])
def test_features_extraction_writes_the_same_files_for_every_batch_size(kind, tmp_path, monkeypatch):
    """Five generated wave files, one of them at half the vocoder's rate (it takes the preprocwav route inside the batch), the tracks
    estimated: the raw streams of batch_size 1, 2 and 5 are the bytes of batch_size None."""
    import importlib
    from percivaltts_amd import vocoders
    monkeypatch.setenv('PERCIVAL_CORPUS', str(tmp_path / 'corpus'))
    monkeypatch.chdir(tmp_path)
    import percivaltts_amd.run as run
    run = importlib.reload(run)
    try:
        fs = 8000
        voc = run.vocoder = vocoder(kind)
        fids, lens = ['utt_{}'.format(i) for i in range(5)], [31, 24, 40, 17, 28]
        os.makedirs(str(tmp_path / 'corpus' / 'wav'))
        rng = np.random.RandomState(11)
        for i, (fid, T) in enumerate(zip(fids, lens)):
            rate = fs // 2 if i == 3 else fs
            N = int(round(SHIFT * (T - 1) * rate))
            f0 = 170.0 + 40.0 * np.sin(np.arange(T) / 5.0 + rng.rand())
            phase = 2 * np.pi * np.cumsum(np.interp(np.arange(N) / float(rate), SHIFT * np.arange(T), f0)) / rate
            wav = 0.1 * sum(np.cos(h * phase) / h for h in range(1, 9)) + 0.01 * rng.randn(N)
            wav[:N // 5] *= 0.0 if i == 1 else 1.0             # a silent start: unvoiced frames
            vocoders.wavwrite(str(tmp_path / 'corpus' / 'wav' / (fid + '.wav')), wav, rate)
        streams = {}
        for k in (None, 1, 2, 5):
            base = str(tmp_path / ('raw_{}'.format(k)))
            rawpaths = [base + '/f0/*.lf0', base + '/spec/*.spec', base + '/noise/*.noise'] + ([base + '/vuv/*.vuv'] if kind == 'WORLD' else [])
            assert run._extract_raw_streams(None, None, rawpaths, fids, F0_MIN, F0_MAX, None, batch_size=k) == rawpaths
            streams[k] = _files(base)
        assert len(streams[None]) == 5 * (4 if kind == 'WORLD' else 3) and all(len(v) > 0 for v in streams[None].values())
        lf0 = np.frombuffer(streams[None]['f0/utt_3.lf0'], dtype=np.float32)
        assert lf0.size in (17, 18) and np.isfinite(lf0).all()
        for k in (1, 2, 5):
            assert streams[k] == streams[None], k
    finally:
        importlib.reload(run)


# ---------------------------------------------------------------------------------------------------------------------------
# the entry points' own checks: nothing to do is no launch, the frame cap is per utterance
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_entry_points_without_work_and_with_bad_arguments():
    from percivaltts_amd import _hip, ops
    l = _hip.lib()
    cand = (8, SHIFT, 8000.0, 512, F0_MIN, F0_MAX, None, tf.VOICING_THRESHOLD, tf.SILENCE_THRESHOLD, tf.OCTAVE_COST, None)
    vit = (SHIFT, tf.OCTAVE_JUMP_COST, tf.VOICED_UNVOICED_COST, None)
    assert l.ptts_wave_peak(None, None, 0, 0, None, None, None) == 0
    assert l.ptts_wave_peak(None, None, 0, 3, None, None, None) != 0                        # null tensors
    assert l.ptts_wave_peak(None, None, 0, 65536, None, None, None) != 0
    assert l.ptts_f0_track(None, 0, None, 0, None, 0, 0, None, None, None, F0_MIN, F0_MAX, None) == 0
    assert l.ptts_f0_track(None, 0, None, 0, None, 0, 0, None, None, None, F0_MAX, F0_MIN, None) != 0
    assert l.ptts_f0_track(None, 0, None, 3, None, 4, 0, None, None, None, F0_MIN, F0_MAX, None) != 0       # more rows out than in
    assert l.ptts_f0_candidates_batch(None, None, 0, None, 0, 0, None, 0, None, None, None, None, None, *cand) == 0
    assert l.ptts_f0_candidates_batch(None, None, 0, None, 2, 5, None, 0, None, None, None, None, None, *cand) != 0
    assert l.ptts_f0_candidates_batch(None, None, 0, None, 0, 0, None, 0, None, None, None, None, None, 17, *cand[1:]) != 0
    assert l.ptts_f0_viterbi_batch(None, None, None, None, None, None, 0, 0, 0, 8, *vit) == 0
    assert l.ptts_f0_viterbi_batch(None, None, None, None, None, None, 2, 2 * tf.MAX_FRAMES, tf.MAX_FRAMES + 1, 8, *vit) != 0
    assert l.ptts_f0_viterbi_batch(None, None, None, None, None, None, 2, 10, tf.MAX_FRAMES // 2 + 1, 9, *vit) != 0
    assert l.ptts_f0_refine_batch(None, None, 0, None, 0, 0, None, None, None, SHIFT, 8000.0, F0_MIN, F0_MAX, None) == 0
    assert l.ptts_f0_refine_batch(None, None, 0, None, 0, 0, None, None, None, SHIFT, 48000.0, 8.78, F0_MAX, None) != 0
    assert l.ptts_frame_harmonics_batch(None, None, 0, None, 0, 0, None, None, None, 38, SHIFT, 8000.0, 512, 1, None) == 0
    assert l.ptts_frame_harmonics_batch(None, None, 0, None, 0, 0, None, None, None, 38, SHIFT, 8000.0, 500, 1, None) != 0
    assert l.ptts_phase_coherence_batch(None, None, None, None, None, 0, 0, 38, NB, SHIFT, 8000.0, 512, None, 0, None, 0, None) == 0
    assert l.ptts_phase_coherence_batch(None, None, None, None, None, 0, 0, 38, 1, SHIFT, 8000.0, 512, None, 0, None, 0, None) != 0
    assert l.ptts_world_envelope_batch(None, None, 0, None, 0, 0, None, None, SHIFT, 8000.0, 512, 1, None) == 0
    assert l.ptts_world_envelope_batch(None, None, 0, None, 1, 1, None, None, SHIFT, 8000.0, 512, 1, None) != 0
    assert l.ptts_world_aperiodicity_batch(None, None, 0, None, 0, 0, None, None, None, NB, SHIFT, 8000.0, 512, None, 0, None) == 0
    assert l.ptts_world_aperiodicity_batch(None, None, 0, None, 0, 0, None, None, None, 1, SHIFT, 8000.0, 512, None, 0, None) != 0
    # the cap of the path finder holds for each utterance: two utterances that together exceed it pass, one that exceeds it does not
    with pytest.raises(ValueError, match='one utterance takes at most'):
        ops.f0_viterbi_batch(torch.zeros((tf.MAX_FRAMES + 1, 8)).cuda(), torch.zeros((tf.MAX_FRAMES + 1, 8)).cuda(),
                             torch.zeros(tf.MAX_FRAMES + 1, dtype=torch.int32).cuda(), [tf.MAX_FRAMES + 1], SHIFT)
    T = tf.MAX_FRAMES // 2 + 100
    freq, strength, n = tf.random_table(200, 8, seed=4)
    rep = lambda a, dtype: torch.tensor(np.concatenate([np.resize(np.asarray(a), (T,) + np.asarray(a).shape[1:])] * 2), dtype=dtype).cuda()
    f0 = ops.f0_viterbi_batch(rep(freq, torch.float32), rep(strength, torch.float32), rep(n, torch.int32), [T, T], SHIFT)
    one = ops.f0_viterbi(rep(freq, torch.float32)[:T].contiguous(), rep(strength, torch.float32)[:T].contiguous(),
                         rep(n, torch.int32)[:T].contiguous(), SHIFT)
    assert 2 * T > tf.MAX_FRAMES and tuple(f0.shape) == (2 * T,)
    np.testing.assert_array_equal(f0[:T].cpu().numpy(), one.cpu().numpy())
    np.testing.assert_array_equal(f0[T:].cpu().numpy(), one.cpu().numpy())
