"""The pulse table on the device (csrc/pulsetable.hip; ops.pulse_table_device): it equals ops.pulse_table / ops.world_pulse_table
bit for bit, for one utterance and for a batch, and what the host refuses with a ValueError comes back as a status word.

Equality, not a tolerance: the host's table is a fixed sequence of correctly rounded fp64 operations (+, -, *, /, floor, compare)
and the kernels repeat that sequence, with numpy.interp restated as in `interp_restated` below.  The CPU tests hold that
restatement against numpy itself."""
import inspect
import math

import numpy as np
import pytest
import torch

from test_pulsesynth import SHIFT, wavlen_of
from test_worldsynth import low_onset

A = dict(fs=8000, L=512)
B = dict(fs=32000, L=4096)
C = dict(fs=8000, L=1024)                       # room for the 50-Hz window (641 samples) at shape A's rate
PML_ROWS = ('start', 'winlen', 'lb', 'rb', 'fr')
WORLD_ROWS = PML_ROWS + ('i0', 'i1', 'v')


def f0_of(T, phase=0.0, offset=0.0):
    return (170.0 + offset + 60.0 * np.sin(np.arange(T) / 7.0 + phase)).astype(np.float32)


def voiced_of(T, unvoiced):
    v = np.ones(T, dtype=bool)
    for a, b in unvoiced:
        v[a:b] = False
    return v


def host_table(f0, voiced, shape):
    from percivaltts_amd import ops
    wavlen = wavlen_of(len(f0), shape['fs'])
    if voiced is None:
        return ops.pulse_table(f0, SHIFT, shape['fs'], wavlen, shape['L'])
    return ops.world_pulse_table(f0, voiced, SHIFT, shape['fs'], wavlen, shape['L'])


def device_table(f0s, voiceds, shape, **kw):
    from percivaltts_amd import ops
    f0 = torch.from_numpy(np.concatenate(f0s).astype(np.float32)).cuda()
    voiced = None if voiceds is None else torch.from_numpy(np.concatenate(voiceds)).cuda()
    return ops.pulse_table_device(f0, [len(f) for f in f0s], SHIFT, shape['fs'], shape['L'], voiced=voiced, **kw)


def assert_tables_equal(got, want, world):
    keys = ('t', 'delay', 'f0') + (('w',) if world else ()) + (WORLD_ROWS if world else PML_ROWS)
    assert set(got) == set(keys) == set(want)
    for key in keys:
        assert got[key].dtype == want[key].dtype and got[key].shape == want[key].shape, (key, got[key].dtype, got[key].shape)
        np.testing.assert_array_equal(got[key], want[key], err_msg=key)


# ---------------------------------------------------------------------------------------------------------------------------
# CPU: the definition the kernels repeat, and the interface
# ---------------------------------------------------------------------------------------------------------------------------
def interp_restated(x, shift, f0):
    """numpy.interp(x, shift * arange(T), f0) as csrc/pulsetable.hip computes it; f0 fp64."""
    T = len(f0)
    j = min(int(x / shift), T - 1)
    while j > 0 and shift * j > x:
        j -= 1
    while j < T - 1 and shift * (j + 1) <= x:
        j += 1
    if j >= T - 1:
        return float(f0[T - 1])
    xj = shift * j
    if x == xj:
        return float(f0[j])
    slope = (float(f0[j + 1]) - float(f0[j])) / (shift * (j + 1) - xj)
    return slope * (x - xj) + float(f0[j])


def walk_restated(f0, voiced, shift, fs, wavlen):
    f0 = np.asarray(f0, dtype=np.float64)
    T = len(f0)

    def rate(x):
        if voiced is not None and not voiced[min(max(int(math.floor(x / shift + 0.5)), 0), T - 1)]:
            return 500.0
        return max(interp_restated(x, shift, f0), 50.0)
    t = [0.0]
    while t[-1] < wavlen / float(fs):
        t.append(t[-1] + 1.0 / rate(t[-1]))
    return np.array(t)


def test_interp_restatement_equals_numpy():
    rng = np.random.RandomState(7)
    for T, shift in ((40, 0.005), (1, 0.005), (2, 0.005), (333, 0.005), (57, 0.01), (24, 0.00725)):
        f0 = (170.0 + 60.0 * np.sin(np.arange(T) / 7.0) + rng.uniform(-30, 30, T)).astype(np.float32).astype(np.float64)
        times = shift * np.arange(T)
        end = shift * (T - 1)
        xs = np.concatenate([times, np.arange(0.0, end + 0.05, 0.002), rng.uniform(0.0, end + 0.03, 4000),
                             np.nextafter(times, np.inf), np.nextafter(times[1:], -np.inf)])
        for x in xs:
            assert interp_restated(float(x), shift, f0) == float(np.interp(x, times, f0)), (T, shift, x)


@pytest.mark.parametrize('shape,T,unvoiced', [(A, 40, None), (B, 24, None), (A, 3, None), (A, 40, [(0, 8), (26, 32)]),
                                              (B, 24, [(10, 16)]), (C, 40, [(0, 40)])])
def test_walk_restatement_equals_the_host_table(shape, T, unvoiced):
    f0 = f0_of(T)
    voiced = None if unvoiced is None else voiced_of(T, unvoiced)
    want = host_table(f0, voiced, shape)['t']
    np.testing.assert_array_equal(walk_restated(f0, voiced, SHIFT, shape['fs'], wavlen_of(T, shape['fs'])), want)


def test_cap():
    from percivaltts_amd import ops
    assert ops.PULSE_F0_CAP == 1000.0
    assert ops.pulse_table_cap(1, 0.005) == 2
    assert ops.pulse_table_cap(1000, 0.005) == int(math.ceil(0.005 * 999 * 1000.0)) + 2 == 4997
    assert ops.pulse_table_cap(41, 0.005, f0_cap=300.0) == int(math.ceil(0.005 * 40 * 500.0)) + 2 == 102       # the unvoiced rate
    assert ops.pulse_table_cap(41, 0.01, f0_cap=2000.0) == 802
    for bad in ((0, 0.005, 1000.0), (10, 0.0, 1000.0), (10, 0.005, 0.0), (2.5, 0.005, 1000.0)):
        with pytest.raises(ValueError):
            ops.pulse_table_cap(*bad)


def test_signatures_and_argument_errors_without_a_device():
    from percivaltts_amd import ops, ops_offline, vocoders
    assert list(inspect.signature(ops.pulse_table_device).parameters) == ['f0', 'lengths', 'shift', 'fs', 'dftlen', 'voiced', 'f0_cap']
    assert inspect.signature(ops.pulse_table_device).parameters['voiced'].default is None
    assert inspect.signature(ops.pulse_table_device).parameters['f0_cap'].default == 1000.0
    assert list(inspect.signature(ops.pulse_synthesis_batch).parameters) == ['spec', 'mask', 'table', 'noise', 'fs', 'dftlen']
    assert list(inspect.signature(ops.world_synthesis_batch).parameters) == ['spec', 'aper', 'table', 'noise', 'fs', 'dftlen']
    for name in ('pulse_table_device', 'pulse_synthesis_batch', 'world_synthesis_batch', 'pulse_table_cap', 'PulseTableDevice'):
        assert name in ops_offline.__all__ and getattr(ops, name) is getattr(ops_offline, name)
    for cls in (vocoders.VocoderPML, vocoders.VocoderWORLDDevice):
        assert list(inspect.signature(cls.synthesis_device_batch).parameters) == ['self', 'CMPs', 'pp_mcep', 'noise']
    assert not hasattr(vocoders.VocoderWORLD, 'synthesis_device_batch')
    f0 = torch.zeros(10)
    for lengths, shift, fs, L, cap in (([], SHIFT, 8000, 512, 1000.0), ([10, 0], SHIFT, 8000, 512, 1000.0), (None, SHIFT, 8000, 512, 1000.0),
                                       ([10], SHIFT, 8000, 500, 1000.0), ([10], 0.0, 8000, 512, 1000.0), ([10], SHIFT, 8000, 512, -1.0),
                                       ([10], SHIFT, 0, 512, 1000.0)):
        with pytest.raises(ValueError):
            ops.pulse_table_device(f0, lengths, shift, fs, L, f0_cap=cap)
    with pytest.raises(ValueError):
        ops.pulse_synthesis_batch(f0, f0, {'start': []}, [f0], 8000, 512)        # a host table is not a device table
    voc = vocoders.VocoderPML(8000, SHIFT, 12, 9, dftlen=512)
    ok = np.zeros((4, voc.featuressizeraw()), dtype=np.float32)
    for CMPs, noise in (([], None), ([ok[:, :-1]], None), ([ok[:0]], None), ([ok, ok], [None])):
        with pytest.raises(ValueError):
            voc.synthesis_device_batch(CMPs, noise=noise)


# ---------------------------------------------------------------------------------------------------------------------------
# GPU 1: the table of one utterance equals the host's
# ---------------------------------------------------------------------------------------------------------------------------
PML_CASES = {
    'A': (A, lambda: f0_of(40)), 'B': (B, lambda: f0_of(24)), 'T3': (A, lambda: f0_of(3)), 'T2': (A, lambda: f0_of(2)),
    'T1': (A, lambda: f0_of(1)),
    'const100': (C, lambda: np.full(40, 100.0, dtype=np.float32)), 'const40': (C, lambda: np.full(40, 40.0, dtype=np.float32)),
}


@pytest.mark.gpu
@pytest.mark.parametrize('name', sorted(PML_CASES))
def test_pml_table_equals_the_host_table(name):
    shape, make = PML_CASES[name]
    f0 = make()
    want = host_table(f0, None, shape)
    tab = device_table([f0], None, shape)
    assert_tables_equal(tab.rows(0), want, world=False)
    assert tab.P == len(want['t']) and tab.W == want['winlen'].max() and not tab.world
    if name == 'A':                                             # windows cropped at both ends
        assert (want['start'] < 0).any() and (want['start'] + want['winlen'] > wavlen_of(40, A['fs'])).any()
    if name == 'T3':
        assert tab.P == 3
    if name == 'const40':
        np.testing.assert_array_equal(tab.rows(0)['f0'], 50.0)


def _world_cases():
    fs, L, T, f0, voiced, _ = low_onset()
    return {
        'A': (A, f0_of(40), voiced_of(40, [(0, 8), (26, 32)])), 'B': (B, f0_of(24), voiced_of(24, [(10, 16)])),
        'voiced': (A, f0_of(40), voiced_of(40, [])), 'unvoiced': (A, f0_of(40), voiced_of(40, [(0, 40)])),
        'low_onset': (dict(fs=fs, L=L), f0.astype(np.float32), voiced), 'T1': (A, f0_of(1), voiced_of(1, [(0, 1)])),
    }


@pytest.mark.gpu
@pytest.mark.parametrize('name', ['A', 'B', 'voiced', 'unvoiced', 'low_onset', 'T1'])
def test_world_table_equals_the_host_table(name):
    shape, f0, voiced = _world_cases()[name]
    want = host_table(f0, voiced, shape)
    tab = device_table([f0], [voiced], shape)
    got = tab.rows(0)
    assert_tables_equal(got, want, world=True)
    assert tab.world and tab.W == want['winlen'].max()
    if name == 'voiced':                                        # the PML table in the rows the two share
        pml = device_table([f0], None, shape).rows(0)
        for key in ('t', 'delay', 'f0') + PML_ROWS:
            np.testing.assert_array_equal(got[key], pml[key], err_msg=key)
    if name == 'unvoiced':
        np.testing.assert_array_equal(got['f0'], 500.0)
    if name == 'low_onset':
        assert got['winlen'].max() == 493 and got['winlen'].min() == 401
    # uint8 in place of bool
    again = device_table([f0], [voiced.astype(np.uint8)], shape).rows(0)
    assert_tables_equal(again, want, world=True)


@pytest.mark.gpu
def test_a_track_longer_than_the_staged_frames():
    """More than 8192 frames: the walk reads the track in place instead of from LDS (PT_LDS_FRAMES of csrc/pulsetable.hip)."""
    T = 8192 + 9
    f0 = f0_of(T)
    voiced = (np.arange(T) // 50) % 2 == 0
    for v in (None, voiced):
        want = host_table(f0, v, A)
        got = device_table([f0], None if v is None else [v], A).rows(0)
        assert_tables_equal(got, want, world=v is not None)


# ---------------------------------------------------------------------------------------------------------------------------
# GPU 2: a batch equals its utterances
# ---------------------------------------------------------------------------------------------------------------------------
def batch_inputs(lengths, seed):
    """Seeded f0 contours around 170 + 60 sin(i/7), another one per utterance, and voiced stretches."""
    rng = np.random.RandomState(seed)
    f0s = [f0_of(T, phase=rng.uniform(0, 6.28), offset=rng.uniform(-20, 20)) for T in lengths]
    voiceds = []
    for T in lengths:
        v = np.ones(T, dtype=bool)
        a = rng.randint(0, T)
        v[a:a + max(1, T // 4)] = False
        voiceds.append(v if T > 1 else np.array([bool(rng.randint(2))]))
    return f0s, voiceds


BATCHES = {'A': (A, [40, 1, 3, 17, 2]), 'B': (B, [24, 5])}


@pytest.mark.gpu
@pytest.mark.parametrize('world', [False, True])
@pytest.mark.parametrize('name', ['A', 'B'])
def test_a_batch_equals_its_utterances(name, world):
    shape, lengths = BATCHES[name]
    f0s, voiceds = batch_inputs(lengths, seed=11 if name == 'A' else 13)
    tab = device_table(f0s, voiceds if world else None, shape)
    wants = [host_table(f0, v if world else None, shape) for f0, v in zip(f0s, voiceds)]
    for b, want in enumerate(wants):
        assert_tables_equal(tab.rows(b), want, world)
    counts = [len(w['t']) for w in wants]
    wavlens = [wavlen_of(T, shape['fs']) for T in lengths]
    assert list(tab.counts) == counts and list(tab.lengths) == lengths and list(tab.wavlens) == wavlens
    np.testing.assert_array_equal(tab.pulse_off, np.concatenate([[0], np.cumsum(counts)]))
    np.testing.assert_array_equal(tab.frame_off, np.concatenate([[0], np.cumsum(lengths)]))
    np.testing.assert_array_equal(tab.sample_off, np.concatenate([[0], np.cumsum(wavlens)]))
    np.testing.assert_array_equal(tab.pulse_off_dev.cpu().numpy(), tab.pulse_off)
    assert tab.P == sum(counts) and tab.W == max(w['winlen'].max() for w in wants)
    assert tuple(tab.itab.shape) == (8 if world else 5, tab.P) and tuple(tab.dtab.shape) == (3 if world else 2, tab.P)
    assert tuple(tab.t.shape) == (len(lengths), tab.cap) and tab.t.dtype == torch.float64
    # the packed form: the same rows, frames and samples shifted by the utterance's offsets
    rel, packed = tab.itab.cpu().numpy(), tab.itab_packed.cpu().numpy()
    for b in range(len(lengths)):
        p = slice(int(tab.pulse_off[b]), int(tab.pulse_off[b + 1]))
        for r, key in enumerate(WORLD_ROWS if world else PML_ROWS):
            shift_by = tab.sample_off[b] if key in ('start', 'lb', 'rb') else tab.frame_off[b] if key in ('fr', 'i0', 'i1') else 0
            want = rel[r, p] + shift_by
            if key == 'winlen' and wavlens[b] == 0:
                want = np.zeros_like(want)                      # no pulse work for an utterance without samples
            np.testing.assert_array_equal(packed[r, p], want, err_msg=(b, key))
    if name == 'A':                                             # T = 1: the host's one-pulse table, no samples
        assert counts[1] == 1 and wavlens[1] == 0 and tab.rows(1)['rb'][0] == 0


# ---------------------------------------------------------------------------------------------------------------------------
# GPU 3: refusals are ValueErrors that name the utterance; nothing faults and the next call works
# ---------------------------------------------------------------------------------------------------------------------------
def falling_track():
    """400 Hz, then 50 Hz from one frame to the next: while f0 falls through 80 Hz the window, and with it the lead of a pulse
    over its window, grows by more samples than the pulses are apart, so a start steps backwards.  The host's check refuses it."""
    from percivaltts_amd import ops_offline
    T = 12
    f0 = np.where(np.arange(T) < 6, 400.0, 50.0).astype(np.float32)
    table = host_table(f0, None, C)
    with pytest.raises(ValueError, match='ascend'):
        ops_offline._pulse_table_rows(table, T, C['L'], wavlen_of(T, C['fs']))
    return f0


def _refused(case):
    T = 12
    good = f0_of(T)
    if case == 'window':                                        # 4 fs / 55 = 2327 samples; 0.05 fs = 1600 fit
        return dict(fs=32000, L=2048), np.full(T, 55.0, dtype=np.float32), 'does not fit dftlen=2048', {}
    if case == 'nan':
        bad = good.copy(); bad[T - 2] = np.nan
        return A, bad, 'positive finite', {}
    if case == 'inf':
        bad = good.copy(); bad[3] = np.inf
        return A, bad, 'positive finite', {}
    if case == 'nonpositive':
        bad = good.copy(); bad[5] = 0.0
        return A, bad, 'positive finite', {}
    if case == 'negative':
        bad = good.copy(); bad[0] = -170.0
        return A, bad, 'positive finite', {}
    if case == 'rate':
        return A, np.full(T, 1200.0, dtype=np.float32), 'f0_cap', {}
    if case == 'rate_custom_cap':
        return A, good, 'f0_cap=150', dict(f0_cap=150.0)
    assert case == 'descending'
    return C, falling_track(), 'ascend', {}


# the WORLD table leads every pulse by the same number of samples, so its starts cannot descend: that case is PML's alone
REFUSALS = [(case, world) for case in ('window', 'nan', 'inf', 'nonpositive', 'negative', 'rate', 'rate_custom_cap')
            for world in (False, True)] + [('descending', False)]


@pytest.mark.gpu
@pytest.mark.parametrize('case,world', REFUSALS)
def test_refusals_name_the_utterance(case, world):
    """The issue's window case reads 'f0 = 55 at fs 32000, dftlen 1024' with the other two utterances valid; at fs 32000 no window
    fits 1024 samples (0.05 fs = 1600), so the batch with valid neighbours is at dftlen 2048 and the literal figures are tested
    below for the refusal alone."""
    shape, bad, words, kw = _refused(case)
    T = len(bad)
    if case == 'rate_custom_cap':
        ok = [np.full(T, 120.0, dtype=np.float32), np.full(T, 140.0, dtype=np.float32)]
    else:
        ok = [f0_of(T), f0_of(T, phase=1.0)]
    voiceds = [np.ones(T, dtype=bool)] * 3 if world else None
    with pytest.raises(ValueError, match='utterance 1: .*' + words):
        device_table([ok[0], bad, ok[1]], voiceds, shape, **kw)
    tab = device_table([ok[0], ok[1]], None if voiceds is None else voiceds[:2], shape, **kw)      # a following valid call
    assert_tables_equal(tab.rows(1), host_table(ok[1], None if voiceds is None else voiceds[1], shape), world)


@pytest.mark.gpu
def test_refusals_window_at_the_figures_of_the_issue_and_too_many_pulses():
    T = 12
    with pytest.raises(ValueError, match='does not fit dftlen=1024'):
        device_table([f0_of(T), np.full(T, 55.0, dtype=np.float32), f0_of(T)], None, dict(fs=32000, L=1024))
    # an unvoiced stretch at 500 pulses a second under a cap the caller set too low never happens (cap takes the larger rate);
    # a table of more than cap pulses is refused all the same: the same launch, cap passed for a shorter utterance
    from percivaltts_amd import _hip, ops
    from percivaltts_amd._hip import call, ptr, stream
    f0 = torch.from_numpy(np.full(T, 900.0, dtype=np.float32)).cuda()
    offs = torch.tensor([[0, T], [0, wavlen_of(T, 8000)]], dtype=torch.int64).cuda()
    cap = 7
    t = torch.full((1, cap + 3), -1.0, dtype=torch.float64).cuda()
    info = torch.zeros((1, 4), dtype=torch.int32).cuda()
    call('ptts_pulse_walk', ptr(f0), None, ptr(offs), 1, SHIFT, 8000.0, 512, cap, 1000.0, ptr(t), ptr(info), stream())
    count, _, status, _ = info.cpu().numpy()[0]
    assert count == cap and status == _hip._define('PTTS_PULSE_TOO_MANY')
    np.testing.assert_array_equal(t.cpu().numpy()[0, cap:], -1.0)              # nothing beyond the slots
    assert ops.pulse_table_cap(T, SHIFT) > cap
