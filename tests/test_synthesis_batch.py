"""Both waveform synthesisers over a batch of utterances (ops.pulse_synthesis_batch / ops.world_synthesis_batch on the table of
ops.pulse_table_device, VocoderPML / VocoderWORLDDevice.synthesis_device_batch, ModelTTS.generate_params(wavdir=)): a batch gives,
byte for byte, what the per-utterance path gives for each of its utterances, in one launch per kernel.

Equality, not a tolerance: the table is the host's bit for bit (tests/test_pulsetable.py), a segment is computed by the same
kernel from the same rows, and a sample sums the same segments in the same order.  One comparison against the fp64 restatement
of tests/test_pulsesynth.py, with its bound, ties the batched path to the definition as well."""
import os

import numpy as np
import pytest
import torch

import test_pulsesynth as tp
import test_worldsynth as tw
from test_pulsesynth import SHIFT, wavlen_of
from test_pulsetable import A, B, BATCHES, batch_inputs

pytestmark = pytest.mark.gpu
NB, NS, NA = tp.NB, tw.NS, tw.NA


def _dev(a, dtype=torch.float32):
    return torch.tensor(np.asarray(a), dtype=dtype).cuda().contiguous()


def utterances(name, world):
    """Per utterance of the batch `name`: the inputs of tests/test_pulsesynth.py or tests/test_worldsynth.py with a seeded f0 (and
    voicing) of its own."""
    shape, lengths = BATCHES[name]
    f0s, voiceds = batch_inputs(lengths, seed=11 if name == 'A' else 13)
    out = []
    for b, T in enumerate(lengths):
        if world:
            c = tw.make_inputs(name, voiced=voiceds[b], seed=100 + b)
        else:
            c = tp.make_inputs(name, T=T, seed=100 + b)
        c['f0'] = f0s[b]
        out.append(c)
    return shape, lengths, out


def batch_synthesis(shape, cs, world, packed_noise=False):
    from percivaltts_amd import ops
    f0 = _dev(np.concatenate([c['f0'] for c in cs]))
    voiced = torch.from_numpy(np.concatenate([c['voiced'] for c in cs])).cuda() if world else None
    table = ops.pulse_table_device(f0, [c['T'] for c in cs], SHIFT, shape['fs'], shape['L'], voiced=voiced)
    spec = _dev(np.concatenate([c['spec'] for c in cs]))
    rows = _dev(np.concatenate([c['aper' if world else 'mask'] for c in cs]))
    noise = [_dev(c['g']) for c in cs]
    if packed_noise:
        noise = torch.cat(noise)
    fn = ops.world_synthesis_batch if world else ops.pulse_synthesis_batch
    wavs = fn(spec, rows, table, noise, shape['fs'], shape['L'])
    assert len(wavs) == len(cs)
    for w, c in zip(wavs, cs):
        assert w.dtype == torch.float32 and w.is_cuda and tuple(w.shape) == (c['wavlen'],)
    return [w.cpu().numpy() for w in wavs]


def single_synthesis(shape, c, world):
    from percivaltts_amd import ops
    if world:
        tab = ops.world_pulse_table(c['f0'], c['voiced'], SHIFT, shape['fs'], c['wavlen'], shape['L'])
        return ops.world_synthesis(_dev(c['spec']), _dev(c['aper']), tab, _dev(c['g']), shape['fs'], shape['L'], c['wavlen']).cpu().numpy()
    tab = ops.pulse_table(c['f0'], SHIFT, shape['fs'], c['wavlen'], shape['L'])
    return ops.pulse_synthesis(_dev(c['spec']), _dev(c['mask']), tab, _dev(c['g']), shape['fs'], shape['L'], c['wavlen']).cpu().numpy()


# ---------------------------------------------------------------------------------------------------------------------------
# 4: the batched ops equal the per-utterance ops
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('world', [False, True])
@pytest.mark.parametrize('name', ['A', 'B'])
def test_batched_synthesis_equals_the_per_utterance_ops(name, world):
    shape, lengths, cs = utterances(name, world)
    got = batch_synthesis(shape, cs, world)
    for b, c in enumerate(cs):
        want = single_synthesis(shape, c, world)
        np.testing.assert_array_equal(got[b], want, err_msg='utterance {}'.format(b))
        assert want.size == 0 or np.abs(want).max() > 0
    if name == 'A':
        assert got[1].shape == (0,)                             # T = 1
        again = batch_synthesis(shape, cs, world, packed_noise=True)           # one packed noise tensor
        for a, g in zip(again, got):
            np.testing.assert_array_equal(a, g)


def test_a_batch_of_one_against_the_restatement():
    c = tp.case('A')
    got = batch_synthesis(A, [c], world=False)[0]
    assert np.abs(c['wav64']).max() > 1e-3
    tp.check(got, c['wav64'], c['wav32'], 'pulse_synthesis_batch A, one utterance')
    w = tw.case('A')
    tw.check(batch_synthesis(A, [w], world=True)[0], w['wav64'], w['wav32'], 'world_synthesis_batch A, one utterance')


def test_an_utterance_of_one_frame_alone_and_argument_checks():
    from percivaltts_amd import _hip, ops
    one = tp.make_inputs('A', T=1)
    table = ops.pulse_table_device(_dev(one['f0']), [1], SHIFT, A['fs'], A['L'])
    with _hip.KernelTimer() as kt:
        wavs = ops.pulse_synthesis_batch(_dev(one['spec']), _dev(one['mask']), table, [_dev(one['g'])], A['fs'], A['L'])
    assert len(wavs) == 1 and tuple(wavs[0].shape) == (0,) and kt.records == []
    c = tp.case('A')
    spec, mask, g = _dev(c['spec']), _dev(c['mask']), _dev(c['g'])
    table = ops.pulse_table_device(_dev(c['f0']), [c['T']], SHIFT, A['fs'], A['L'])
    wtable = ops.pulse_table_device(_dev(c['f0']), [c['T']], SHIFT, A['fs'], A['L'], voiced=torch.ones(c['T'], dtype=torch.bool).cuda())
    with pytest.raises(_hip.HipLibraryError):
        ops.pulse_synthesis_batch(spec.cpu(), mask, table, [g], A['fs'], A['L'])
    with pytest.raises(_hip.HipLibraryError):
        ops.pulse_table_device(_dev(c['f0']).double(), [c['T']], SHIFT, A['fs'], A['L'])
    with pytest.raises(_hip.HipLibraryError):
        ops.pulse_table_device(_dev(c['f0']), [c['T']], SHIFT, A['fs'], A['L'], voiced=torch.ones(c['T']).cuda())
    for bad in (lambda: ops.pulse_synthesis_batch(spec, mask[:, :-1].contiguous(), table, [g], A['fs'], A['L']),
                lambda: ops.pulse_synthesis_batch(spec[:-1].contiguous(), mask[:-1].contiguous(), table, [g], A['fs'], A['L']),
                lambda: ops.pulse_synthesis_batch(spec, mask, table, [g[:-1].contiguous()], A['fs'], A['L']),
                lambda: ops.pulse_synthesis_batch(spec, mask, table, [g, g], A['fs'], A['L']),
                lambda: ops.pulse_synthesis_batch(spec, mask, table, g[:-1].contiguous(), A['fs'], A['L']),
                lambda: ops.pulse_synthesis_batch(spec.clone().requires_grad_(True), mask, table, [g], A['fs'], A['L']),
                lambda: ops.pulse_synthesis_batch(spec, mask, table, [g], A['fs'], 2 * A['L']),
                lambda: ops.pulse_synthesis_batch(spec, mask, wtable, [g], A['fs'], A['L']),
                lambda: ops.world_synthesis_batch(spec, mask, table, [g], A['fs'], A['L']),
                lambda: ops.pulse_table_device(_dev(c['f0']), [c['T'] - 1], SHIFT, A['fs'], A['L']),
                lambda: ops.pulse_table_device(_dev(c['f0']), [c['T']], SHIFT, A['fs'], A['L'], voiced=torch.ones(3, dtype=torch.bool).cuda())):
        with pytest.raises(ValueError):
            bad()


# ---------------------------------------------------------------------------------------------------------------------------
# 5: the vocoders
# ---------------------------------------------------------------------------------------------------------------------------
def vocoder_and_cmps(world, name='A'):
    from percivaltts_amd import vocoders
    shape, lengths, cs = utterances(name, world)
    if world:
        voc = vocoders.VocoderWORLDDevice(shape['fs'], SHIFT, NS, NA, dftlen=shape['L'])
        CMPs = [tw._cmp_of(c, voc) for c in cs]
    else:
        voc = vocoders.VocoderPML(shape['fs'], SHIFT, 12, NB, dftlen=shape['L'])
        CMPs = [tp._cmp_of(c, voc) for c in cs]
    return voc, CMPs, cs


@pytest.mark.parametrize('pp_mcep', [False, True])
@pytest.mark.parametrize('world', [False, True])
def test_synthesis_device_batch_equals_the_loop(world, pp_mcep):
    voc, CMPs, cs = vocoder_and_cmps(world)
    noise = [_dev(c['g']) for c in cs]
    want = [voc.synthesis_device(c, pp_mcep=pp_mcep, noise=n) for c, n in zip(CMPs, noise)]
    got = voc.synthesis_device_batch(CMPs, pp_mcep=pp_mcep, noise=noise)
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert g.dtype == np.float32 and g.shape == w.shape
        np.testing.assert_array_equal(g, w)
    assert max(np.abs(w).max() for w in want if w.size) > 0
    if not pp_mcep:                                             # device tensors in, and a mixture of the two
        for form in ([_dev(c) for c in CMPs], [_dev(c) if i % 2 else c for i, c in enumerate(CMPs)]):
            for g, w in zip(voc.synthesis_device_batch(form, noise=noise), want):
                np.testing.assert_array_equal(g, w)
    else:                                                       # the post-filter does something
        plain = voc.synthesis_device_batch(CMPs, noise=noise)
        assert any(np.abs(p - g).max() > 0 for p, g in zip(plain, got) if p.size)


@pytest.mark.parametrize('world', [False, True])
def test_synthesis_device_batch_follows_the_seed_like_the_loop(world):
    from percivaltts_amd import ops
    voc, CMPs, _ = vocoder_and_cmps(world)
    CMPs = [c for c in CMPs if c.shape[0] > 1]          # the generator draws no empty tensor: T = 1 needs its noise given, in both
    assert len(CMPs) == 4
    ops.rng_seed(4321)
    want = [voc.synthesis_device(c) for c in CMPs]
    state = ops.rng_state()
    ops.rng_seed(4321)
    got = voc.synthesis_device_batch(CMPs)
    assert ops.rng_state() == state
    for g, w in zip(got, want):
        np.testing.assert_array_equal(g, w)
    ops.rng_seed(4322)
    other = voc.synthesis_device_batch(CMPs)
    assert np.abs(other[0] - got[0]).max() > 0


# ---------------------------------------------------------------------------------------------------------------------------
# 6: generate_params writes the files the per-utterance path writes
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('wins', [None, [[-0.5, 0.0, 0.5], [1.0, -2.0, 1.0]]])
def test_generate_params_writes_the_same_files(wins, tmp_path):
    from percivaltts_amd import modeltts_common, ops, vocoders
    ctx, fs, L = 19, 8000, 512
    voc = vocoders.VocoderPML(fs, SHIFT, 12, 4, dftlen=L, mlpg_wins=wins)
    mod = modeltts_common.Generic(ctx, voc, layertypes=['FC', 'BLSTM'], cfgarch=tp._small_cfg())
    rng = np.random.RandomState(0)
    nout, nraw = voc.featuressize(), voc.featuressizeraw()
    lens = [41, 23, 9]
    (tmp_path / 'lab').mkdir(); (tmp_path / 'cmp').mkdir()
    fids = ['utt_{:02d}'.format(i) for i in range(len(lens))]
    for fid, n in zip(fids, lens):
        (rng.rand(n, ctx) * 2 - 1).astype(np.float32).tofile(str(tmp_path / 'lab' / (fid + '.lab')))
    mean = (rng.randn(nout) * 0.3).astype(np.float32)
    mean[0] = np.log(170.0)                                     # log f0: keeps winlen within dftlen
    std = np.full(nout, 0.1, dtype=np.float32)
    mean.tofile(str(tmp_path / 'cmp' / 'mean4norm.dat')); std.tofile(str(tmp_path / 'cmp' / 'std4norm.dat'))
    inpath = str(tmp_path / 'lab') + '/*.lab:(-1,{})'.format(ctx)
    outpath = str(tmp_path / 'cmp') + '/*.cmp:(-1,{})'.format(nout)

    ops.rng_seed(99)
    mod.generate_params(inpath, outpath, fids, str(tmp_path / 'gen'), do_objmeas=False, batch_size=2, wavdir=str(tmp_path / 'wav'))
    ops.rng_seed(99)
    (tmp_path / 'ref').mkdir()
    for fid, n in zip(fids, lens):
        CMP = np.fromfile(str(tmp_path / 'gen' / (fid + '.cmp')), dtype=np.float32).reshape(-1, nraw)
        assert CMP.shape[0] == n
        vocoders.wavwrite(str(tmp_path / 'ref' / (fid + '.wav')), voc.synthesis_device(CMP), fs)
    for fid in fids:
        with open(str(tmp_path / 'wav' / (fid + '.wav')), 'rb') as f, open(str(tmp_path / 'ref' / (fid + '.wav')), 'rb') as g:
            got, want = f.read(), g.read()
        assert len(want) > 44 and got == want, fid


# ---------------------------------------------------------------------------------------------------------------------------
# 7: one launch per kernel and batch
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('world', [False, True])
def test_one_launch_per_kernel_and_batch(world):
    from percivaltts_amd import _hip
    voc, CMPs, cs = vocoder_and_cmps(world)
    CMPs, cs = [CMPs[0], CMPs[3], CMPs[2], CMPs[4]], [cs[0], cs[3], cs[2], cs[4]]          # four utterances, each with samples
    noise = [_dev(c['g']) for c in cs]
    voc.synthesis_device_batch(CMPs, noise=noise)               # tables of the band axis are built at a first call
    with _hip.KernelTimer() as kt:
        voc.synthesis_device_batch(CMPs, noise=noise)
    names = [r[0] for r in kt.records]
    rows, segments = ('ptts_aper_rows', 'ptts_world_segments') if world else ('ptts_noise_mask', 'ptts_pulse_segments')
    for name in ('ptts_pulse_walk', 'ptts_pulse_rows', segments, 'ptts_pulse_overlap_add_batch', rows):
        assert names.count(name) == 1, (name, names)
    assert 'ptts_pulse_overlap_add' not in names
    assert sorted(names) == sorted(['ptts_pulse_walk', 'ptts_pulse_rows', segments, 'ptts_pulse_overlap_add_batch', rows, 'ptts_fwbnd2spec']), names
