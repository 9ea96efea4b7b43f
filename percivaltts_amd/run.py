"""Experiment script with the shape of the reference's percivaltts/run.py:57-230: a module-level `cfg`,
`build_model()`, `training(cont)`, `generate()`.  The corpus-preparation stages of the reference
split in two.  `features_extraction()` is the reference's stage of that name (run.py:147-165) with the build's own waveform
analysis (VocoderPML.analysisfid_device or VocoderWORLDAnalysisDevice.analysisfid_device) in the place of
pulsemodel's or pyworld's, the build's own F0 estimator (or a
caller's F0 tracks) in the place of the REAPER binary, and Vocoder.preprocwav (resampling, high-pass) in front of both;
`synthesize_corpus()` writes a synthetic corpus of the same on-disk
format (headerless float32 `path:(-1,D)`
files + file_id_list.scp) so that the training stages run without recordings.  `contexts_extraction()` is the reference's stage of
that name (run.py:168-180): HTS labels through the label normaliser (percivaltts_amd.external.merlin, on the device), the
time weights from the labels, and the min-max normalised inputs `cfg.inpath` points at.  `features_compose()` is the
composition half of the reference's features_extraction (run.py:155-165): from raw per-stream feature files it writes the time weights and the composed, normalised outputs `cfg.outpath` points at
(percivaltts_amd.compose, on the device).  The duration side is the build's own addition in the same shape: `durations_extraction()`
writes a duration model's corpus from state-aligned labels (phone-level inputs, the five state durations per phone as targets),
`build_duration_model()` / `training_durations()` train it with the least-squares optimiser over the phone index, and
`generate(dur_fparams=..., lab_path=..., lab_questions=...)` takes its context rows from predicted durations
(`contexts_from_durations()`), so that labels without times go through to a waveform.  `labels_alignment()` gives untimed labels
their times for TRAINING: the build's own forced alignment (flat-start Viterbi training on the device) writes the
state-aligned labels that `contexts_extraction()` and `durations_extraction()` read, where the reference's corpus came from an HTK aligner.
"""
from __future__ import print_function

import os
import sys

import numpy as np

from percivaltts_amd import *  # noqa: F401,F403  (configuration, readids, print_log, ...)
from percivaltts_amd import compose, modeltts_common, networks_critic, optimizertts, optimizertts_wgan, vocoders

print_log('Global configurations')
cfg = configuration()

# Corpus
cp = os.environ.get('PERCIVAL_CORPUS', os.path.join(os.getcwd(), 'corpus_synthetic')) + '/'
cfg.fileids = cp + 'file_id_list.scp'
cfg.id_valid_start = 40
cfg.id_valid_nb = 4
cfg.id_test_nb = 4

ctxsize = 416 + 9
cfg.inpath = cp + 'label_state_align_bin' + str(ctxsize) + '_norm_minmaxm11/*.lab:(-1,' + str(ctxsize) + ')'

cfg.vocoder_fs = 16000
cfg.vocoder_shift = 0.005
mlpg_wins = None
vocoder = vocoders.VocoderPML(cfg.vocoder_fs, cfg.vocoder_shift, spec_size=129, nm_size=33, mlpg_wins=mlpg_wins)

errtype = 'WLSWGAN'   # 'LSE', 'WGAN', 'WLSWGAN'

out_size = vocoder.featuressize()
cfg.outpath = cp + 'wav_PML_cmp_lf0_fwlspec' + str(vocoder.specsize()) + '_fwnm' + str(vocoder.noisesize()) + '_nmnoscale/*.cmp:(-1,' + str(out_size) + ')'
cfg.wpath = cp + 'label_state_align_weights/*.w:(-1,1)'

# Duration model (a build extension: durations_extraction, build_duration_model, training_durations, generate(dur_fparams=...))
dur_ctxsize = 416
dur_nstates = 5
cfg.dur_inpath = cp + 'label_phone_bin' + str(dur_ctxsize) + '_norm_minmaxm11/*.lab:(-1,' + str(dur_ctxsize) + ')'
cfg.dur_outpath = cp + 'label_state_align_dur' + str(dur_nstates) + '_norm_meanstd/*.dur:(-1,' + str(dur_nstates) + ')'
cfg.dur_wpath = cp + 'label_phone_weights/*.w:(-1,1)'
cfg.dur_fparams_fullset = 'model-dur.h5'
dur_layertypes = ['FC', 'BLSTM']

# Model architecture (run.py:114-120)
cfg.arch_hiddenwidth = 256
cfg.arch_ctx_nbcnnlayers = 1
cfg.arch_ctx_winlen = 21
cfg.arch_gen_nbcnnlayers = 8
cfg.arch_gen_nbfilters = 4
cfg.arch_gen_winlen = 5
cfg.arch_spec_freqlen = 5

# Training (run.py:122-137)
cfg.fparams_fullset = 'model.h5'
cfg.train_batch_size = 10
cfg.train_batch_lengthmax = int(2.0 / 0.005)
cfg.train_wgan_LScoef = 0.25
cfg.train_min_nbepochs = 250
cfg.train_max_nbepochs = 300
cfg.train_cancel_nodecepochs = 25
cfg.train_wgan_critic_LSWGANtransfreqcutoff = 4000
cfg.train_wgan_critic_LSWGANtranscoef = 1.0 / 8.0
cfg.train_wgan_critic_use_WGAN_incnoisefeature = False


def synthesize_corpus(nfiles=48, minlen=450, maxlen=700, seed=123):
    """Synthetic composed features: labels ~ U(-1,1), f0+spec ~ N(0,1), noise mask ~ U(0,1), weights 1 with silent ends."""
    rng = np.random.RandomState(seed)
    fids = ['syn_{:04d}'.format(i) for i in range(nfiles)]
    for path in (cfg.inpath, cfg.outpath, cfg.wpath):
        makedirs(os.path.dirname(path.split(':')[0]))
    with open(cfg.fileids, 'w') as f:
        f.write('\n'.join(fids) + '\n')
    for fid in fids:
        n = int(rng.randint(minlen, maxlen))
        (rng.rand(n, ctxsize) * 2 - 1).astype(np.float32).tofile(cfg.inpath.split(':')[0].replace('*', fid))
        y = rng.randn(n, out_size).astype(np.float32)
        y[:, 1 + vocoder.specsize():] = rng.rand(n, vocoder.noisesize())
        y.tofile(cfg.outpath.split(':')[0].replace('*', fid))
        w = np.ones((n, 1), dtype=np.float32)
        w[:20] = 0.0; w[-20:] = 0.0
        w.tofile(cfg.wpath.split(':')[0].replace('*', fid))
    # the synthetic features count as already normalised: identity statistics beside them (features_compose -> compose.compose writes the real ones)
    np.zeros(out_size, dtype=np.float32).tofile(os.path.join(os.path.dirname(cfg.outpath), 'mean4norm.dat'))
    np.ones(out_size, dtype=np.float32).tofile(os.path.join(os.path.dirname(cfg.outpath), 'std4norm.dat'))
    return fids


def features_compose(rawpaths, fids=None, win_convention='mlpg'):
    """The composition stage of the reference's features_extraction (run.py:155-165).  rawpaths: the raw feature streams in
    the vocoder's order, [f0_path, spec_path, noise_path] without shape selectors (VocoderWORLD: + vuv_path).  Writes the time
    weights from the spectral energy to cfg.wpath and the composed outputs, with `vocoder.mlpg_wins` and the statistics of the
    first cfg.id_valid_start files, to cfg.outpath.  `win_convention`: 'mlpg' by default here, because generate() inverts the
    windows with MLPG (see compose.compose); 'reference' reproduces the reference's files."""
    fids = readids(cfg.fileids) if fids is None else fids
    spec_path = rawpaths[1] + ':(-1,' + str(vocoder.specsize()) + ')'
    mcep = getattr(vocoder, 'spec_type', 'fwbnd') == 'mcep'         # the energy is in c_0 then, not in the bands' mean
    compose.create_weights_spec(spec_path, fids, cfg.wpath, spec_type='mcep' if mcep else 'fwlspec')
    outpaths = [rawpaths[0], spec_path, rawpaths[2] + ':(-1,' + str(vocoder.noisesize()) + ')'] + list(rawpaths[3:])
    normfn = compose.normalise_meanstd_nmnoscale if isinstance(vocoder, vocoders.VocoderPML) else compose.normalise_meanstd
    return compose.compose(outpaths, fids, cfg.outpath, id_valid_start=cfg.id_valid_start, normfn=normfn, wins=vocoder.mlpg_wins,
                           win_convention=win_convention)


def features_extraction(f0in_path=None, wav_path=None, rawpaths=None, fids=None, f0_min=70, f0_max=600, win_convention='mlpg',
                        f0_refine=None, batch_size=None, preproc_hp=None):
    """The reference's features_extraction (run.py:147-165): every file id's waveform `wav_path` ('dir/*.wav', by default
    <corpus>/wav/*.wav) goes through vocoder.analysisfid_device with the F0 track of `f0in_path` ('dir/*.f0': headerless float32 Hz
    values, one per frame, <= 0 unvoiced) or, with f0in_path None, the track of the build's own estimator
    (vocoder.f0_estimate_device; the reference runs REAPER here), which writes the raw
    streams `rawpaths` = [f0_path, spec_path, noise_path] (by default the reference's places beside the waveforms; for a vocoder
    with spec_type 'mcep' the spectral stream goes to <base>_mcep<N>/*.mcep and the weights come from c_0); then
    features_compose.  f0_min / f0_max default to the reference's cfg.vocoder_f0_min / cfg.vocoder_f0_max.  `preproc_hp`: the cut-off
    in Hz of the high-pass filter in front of the analysis, 'auto' for f0_min as in the reference, None for no filter.  A file
    that is not sampled at the vocoder's rate, or any file with preproc_hp, goes through vocoder.preprocwav (resampling, then the
    filter; csrc/preproc.hip) and vocoder.analysis_device; a file at the vocoder's rate without preproc_hp takes
    analysisfid_device as before.  A WORLD vocoder with an analysis (vocoders.VocoderWORLDAnalysisDevice) has four streams,
    `rawpaths` = [f0_path, spec_path, noise_path, vuv_path], by default the reference's <wavdir>_WORLD_lf0, .._fwlspec<N>,
    .._fwdbap<N>/*.fwdbap and .._vuv1/*.vuv (run.py:103-105).  `f0_refine`: True or False sets vocoder.f0_refine (the F0
    refinement in front of the analysis, vocoders.VocoderF0Spec.f0_refine_device) for the duration of the call, None leaves the
    vocoder as it is.  `batch_size`: None analyses file by file as above; k >= 1 collects up to k files (each read with wavread, and
    passed through vocoder.preprocwav under the same conditions) and analyses them with one vocoder.analysis_device_batch call,
    every kernel launching once per batch; the files written are the same bytes for every batch_size.  (It stands in front of
    preproc_hp, which callers pass by keyword and which stays the last parameter.)"""
    _check_batch_size(batch_size)
    fids = readids(cfg.fileids) if fids is None else fids
    if not hasattr(vocoder, 'analysisfid_device'):
        raise ValueError('features_extraction: {} has no waveform analysis in this build'.format(vocoder.name()))
    with vocoder.f0_refine_as(f0_refine):
        rawpaths = _extract_raw_streams(f0in_path, wav_path, rawpaths, fids, f0_min, f0_max, preproc_hp, batch_size=batch_size)
    return features_compose(rawpaths, fids=fids, win_convention=win_convention)


def _check_batch_size(batch_size):
    if batch_size is not None and (int(batch_size) != batch_size or batch_size < 1):
        raise ValueError('features_extraction: batch_size={!r} is not None or an integer >= 1'.format(batch_size))


def _extract_raw_streams(f0in_path, wav_path, rawpaths, fids, f0_min, f0_max, preproc_hp, batch_size=None):
    """The analysis loop of features_extraction: writes the raw streams of every file id and returns `rawpaths`.  With
    `batch_size` the files go through vocoder.analysis_device_batch, up to batch_size of them a call."""
    _check_batch_size(batch_size)
    wav_path = cp + 'wav/*.wav' if wav_path is None else wav_path
    world = isinstance(vocoder, vocoders.VocoderWORLD)      # four streams: the noise stream is 'fwdbap', and there is a 'vuv' one
    if rawpaths is None:
        base = os.path.dirname(wav_path) + ('_WORLD' if world else '_PML')
        noisetag = 'fwdbap' if world else 'fwnm'
        spec_raw = ('_mcep' + str(vocoder.specsize()) + '/*.mcep' if getattr(vocoder, 'spec_type', 'fwbnd') == 'mcep'
                    else '_fwlspec' + str(vocoder.specsize()) + '/*.fwlspec')
        rawpaths = [base + '_lf0/*.lf0', base + spec_raw,
                    base + '_' + noisetag + str(vocoder.noisesize()) + '/*.' + noisetag]
        if world:
            rawpaths.append(base + '_vuv1/*.vuv')
    nstreams = 4 if world else 3
    outputpathdicts = {'f0': rawpaths[0], 'spec': rawpaths[1], 'noise': rawpaths[2]}
    if world:
        outputpathdicts['vuv'] = rawpaths[3]
    if preproc_hp == 'auto':
        preproc_hp = f0_min
    if batch_size is not None:
        for first in range(0, len(fids), int(batch_size)):
            chunk = fids[first:first + int(batch_size)]
            wavs, f0s = [], []
            for fid in chunk:
                fwav = wav_path.replace('*', fid)
                print('Extracting {} features from: '.format('WORLD' if world else 'PML') + fwav)
                wav, fs = vocoders.wavread(fwav)
                if preproc_hp is not None or fs != int(round(vocoder.fs)):
                    wav = vocoder.preprocwav(wav, fs, highpass=preproc_hp)
                wavs.append(wav)
                f0s.append(None if f0in_path is None else np.fromfile(f0in_path.replace('*', fid), dtype=np.float32))
            CMPs = vocoder.analysis_device_batch(wavs, None if f0in_path is None else f0s, f0_min, f0_max)
            for fid, CMP in zip(chunk, CMPs):
                vocoder.write_streams(CMP, *[p.replace('*', fid) for p in rawpaths[:nstreams]])
        return rawpaths
    for fid in fids:
        fwav = wav_path.replace('*', fid)
        if preproc_hp is None and vocoders.wavfs(fwav) == int(round(vocoder.fs)):
            vocoder.analysisfid_device(fid, wav_path, f0in_path, f0_min, f0_max, outputpathdicts)
            continue
        print('Extracting {} features from: '.format('WORLD' if world else 'PML') + fwav)
        wav, fs = vocoders.wavread(fwav)
        wav = vocoder.preprocwav(wav, fs, highpass=preproc_hp)
        f0 = None if f0in_path is None else np.fromfile(f0in_path.replace('*', fid), dtype=np.float32)
        vocoder.write_streams(vocoder.analysis_device(wav, f0, f0_min, f0_max), *[p.replace('*', fid) for p in rawpaths[:nstreams]])
    return rawpaths


def contexts_extraction(lab_path, fids, lab_questions, labbin_path, labs_wpath, inpath, lab_type='state', id_valid_start=-1,
                        shift=0.005):
    """The reference's contexts_extraction (run.py:168-180).  lab_path: the HTS label files ('dir/*.lab'), state-aligned for
    lab_type 'state' (sub-phone features 'full'), phone-aligned for any false value or 'phone' ('coarse_coding'); fids: the file
    ids (a list, or the path of the id list); lab_questions: the HTK question file (the package ships none).  Writes the
    un-normalised context matrices to labbin_path, one weight per frame (0 over 'sil') to labs_wpath, and the inputs, min-max
    normalised to [-1, 1] from the statistics of the first `id_valid_start` files, to inpath (a ':(-1,D)' suffix on labbin_path /
    inpath is ignored).  All files go through the normaliser in one call: a chunk of utterances is two kernel launches."""
    from percivaltts_amd.external.merlin.label_normalisation import HTSLabelNormalisation
    fids = readids(fids) if isinstance(fids, str) else list(fids)
    state = bool(lab_type) and lab_type != 'phone'
    normaliser = HTSLabelNormalisation(question_file_name=lab_questions, add_frame_features=True,
                                       subphone_feats='full' if state else 'coarse_coding')
    labbin_path = labbin_path.split(':')[0]
    makedirs(os.path.dirname(labbin_path))
    normaliser.perform_normalisation([lab_path.replace('*', fid) for fid in fids], [labbin_path.replace('*', fid) for fid in fids],
                                     label_type='state_align' if state else 'phone_align')
    compose.create_weights_lab(lab_path, fids, labs_wpath, silencesymbol='sil', shift=shift)
    return compose.compose([labbin_path + ':(-1,' + str(normaliser.dimension) + ')'], fids, inpath, id_valid_start=id_valid_start,
                           normfn=compose.normalise_minmax, wins=[], do_finalcheck=False)


def phone_labels_from_state_labels(lab_path, fids, phonelab_path):
    """State-aligned HTS labels (five lines "start end label[k]", k = 2 .. 6, per phone) -> phone-aligned ones: one line
    "start end label" per phone, from the start of its first state to the end of its last, the state suffix dropped.  What a
    duration model reads, one row per line (HTSDurationLabelNormalisation)."""
    fids = readids(fids) if isinstance(fids, str) else list(fids)
    makedirs(os.path.dirname(phonelab_path))
    for fid in fids:
        with open(lab_path.replace('*', fid)) as f:
            rows = [line.split() for line in f if line.strip()]
        if len(rows) % 5 or any(len(r) != 3 for r in rows) or any([r[2][-3:] for r in rows[i:i + 5]] != ['[2]', '[3]', '[4]', '[5]', '[6]']
                                                                for i in range(0, len(rows), 5)):
            raise ValueError('{}: a state-aligned label file holds five lines "start end label[k]", k = 2 .. 6, per phone'.format(lab_path.replace('*', fid)))
        with open(phonelab_path.replace('*', fid), 'w') as f:
            f.writelines('{} {} {}\n'.format(rows[i][0], rows[i + 4][1], rows[i][2][:-3]) for i in range(0, len(rows), 5))


def durations_extraction(lab_path, fids, lab_questions, phonelab_path, labbin_path, dur_path, durs_wpath, inpath, outpath, id_valid_start=-1):
    """The corpus of a duration model from state-aligned HTS labels `lab_path` ('dir/*.lab'): phone-aligned labels to
    phonelab_path (phone_labels_from_state_labels); the phone-level inputs -- one row of question columns per phone,
    HTSDurationLabelNormalisation -- un-normalised to labbin_path and min-max normalised to [-1, 1] to inpath; the targets -- the
    five state durations of every phone in frames, HTSLabelNormalisation.prepare_dur_data -- un-normalised to dur_path and
    mean/std normalised to outpath; one weight per phone, all ones, to durs_wpath.  The statistics are those of the first
    `id_valid_start` files, written beside inpath (min4norm.dat, max4norm.dat) and outpath (mean4norm.dat, std4norm.dat) by
    compose.compose.  A ':(-1,D)' suffix on a path is ignored.  Returns the two compose results as {'in': ..., 'out': ...}."""
    from percivaltts_amd.external.merlin.label_normalisation import HTSDurationLabelNormalisation, HTSLabelNormalisation
    fids = readids(fids) if isinstance(fids, str) else list(fids)
    phonelab_path, labbin_path, dur_path, durs_wpath = (p.split(':')[0] for p in (phonelab_path, labbin_path, dur_path, durs_wpath))
    phone_labels_from_state_labels(lab_path, fids, phonelab_path)
    for p in (labbin_path, dur_path, durs_wpath):
        makedirs(os.path.dirname(p))
    each = lambda path: [path.replace('*', fid) for fid in fids]
    inputs = HTSDurationLabelNormalisation(question_file_name=lab_questions)
    inputs.perform_normalisation(each(phonelab_path), each(labbin_path))
    HTSLabelNormalisation(question_file_name=lab_questions).prepare_dur_data(each(lab_path), each(dur_path), label_type='state_align')
    for d, w in zip(each(dur_path), each(durs_wpath)):
        np.ones((os.path.getsize(d) // (4 * dur_nstates), 1), dtype=np.float32).tofile(w)
    res_in = compose.compose([labbin_path + ':(-1,' + str(inputs.dimension) + ')'], fids, inpath, id_valid_start=id_valid_start,
                             normfn=compose.normalise_minmax, wins=[], do_finalcheck=False)
    res_out = compose.compose([dur_path + ':(-1,' + str(dur_nstates) + ')'], fids, outpath, id_valid_start=id_valid_start,
                              normfn=compose.normalise_meanstd, wins=[], do_finalcheck=False)
    return {'in': res_in, 'out': res_out}


def contexts_from_durations(lab_path, fids, lab_questions, dur_path, inpath, outpath, lab_type='state', min_frames=1, batch_size=64):
    """The inputs of the acoustic model from durations instead of a forced alignment: the labels of `lab_path` (their times, if
    any, are ignored) and the duration files `dur_path` ('dir/*.dur': float32 [P,5] frames per state for lab_type 'state', [P,1]
    frames per phone for 'phone') go through HTSLabelNormalisation.normalise_with_durations, `batch_size` utterances a call, and
    the rows, still on the device, through the min-max normalisation whose statistics contexts_extraction stored beside `inpath`
    (min4norm.dat / max4norm.dat; compose.normalise_minmax_stored -- they are read, not recomputed).  Writes `outpath` ('dir/*.lab')
    and returns the number of rows of every file."""
    import torch
    from percivaltts_amd.external.merlin.label_normalisation import HTSLabelNormalisation
    fids = readids(fids) if isinstance(fids, str) else list(fids)
    state = bool(lab_type) and lab_type != 'phone'
    normaliser = HTSLabelNormalisation(question_file_name=lab_questions, add_frame_features=True,
                                       subphone_feats='full' if state else 'coarse_coding')
    dur_path, outpath, statsdir = dur_path.split(':')[0], outpath.split(':')[0], os.path.dirname(inpath.split(':')[0])
    makedirs(os.path.dirname(outpath))
    dev = compose._device()
    nbrows = []
    for first in range(0, len(fids), int(batch_size)):
        chunk = fids[first:first + int(batch_size)]
        durs = [torch.from_numpy(np.fromfile(dur_path.replace('*', fid), dtype=np.float32).reshape(-1, dur_nstates if state else 1)).to(dev)
                for fid in chunk]
        X, offs = normaliser.normalise_with_durations([lab_path.replace('*', fid) for fid in chunk], durs,
                                                      label_type='state_align' if state else 'phone_align', min_frames=min_frames)
        compose._write_rows(compose.normalise_minmax_stored(X, statsdir).cpu().numpy(), offs, outpath, chunk)
        nbrows.extend(int(n) for n in np.diff(offs))
    return nbrows


def labels_alignment(lab_path, fids, feat_path, outlab_path, cols=None, lab_type='state', n_iter=20, model_in=None, model_out=None,
                     lineheadregexp=None, var_floor=0.01, min_count=2, shift=0.005, workspace_bytes=None):
    """Timed labels from untimed ones by forced alignment (ops.forced_align_train: flat-start Viterbi training of monophone,
    five-state, left-to-right diagonal Gaussians; the build's own definition), so that a corpus of recordings
    and untimed full-context labels enters the project without an outside aligner.  lab_path: the HTS label files ('dir/*.lab'),
    one phone per line or five state lines per phone; their times, if any, are ignored (parse_phone_labels).  feat_path: the
    [T,Dx] float32 feature files the alignment is made on ('dir/*.cmp:(-1,Dx)'; the composed, normalised acoustic outputs are the
    intended input) and cols = (c0, c1) the block of columns used (None: all; the spectrum block is the intended one).  A phone's
    model is chosen by its centre-phone name, group 3 of `lineheadregexp` (compose.create_weights_lab's default).  Writes to
    outlab_path ('dir/*.lab') state-aligned labels for lab_type 'state' -- what contexts_extraction and durations_extraction read
    -- or phone-aligned ones for 'phone' (or any false value).  With model_in (an .npz of mu, var [Q,D] and the model names) the
    stored models are used, and with n_iter=0 besides they are not re-estimated: new utterances aligned with stored models; model_out
    stores the models.  A label the expression does not match, a phone without a stored model and an utterance that cannot be
    aligned (fewer frames than states, a feature that is not finite, ...) are ValueErrors naming the file.  Returns the history of
    ops.forced_align_train."""
    import torch
    from percivaltts_amd import data, ops
    from percivaltts_amd.external.merlin import label_normalisation as ln
    fids = readids(fids) if isinstance(fids, str) else list(fids)
    if float(shift) != 0.005:
        raise ValueError('labels_alignment: shift={!r}: label times are written at 50000 units per frame (0.005 s) and no other'.format(shift))
    regexp = ln.LABEL_HEAD_REGEXP if lineheadregexp is None else lineheadregexp
    feat_path, shape = data.getpathandshape(feat_path)
    if shape is None or len(shape) != 2 or shape[1] < 1:
        raise ValueError('labels_alignment: feat_path has to end with the shape of its files, ":(-1,Dx)"')
    Dx, S = shape[1], ops.LABELS_SEG_STATES
    c0, c1 = (0, Dx) if cols is None else cols
    labfiles = [lab_path.replace('*', fid) for fid in fids]
    phones, centres = [], []
    for fname in labfiles:                                  # every label is checked before the device is touched
        ph, linenos = ln.parse_phone_label_lines(fname, 'state_align')
        phones.append(ph)
        centres.append([ln.centre_phone(p, regexp, where='{}:{}'.format(fname, n)) for p, n in zip(ph, linenos)])
    stored = None
    if model_in is not None:
        with np.load(model_in, allow_pickle=False) as z:
            stored = (z['mu'], z['var'], [str(n) for n in z['names']])
        names = stored[2]
        if stored[0].shape != (len(names) * S, c1 - c0) or stored[1].shape != stored[0].shape:
            raise ValueError('{}: mu and var {} are not [{} models x {} states, {} columns]'.format(model_in, stored[0].shape, len(names), S, c1 - c0))
    else:
        names = sorted(set(c for cs in centres for c in cs))
    index = {n: i for i, n in enumerate(names)}
    chains = []
    for fname, cs in zip(labfiles, centres):
        for c in cs:
            if c not in index:
                raise ValueError('{}: the phone {!r} has no model in {}'.format(fname, c, model_in))
        chains.append((np.asarray([index[c] for c in cs], dtype=np.int64)[:, None] * S + np.arange(S)[None, :]).reshape(-1))
    feats = [data.loadfile(feat_path, fid, shape=(-1, Dx)) for fid in fids]
    dev = compose._device()
    X = torch.from_numpy(np.ascontiguousarray(np.concatenate(feats), dtype=np.float32)).to(dev)
    model = None if stored is None else ops.AlignModel.from_host(stored[0], stored[1], dev)
    model, dur, history = ops.forced_align_train(X, [f.shape[0] for f in feats], chains, len(names) * S, c0, c1, n_iter=n_iter,
                                                 var_floor=var_floor, min_count=min_count, model=model, names=labfiles,
                                                 **({} if workspace_bytes is None else {'workspace_bytes': workspace_bytes}))
    dur = dur.cpu().numpy()
    outlab_path = outlab_path.split(':')[0]
    makedirs(os.path.dirname(outlab_path))
    state = bool(lab_type) and lab_type != 'phone'
    at = 0
    for fid, ph in zip(fids, phones):
        d = dur[at:at + S * len(ph)].reshape(-1, S)
        at += S * len(ph)
        (ln.write_state_labels if state else ln.write_phone_labels)(outlab_path.replace('*', fid), ph, d, shift=shift)
    if model_out is not None:
        makedirs(os.path.dirname(os.path.abspath(model_out)))
        mu, var = model.host()
        np.savez(model_out, mu=mu, var=var, names=np.asarray(names))
    return history


def build_model():
    return modeltts_common.DCNNF0SpecNoiseFeatures(ctxsize, vocoder, cfg)    # DCNN in the paper


def training(cont=False):
    fids = readids(cfg.fileids)
    fid_lst_tra = fids[:cfg.id_train_nb()]
    fid_lst_val = fids[cfg.id_valid_start:cfg.id_valid_start + cfg.id_valid_nb]
    mod = build_model()
    # cfg.train_validation_batch_size = n (unset here: one utterance at a time, as the reference does): the validation costs of every
    # epoch on ragged batches of up to n utterances of similar length -- one generator forward per batch feeds the RMSE, the
    # generator's and the critic's cost (OptimizerTTSWGAN.validation_costs_batch); with the bf16 critic only as
    # cfg.arch_critic_bf16 = 'chain' (its Conv2D stack takes a length per row; True is refused at prepare())
    # cfg.train_data_on_device = True (unset here: load_inoutset reads the files of every batch, as the reference does): the training
    # set is read, cropped and uploaded once (data.DeviceCorpus) and every batch is one gather launch at the windows the host loader
    # would draw -- same numpy draws, same batches, same model; cfg.train_data_on_device_maxbytes bounds the device memory it may take
    # (None: half of what is free), a larger set is trained from the host loader
    if errtype == 'LSE': opti = optimizertts.OptimizerTTS(cfg, mod)
    else:                opti = optimizertts_wgan.OptimizerTTSWGAN(cfg, mod, errtype=errtype, critic=networks_critic.Critic(vocoder, ctxsize, cfg))
    opti.train(cfg.inpath, cfg.outpath, cfg.wpath, fid_lst_tra, fid_lst_val, cfg.fparams_fullset, cont=cont)
    del mod


def build_duration_model():
    return modeltts_common.DurationModel(dur_ctxsize, cfg, layertypes=dur_layertypes, nstates=dur_nstates)


def training_durations(cont=False):
    """training() for the duration model: the LSE optimiser on cfg.dur_inpath / cfg.dur_outpath / cfg.dur_wpath, whose time axis
    is the phone index (cfg.train_batch_lengthmax then counts phones); the model goes to cfg.dur_fparams_fullset."""
    fids = readids(cfg.fileids)
    fid_lst_tra = fids[:cfg.id_train_nb()]
    fid_lst_val = fids[cfg.id_valid_start:cfg.id_valid_start + cfg.id_valid_nb]
    mod = build_duration_model()
    opti = optimizertts.OptimizerTTS(cfg, mod)
    opti.train(cfg.dur_inpath, cfg.dur_outpath, cfg.dur_wpath, fid_lst_tra, fid_lst_val, cfg.dur_fparams_fullset, cont=cont)
    del mod


def generate(fparams=None, dur_fparams=None, lab_path=None, lab_questions=None):
    """`dur_fparams` (with `lab_path`, the test utterances' labels -- times are not needed -- and `lab_questions`): the context
    rows come from predicted durations instead of cfg.inpath's aligned ones.  The duration model of that file predicts from
    cfg.dur_inpath (DurationModel.generate_durations, <model>-gen-dur/*.dur), contexts_from_durations expands them and normalises
    the rows with the statistics stored beside cfg.inpath, and generation goes on from <model>-gen-lab/*.lab.  The generated
    utterances then no longer have the targets' lengths: without cfg.objmeas_align the objective measures are left out; with
    cfg.objmeas_align = 'dtw' they are taken along each utterance's DTW path to its target of cfg.outpath
    (generate_params(objmeas_align='dtw'), csrc/dtw.hip).  cfg.objmeas_align is passed on without dur_fparams as well."""
    if dur_fparams is not None and (lab_path is None or lab_questions is None):
        raise ValueError('generate: dur_fparams goes with lab_path and lab_questions')
    fparams = cfg.fparams_fullset if fparams is None else fparams
    fids = readids(cfg.fileids)
    fid_lst_test = fids[cfg.id_valid_start + cfg.id_valid_nb:cfg.id_valid_start + cfg.id_valid_nb + cfg.id_test_nb]
    inpath, do_objmeas, objmeas_align = cfg.inpath, True, getattr(cfg, 'objmeas_align', None)
    if dur_fparams is not None:
        durmod = build_duration_model()
        durmod.load(dur_fparams)
        durdir = os.path.splitext(fparams)[0] + '-gen-dur'
        durmod.generate_durations(cfg.dur_inpath, cfg.dur_outpath, fid_lst_test, durdir, do_objmeas=False)
        del durmod
        inpath = os.path.splitext(fparams)[0] + '-gen-lab/*.lab:(-1,' + str(ctxsize) + ')'
        contexts_from_durations(lab_path, fid_lst_test, lab_questions, durdir + '/*.dur', cfg.inpath, inpath)
        do_objmeas = objmeas_align is not None
    mod = build_model()
    mod.load(fparams)
    mod.generate_cmp(inpath, os.path.splitext(fparams)[0] + '-gen/*.cmp', fid_lst_test)
    # where the reference calls generate_wav (run.py:218): everything of it up to the vocoder's synthesis, and, for a vocoder
    # with synthesis_device (VocoderPML, VocoderWORLDDevice), the waveforms of the build's own synthesiser in <model>-demo-snd
    # (cfg.wavdir overrides the place)
    demostart = cfg.id_test_demostart if hasattr(cfg, 'id_test_demostart') else 0
    # cfg.specdir / cfg.pp_mcep, if present: also write the decompressed (post-filtered) spectral envelopes;
    # cfg.predict_batched, if present and true: the network runs on each group of utterances at once (ragged inference)
    # (cfg.group_by_length beside it: the groups hold utterances of similar length); the counterpart for the validation sweep of
    # training() is cfg.train_validation_batch_size -- all three unset here
    mod.generate_params(inpath, cfg.outpath, fid_lst_test[demostart:demostart + 10], os.path.splitext(fparams)[0] + '-demo-params',
                        do_objmeas=do_objmeas, pp_mcep=getattr(cfg, 'pp_mcep', False), specdir=getattr(cfg, 'specdir', None),
                        wavdir=(getattr(cfg, 'wavdir', os.path.splitext(fparams)[0] + '-demo-snd')
                                if hasattr(mod.vocoder, 'synthesis_device') else None),
                        predict_batched=bool(getattr(cfg, 'predict_batched', False)),
                        group_by_length=bool(getattr(cfg, 'group_by_length', False)), objmeas_align=objmeas_align)


if __name__ == "__main__":
    if not os.path.exists(cfg.fileids):
        synthesize_corpus()
    training(cont='--continue' in sys.argv)
    generate()
