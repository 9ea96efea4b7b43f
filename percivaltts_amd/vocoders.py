"""Vocoder descriptors: only what the acoustic-model hot path reads.

The reference's vocoders.py:33-352 also does signal analysis/synthesis through the `pulsemodel`
submodule (absent from the reference checkout) and pyworld; that DSP is out of scope here (SURVEY.md
section 2, row 9).  The networks, the critic and the WGAN losses only need the feature-size accessors
(vocoders.py:95-109,130-131,176-179,228-232), `fs`, `shift`, `mlpg_wins`, and the class identity that
network_final switches on (networktts.py:195,212).  The objective measures of vocoders.py:112-117,209-218,333-342
(`objmeasures_clear / objmeasures_add / objmeasures_stats`) are plain numpy on a few hundred kilobytes per utterance.
`decompress_spectrum` (vocoders.py:147-166), the frame-wise step in front of the waveform generator, runs on the device
(csrc/spectrum.hip).  `VocoderPML.synthesis_device` is the build's own pulse-and-noise synthesiser (csrc/pulsesynth.hip, DESIGN.md
section 3), `VocoderWORLDDevice.synthesis_device` its periodic-plus-aperiodic synthesiser for the WORLD parameters (csrc/worldsynth.hip,
DESIGN.md section 3; VocoderWORLD itself has none); `synthesis` keeps its name for pulsemodel's / pyworld's waveform and keeps raising.  `VocoderPML.analysis_device` (with
`analysisf_device` / `analysisfid_device` around it) is the build's own waveform analysis for the same parameters
(csrc/analysis.hip), from a caller's F0 track or, without one, from the build's own F0 estimator
(`VocoderF0Spec.f0_estimate_device`, csrc/f0.hip); with `VocoderF0Spec.f0_refine` set, either track goes through the build's F0
refinement first (`f0_refine_device`, csrc/f0.hip; the StoneMask step of the reference's WORLD chain); `compress_spectrum` is the
inverse of `decompress_spectrum` for 'fwbnd'.
`VocoderF0Spec.compress_spectrum_device` is that inverse for both spectral types: for 'mcep' the build's own least-squares fit on
the warped axis (ops.spec2mcep, csrc/spectrum.hip) in the place of SPTK's, for which `compress_spectrum` keeps
its name and keeps raising; `analysis_device` takes either type.  `VocoderWORLDAnalysisDevice` adds the same three methods and
`write_streams` for the WORLD parameters (ln f0 | spec | aperiodicity [dB] | vuv): the build's own analysis, the counterpart of
`VocoderWORLDDevice.synthesis_device` (csrc/worldanalysis.hip, DESIGN.md section 3: an envelope after CheapTrick, band
aperiodicities from two windows one period apart), in the place of pyworld's; VocoderWORLD and VocoderWORLDDevice have none.
`analysis_device_batch` of both analysing vocoders is `analysis_device` over a list of utterances, every kernel launching once per
batch and nothing coming back to the host before the end (csrc/analysisbatch.hip and the *_batch kernels).
`analysisf` / `analysisfid` keep their names for pulsemodel's / pyworld's analysis and keep raising.  `Vocoder.preprocwav` (vocoders.py:45-63) is
the step in front of the analysis, on the device (csrc/preproc.hip): the build's own rational-ratio resampler in
the place of pulsemodel's, and the zero-phase order-4 Butterworth high-pass with `highpass` as the cut-off in Hz.
"""
from __future__ import print_function

import contextlib
import os

import numpy as np


def bark_alpha(fs):
    """All-pass coefficient of the Bark-like warping at sampling frequency fs (the reference's sigproc.bark_alpha)."""
    from . import ops_offline as ops
    return ops.bark_alpha(fs)


def _check_f0_refine(value):
    if value is not None and not isinstance(value, bool):
        raise ValueError('f0_refine={!r} is not None, True or False'.format(value))


def log2db(x):
    """Natural-log amplitude -> decibels (the reference's sigproc.log2db)."""
    return (20.0 / np.log(10.0)) * x


def wavwrite(path, wav, fs):
    """Write a mono waveform as 16-bit PCM (the standard library's `wave`).  A waveform whose peak exceeds 1 is divided by its peak
    first, and a line says so."""
    import wave
    wav = np.asarray(wav, dtype=np.float64).reshape(-1)
    peak = float(np.abs(wav).max()) if wav.size else 0.0
    if peak > 1.0:
        print('    wavwrite: peak {:.3f} above full scale, {} divided by its peak'.format(peak, path))
        wav = wav / peak
    pcm = np.round(wav * 32767.0).astype('<i2')
    f = wave.open(path, 'wb')
    try:
        f.setnchannels(1)
        f.setsampwidth(2)
        f.setframerate(int(round(fs)))
        f.writeframes(pcm.tobytes())
    finally:
        f.close()


def wavread(path):
    """A 16-bit mono PCM file -> (float64 waveform in [-1, 1], fs): the inverse of wavwrite.  Anything else is a ValueError."""
    import wave
    try:
        f = wave.open(path, 'rb')
    except (wave.Error, EOFError) as e:
        raise ValueError('wavread: {} is not a PCM wave file ({})'.format(path, e))
    try:
        if f.getnchannels() != 1 or f.getsampwidth() != 2 or f.getcomptype() != 'NONE':
            raise ValueError('wavread: {} is not 16-bit mono PCM ({} channels, {} bytes a sample)'.format(
                path, f.getnchannels(), f.getsampwidth()))
        fs = f.getframerate()
        pcm = np.frombuffer(f.readframes(f.getnframes()), dtype='<i2')
    finally:
        f.close()
    return pcm.astype(np.float64) / 32767.0, fs


def wavfs(path):
    """The sampling rate in a wave file's header.  Anything that is not a PCM wave file is a ValueError."""
    import wave
    try:
        f = wave.open(path, 'rb')
    except (wave.Error, EOFError) as e:
        raise ValueError('wavfs: {} is not a PCM wave file ({})'.format(path, e))
    try:
        return f.getframerate()
    finally:
        f.close()


class Vocoder(object):
    def __init__(self, name, fs, shift, mlpg_wins=None):
        self._name, self.fs, self.shift, self.mlpg_wins = name, fs, shift, mlpg_wins
        self.features_err = dict()      # per instance (a class-level dict in the reference, shared between vocoders by accident)

    def __str__(self):
        return '{} (fs={}, shift={})'.format(self.name(), self.fs, self.shift)

    def name(self):
        return self._name

    def featuressizeraw(self):
        raise ValueError('This member function has to be re-implemented in the sub-classes')

    def featuressize(self):
        n = self.featuressizeraw()
        return n * (len(self.mlpg_wins) + 1) if self.mlpg_wins is not None else n

    def f0size(self): return -1
    def specsize(self): return -1
    def noisesize(self): return -1
    def vuvsize(self): return -1

    def preprocwav(self, wav, fs, highpass=None):
        """A mono waveform at `fs` -> the waveform the analysis takes (the reference's preprocwav, vocoders.py:45-63, with its name,
        argument order and two printed lines), on the device (csrc/preproc.hip): resampled to self.fs when `fs`
        differs (ops.resample), then, with `highpass`, the zero-phase order-4 Butterworth high-pass (ops.highpass_zerophase, odd
        extension by padlen = ops.HIGHPASS_PADLEN samples).  `highpass` is the cut-off in Hz: the reference normalises it as
        highpass / (fs / 0.5), which puts the cut-off at highpass / 4 Hz; that is not reproduced.  numpy (any float array) in ->
        numpy float32 out, device tensor in -> device tensor out.  A waveform that is not finite, not 1-D, or not longer than
        padlen where it is filtered, is a ValueError, and so are rates and cut-offs that ops.preproc_check refuses."""
        import torch
        from . import backend_hip, ops_offline as ops
        padlen = ops.HIGHPASS_PADLEN
        ops.preproc_check(fs, self.fs, highpass, padlen)
        fs, fs_out = int(fs), int(self.fs)
        as_numpy = not torch.is_tensor(wav)
        if as_numpy:
            wav = np.asarray(wav, dtype=np.float64)
            if wav.ndim != 1 or not np.isfinite(wav).all():
                raise ValueError('preprocwav: wav is not a finite [N] waveform')
        elif wav.dim() != 1:
            raise ValueError('preprocwav: wav is not an [N] waveform')
        if highpass is not None:
            up, down, _ = ops.preproc_check(fs, fs_out)
            n = len(wav) if fs == fs_out else ops.resample_length(len(wav), up, down)
            if n <= padlen:
                raise ValueError('preprocwav: {} samples at {} Hz are not longer than padlen={}'.format(n, fs_out, padlen))
        x = wav
        if as_numpy:
            x = torch.from_numpy(wav.astype(np.float32)).to(backend_hip.device())
        elif not bool(torch.isfinite(x).all()):
            raise ValueError('preprocwav: wav is not a finite [N] waveform')
        if fs != fs_out:
            print('    Resampling the waveform (new fs={}Hz)'.format(self.fs))
            x = ops.resample(x, fs, fs_out)
        if highpass is not None:
            print('    High-pass filter the waveform (cutt-off={}Hz)'.format(highpass))
            x = ops.highpass_zerophase(x, fs_out, highpass, padlen=padlen)
        return x.cpu().numpy() if as_numpy else x

    # Objective measures (vocoders.py:112-117): lists of per-utterance errors, keyed by feature
    def objmeasures_clear(self):
        self.features_err = dict()

    def objmeasures_stats(self):
        """Print `key: mean` per feature as the reference does, and return them as a dict."""
        stats = dict()
        for key in self.features_err:
            stats[key] = float(np.mean(np.vstack(self.features_err[key])))
            print('{}: {}'.format(key, stats[key]))
        return stats

    # Objective measures of a pair of unequal length, along its DTW path (the build's own; DESIGN.md section 3, "DTW alignment")
    def alignment_columns(self):
        """(c0, c1, scale): the columns [c0, c1) of the raw features whose distance, times `scale`, is the local cost of the DTW
        alignment.  Overridden by the vocoders that have an alignment."""
        raise ValueError('{} has no alignment columns: its features are not frame-level'.format(self.name()))

    @staticmethod
    def check_path(gi, ri, Tg, Tr):
        """A DTW path over a Tg x Tr matrix: (0,0) to (Tg-1,Tr-1) in steps (1,1), (1,0), (0,1) -> (gi, ri) as int64 arrays."""
        gi, ri = np.asarray(gi), np.asarray(ri)
        if gi.ndim != 1 or gi.shape != ri.shape or gi.size < 1 or gi.dtype.kind not in 'iu' or ri.dtype.kind not in 'iu':
            raise ValueError('objmeasures_add_aligned: the path is not two integer index lists of one length')
        gi, ri = gi.astype(np.int64), ri.astype(np.int64)
        if gi.min() < 0 or ri.min() < 0 or gi.max() >= Tg or ri.max() >= Tr:
            raise ValueError('objmeasures_add_aligned: the path leaves the {} x {} frames'.format(Tg, Tr))
        if (gi[0], ri[0]) != (0, 0) or (gi[-1], ri[-1]) != (Tg - 1, Tr - 1):
            raise ValueError('objmeasures_add_aligned: the path does not run from (0,0) to ({},{})'.format(Tg - 1, Tr - 1))
        dg, dr = np.diff(gi), np.diff(ri)
        if not (((dg == 0) | (dg == 1)) & ((dr == 0) | (dr == 1)) & (dg + dr >= 1)).all():
            raise ValueError('objmeasures_add_aligned: a step of the path is not one of (1,1), (1,0), (0,1)')
        return gi, ri

    def objmeasures_add_aligned(self, CMP, REF, path=None):
        """objmeasures_add for a generated CMP [Tg, >=raw] and a reference REF [Tr, >=raw] of unequal length: the class's own
        objmeasures_add(CMP[gi], REF[ri]) along the DTW path (gi, ri), so that every key keeps its meaning, plus
        'DTW[cost/step]' = cost / L and 'DTW[len ratio]' = Tg / Tr.  path: None -- the pair is aligned on the device over
        alignment_columns() (ops.dtw_align); or (gi, ri) or (gi, ri, cost), e.g. of one ops.dtw_align over a batch -- then
        nothing here touches the device, and a cost that is not given is the path's own, summed in fp64 in path order."""
        CMP, REF = np.asarray(CMP), np.asarray(REF)
        raw = self.featuressizeraw()
        if CMP.ndim != 2 or REF.ndim != 2 or min(CMP.shape[0], REF.shape[0]) < 1 or min(CMP.shape[1], REF.shape[1]) < raw:
            raise ValueError('objmeasures_add_aligned: CMP {} and REF {} are not [T>=1, >={}]'.format(CMP.shape, REF.shape, raw))
        c0, c1, scale = self.alignment_columns()
        Tg, Tr = CMP.shape[0], REF.shape[0]
        cost = None
        if path is None:
            import torch
            from . import backend_hip, ops_offline as ops
            dev = backend_hip.device()
            g = torch.from_numpy(np.ascontiguousarray(CMP[:, :raw], dtype=np.float32)).to(dev)
            r = torch.from_numpy(np.ascontiguousarray(REF[:, :raw], dtype=np.float32)).to(dev)
            res = ops.dtw_align(g, r, [Tg], [Tr], cols=(c0, c1), scale=scale)
            gi, ri = res.host()[0]
            cost = float(res.cost.cpu()[0])
        elif len(path) == 3:
            gi, ri, cost = path
            cost = float(cost)
        else:
            gi, ri = path
        gi, ri = self.check_path(gi, ri, Tg, Tr)
        if cost is None:
            d = scale * (CMP[gi, c0:c1].astype(np.float64) - REF[ri, c0:c1].astype(np.float64))
            cost = float(np.sum(np.sqrt(np.sum(d * d, axis=1))))
        self.objmeasures_add(CMP[gi], REF[ri])
        self.features_err.setdefault('DTW[cost/step]', []).append(cost / gi.size)
        self.features_err.setdefault('DTW[len ratio]', []).append(Tg / float(Tr))

    def _out_of_scope(self, *a, **k):
        """analysisf / analysisfid / synthesis promise pulsemodel's or pyworld's signal processing, which this build does not have.
        The build's own synthesisers are VocoderPML.synthesis_device and VocoderWORLDDevice.synthesis_device."""
        raise NotImplementedError('waveform analysis/synthesis is outside the MI355X hot-path build '
                                  '(needs the pulsemodel/pyworld DSP of the reference)')
    analysisf = analysisfid = synthesis = _out_of_scope


class VocoderF0Spec(Vocoder):
    def __init__(self, name, fs, shift, spec_size, spec_type='fwbnd', dftlen=4096, mlpg_wins=None):
        Vocoder.__init__(self, name, fs, shift, mlpg_wins=mlpg_wins)
        self.spec_size, self.spec_type, self.dftlen = spec_size, spec_type, dftlen

    def f0size(self): return 1
    def specsize(self): return self.spec_size

    def decompress_spectrum(self, COMPSPEC, spec_type=None, pp_mcep=False):
        """Compressed spectral columns [T, spec_size] -> amplitude envelope [T, dftlen/2+1] (vocoders.py:147-166), on the device:
        'fwbnd' log-bands by interpolation (ops.fwbnd2spec), 'mcep' mel-cepstra by ops.mcep2spec with alpha = bark_alpha(fs);
        `pp_mcep` applies the formant-enhancing post-filter.  As in the reference the dispatch is on self.spec_type and the
        `spec_type` argument is not looked at.  numpy in -> numpy out, device tensor in -> device tensor out."""
        import torch
        from . import backend_hip, ops_offline as ops
        if self.spec_type not in ('fwbnd', 'mcep'):
            raise ValueError("spec_type is 'fwbnd' or 'mcep', got {!r}".format(self.spec_type))
        as_numpy = not torch.is_tensor(COMPSPEC)
        x = COMPSPEC
        if as_numpy:
            x = torch.from_numpy(np.ascontiguousarray(COMPSPEC, dtype=np.float32)).to(backend_hip.device())
        if self.spec_type == 'fwbnd':
            SPEC = ops.fwbnd2spec(x.contiguous(), self.fs, dftlen=self.dftlen, pp=pp_mcep)
        else:
            SPEC = ops.mcep2spec(x.contiguous(), bark_alpha(self.fs), dftlen=self.dftlen, pp=pp_mcep)
        return SPEC.cpu().numpy() if as_numpy else SPEC

    def compress_spectrum(self, SPEC, spec_type=None, spec_size=None):
        """Amplitude envelope [T, K] -> compressed spectral columns [T, spec_size] (vocoders.py:134-145), on the device: 'fwbnd'
        log-bands by the least-squares inverse of decompress_spectrum (ops.fwbnd_compress), so that
        compress_spectrum(decompress_spectrum(y)) = y; dftlen is read off K = dftlen/2 + 1 as in the reference.  'mcep' is a
        ValueError: the SPTK fit behind it is not built (compress_spectrum_device has the build's own).  As in the reference the
        dispatch is on self.spec_type and the `spec_type` argument is not looked at; spec_size None means self.spec_size.  numpy
        in -> numpy out, device tensor in -> device tensor out."""
        import torch
        from . import backend_hip, ops_offline as ops
        if self.spec_type == 'mcep':
            raise ValueError("compress_spectrum: the 'mcep' fit (SPTK) is not part of this build; "
                             "compress_spectrum_device has the build's own mel-cepstral fit")
        if self.spec_type != 'fwbnd':
            raise ValueError("spec_type is 'fwbnd' or 'mcep', got {!r}".format(self.spec_type))
        spec_size = self.spec_size if spec_size is None else spec_size
        as_numpy = not torch.is_tensor(SPEC)
        x = SPEC
        if as_numpy:
            x = torch.from_numpy(np.ascontiguousarray(SPEC, dtype=np.float32)).to(backend_hip.device())
        COMPSPEC = ops.fwbnd_compress(x.contiguous(), self.fs, spec_size, mode='lsq')
        return COMPSPEC.cpu().numpy() if as_numpy else COMPSPEC

    def compress_spectrum_device(self, SPEC, spec_size=None, log=False):
        """Amplitude envelope [T, K] (`log`: its logarithm) -> compressed spectral columns [T, spec_size], the inverse of
        decompress_spectrum for either spectral type, on the device: 'fwbnd' as compress_spectrum; 'mcep' the mel-cepstrum of order
        spec_size - 1 by the build's own fit, ops.spec2mcep(SPEC, bark_alpha(fs), spec_size - 1, log).  The
        reference's 'mcep' branch scales SPEC by fs first (vocoders.py:141), which its decompress_spectrum does not undo; that is
        not reproduced.  dftlen is read off K; spec_size None means self.spec_size.  numpy in -> numpy out, device tensor in ->
        device tensor out."""
        import torch
        from . import backend_hip, ops_offline as ops
        if self.spec_type not in ('fwbnd', 'mcep'):
            raise ValueError("spec_type is 'fwbnd' or 'mcep', got {!r}".format(self.spec_type))
        spec_size = self.spec_size if spec_size is None else spec_size
        as_numpy = not torch.is_tensor(SPEC)
        x = SPEC
        if as_numpy:
            x = torch.from_numpy(np.ascontiguousarray(SPEC, dtype=np.float32)).to(backend_hip.device())
        if self.spec_type == 'fwbnd':
            COMPSPEC = ops.fwbnd_compress(x.contiguous(), self.fs, spec_size, mode='lsq', log=log)
        else:
            COMPSPEC = ops.spec2mcep(x.contiguous(), bark_alpha(self.fs), spec_size - 1, log=log)
        return COMPSPEC.cpu().numpy() if as_numpy else COMPSPEC

    def f0_estimate_device(self, wav, f0_min, f0_max):
        """A mono waveform at self.fs (any float array) -> its F0 track in Hz, numpy float32, one value per frame at shift * i for
        every frame whose centre lies within the waveform, 0 where unvoiced: the build's own estimator (ops.f0_estimate, csrc/f0.hip,
        DESIGN.md section 3) in the place of the pitch tracker the reference runs."""
        from . import ops_offline as ops
        return ops.f0_estimate(wav, self.shift, self.fs, self.dftlen, f0_min, f0_max)

    # True: the analysis_device of a subclass passes its F0 track, the caller's or the estimated one, through f0_refine_device.
    # A class attribute: it does not enter the instance dictionaries, so stored vocoders stay as they are.
    f0_refine = False

    def f0_refine_device(self, wav, f0, f0_min, f0_max):
        """A mono waveform at self.fs (any float array) and an F0 track in Hz, one value per frame at shift * i (<= 0: unvoiced) ->
        the track refined by the instantaneous frequency of its harmonics, numpy float32, the voicing pattern unchanged
        (ops.f0_refine, csrc/f0.hip): the build's counterpart of the reference's StoneMask step
        (vocoders.py:261)."""
        from . import ops_offline as ops
        return ops.f0_refine(wav, f0, self.shift, self.fs, f0_min, f0_max)

    @contextlib.contextmanager
    def f0_refine_as(self, value):
        """Inside the `with` block self.f0_refine is `value` (True or False); None leaves it alone.  Afterwards, also on an
        exception, the vocoder is as it was: an instance without the attribute of its own has none again."""
        _check_f0_refine(value)
        if value is None:
            yield self
            return
        own = 'f0_refine' in vars(self)
        before = self.f0_refine
        self.f0_refine = value
        try:
            yield self
        finally:
            if own:
                self.f0_refine = before
            else:
                del self.f0_refine

    def _objmeasures_add_f0spec(self, CMP, REF):
        """F0[Hz]: RMS of the exp(f0) differences; SPEC[dB]: per-band RMS of the log2db differences."""
        self.features_err.setdefault('F0[Hz]', []).append(np.sqrt(np.mean((np.exp(REF[:, 0]) - np.exp(CMP[:, 0]))**2)))
        spectrg = log2db(REF[:, 1:1 + self.spec_size])
        specgen = log2db(CMP[:, 1:1 + self.spec_size])
        self.features_err.setdefault('SPEC[dB]', []).append(np.sqrt(np.mean((spectrg - specgen)**2, 0)))

    def alignment_columns(self):
        """The spectral columns, times the log2db factor: the local cost is a distance in dB over the bands.  For 'mcep' c_0 is
        left out (the mel-cepstral-distortion convention), so a spec_size of 1 has nothing to align on."""
        c0 = 2 if self.spec_type == 'mcep' else 1
        if c0 >= 1 + self.spec_size:
            raise ValueError('{}: no alignment columns for spec_type={!r} with spec_size={}'.format(self.name(), self.spec_type,
                                                                                                    self.spec_size))
        return c0, 1 + self.spec_size, log2db(1.0)

    def _objmeasures_add_band(self, key, CMP, REF, size):
        lo = 1 + self.spec_size
        self.features_err.setdefault(key, []).append(np.sqrt(np.mean((REF[:, lo:lo + size] - CMP[:, lo:lo + size])**2, 0)))

    # What the synthesis_device / analysis_device / analysisf_device / write_streams / analysisfid_device of the subclasses share.
    def _synthesis_input(self, CMP, pp_f0_smooth):
        """The checks of a synthesis_device -> (CMP as a device tensor, T, wavlen)."""
        import torch
        from . import backend_hip, ops
        if pp_f0_smooth is not None:
            raise ValueError('pp_f0_smooth={!r}: f0 smoothing is not part of this synthesiser'.format(pp_f0_smooth))
        if not hasattr(CMP, 'shape') or len(CMP.shape) != 2 or CMP.shape[1] != self.featuressizeraw() or CMP.shape[0] < 1:
            raise ValueError('synthesis_device: CMP is not [T, {}] with T >= 1'.format(self.featuressizeraw()))
        ops.pulse_check(self.dftlen, self.fs)
        x = CMP
        if not torch.is_tensor(x):
            x = torch.from_numpy(np.ascontiguousarray(CMP, dtype=np.float32)).to(backend_hip.device())
        if x.requires_grad:
            raise ValueError('synthesis_device has no backward pass: detach its input')
        T = x.shape[0]
        return x, T, int(round(self.shift * (T - 1) * self.fs))

    def _synthesis_batch_input(self, CMPs, noise):
        """The checks of a synthesis_device_batch -> (the utterances' rows packed into one device tensor [sum T, raw], their
        lengths, their wavlens, the noise as a list with one entry per utterance: the caller's tensors, or None to draw)."""
        import torch
        from . import backend_hip, ops
        CMPs = list(CMPs)
        if not CMPs:
            raise ValueError('synthesis_device_batch: no utterance given')
        for c in CMPs:
            if not hasattr(c, 'shape') or len(c.shape) != 2 or c.shape[1] != self.featuressizeraw() or c.shape[0] < 1:
                raise ValueError('synthesis_device_batch: a CMP is not [T, {}] with T >= 1'.format(self.featuressizeraw()))
            if torch.is_tensor(c) and c.requires_grad:
                raise ValueError('synthesis_device_batch has no backward pass: detach its input')
        ops.pulse_check(self.dftlen, self.fs)
        noise = [None] * len(CMPs) if noise is None else list(noise)
        if len(noise) != len(CMPs):
            raise ValueError('synthesis_device_batch: noise is not one [wavlen] tensor per utterance')
        if not any(torch.is_tensor(c) for c in CMPs):
            x = torch.from_numpy(np.concatenate([np.asarray(c, dtype=np.float32) for c in CMPs])).to(backend_hip.device())
        else:
            dev = next(c.device for c in CMPs if torch.is_tensor(c))
            x = torch.cat([c.to(torch.float32) if torch.is_tensor(c) else torch.from_numpy(np.ascontiguousarray(c, dtype=np.float32)).to(dev)
                           for c in CMPs])
        lengths = [int(c.shape[0]) for c in CMPs]
        wavlens = [int(round(self.shift * (T - 1) * self.fs)) for T in lengths]
        return x, lengths, wavlens, noise

    @staticmethod
    def _draw_noise(noise, wavlens, device):
        """Every missing entry drawn by its own ops.normal call, in utterance order: the generator's call counter advances as
        under a loop of synthesis_device calls."""
        from . import ops
        return [ops.normal((n,), device=device, i0=0) if g is None else g for g, n in zip(noise, wavlens)]

    def _analysis_input(self, check, wav, f0, f0_min, f0_max):
        """The checks of an analysis_device (check: ops.analysis_check or ops.world_analysis_check) and its F0 steps -> (wav as
        float64, f0 as given, estimated or refined, the continuous track of ops.f0_track)."""
        from . import ops_offline as ops
        if self.spec_type not in ('fwbnd', 'mcep'):
            raise ValueError("analysis_device: spec_type is 'fwbnd' or 'mcep', got {!r}".format(self.spec_type))
        check(self.dftlen, self.fs, self.shift, f0_min, f0_max)
        if self.spec_type == 'fwbnd':
            ops.fwbnd_compress_check(self.spec_size, self.fs, self.dftlen)
        else:
            ops.spec2mcep_check(self.spec_size - 1, bark_alpha(self.fs), self.dftlen)
        ops.fwbnd_compress_check(self.noisesize(), self.fs, self.dftlen)
        wav = np.asarray(wav, dtype=np.float64)
        if wav.ndim != 1 or not np.isfinite(wav).all():
            raise ValueError('analysis_device: wav is not a finite [N] waveform')
        if f0 is None:
            f0 = self.f0_estimate_device(wav, f0_min, f0_max)
        if self.f0_refine:
            f0 = self.f0_refine_device(wav, f0, f0_min, f0_max)
        return wav, f0, ops.f0_track(f0, f0_min, f0_max, self.fs, self.shift, self.dftlen, wavlen=wav.size)

    def _analysis_device_batch(self, check, frames, wavs, f0s, f0_min, f0_max, want_f0):
        """What the analysis_device_batch of the subclasses share (check: ops.analysis_check or ops.world_analysis_check; frames:
        (wav, wav layout, track, vuv, frame layout) -> (the log-envelope [sum T, K], the columns behind the spectral ones), all on
        the device).  Every check that needs no device runs first, once per batch; then the waveforms (and the given tracks) go up
        in one packed tensor each, the F0 steps of _analysis_input and the frame kernels launch once per batch
        (ops.f0_estimate_batch, ops.f0_refine_batch, ops.f0_track_device, `frames`, compress_spectrum_device), and the host reads
        the status words and the packed matrix back, once each, and takes column 0's logarithm as analysis_device does."""
        import torch
        from . import backend_hip, ops_offline as ops
        fn = 'analysis_device_batch'
        if self.spec_type not in ('fwbnd', 'mcep'):
            raise ValueError("{}: spec_type is 'fwbnd' or 'mcep', got {!r}".format(fn, self.spec_type))
        check(self.dftlen, self.fs, self.shift, f0_min, f0_max)
        if self.spec_type == 'fwbnd':
            ops.fwbnd_compress_check(self.spec_size, self.fs, self.dftlen)
        else:
            ops.spec2mcep_check(self.spec_size - 1, bark_alpha(self.fs), self.dftlen)
        ops.fwbnd_compress_check(self.noisesize(), self.fs, self.dftlen)
        wavs = list(wavs)
        if not wavs:
            raise ValueError('{}: no utterance given'.format(fn))
        if f0s is not None:
            f0s = list(f0s)
            if len(f0s) != len(wavs) or any(f is None for f in f0s):
                raise ValueError('{}: f0s is None (every track is estimated) or one track per utterance, not a mixture'.format(fn))
        else:
            ops.f0_check(self.dftlen, self.fs, self.shift, f0_min, f0_max)
        if self.f0_refine:
            ops.f0_refine_check(self.fs, self.shift, f0_min, f0_max)
        for b, w in enumerate(wavs):
            wavs[b] = w = np.asarray(w, dtype=np.float64)
            if w.ndim != 1 or not np.isfinite(w).all():
                raise ValueError('{}: utterance {}: wav is not a finite [N] waveform'.format(fn, b))
        if f0s is not None:
            for b, f in enumerate(f0s):
                # as the single path: ops.f0_refine takes the track as float32 (NaN: unvoiced), ops.f0_track as float64
                f0s[b] = f = np.array(f, dtype=np.float32) if self.f0_refine else np.asarray(f, dtype=np.float64)
                if f.ndim != 1 or f.size < 1 or not (self.f0_refine or np.isfinite(f).all()):
                    raise ValueError('{}: utterance {}: ops.f0_track: f0 has to be [T] finite Hz values, T >= 1'.format(fn, b))
        dev = backend_hip.device()
        wav = torch.from_numpy(np.concatenate([w.astype(np.float32) for w in wavs])).to(dev)
        wo = ops.packed_offsets([w.size for w in wavs], dev, fn)
        info = torch.zeros(len(wavs), dtype=torch.int32, device=dev)
        if f0s is None:
            f0, fo = ops.f0_estimate_batch(wav, wo, self.shift, self.fs, self.dftlen, f0_min, f0_max, info=info)
        else:
            f0 = torch.from_numpy(np.concatenate(f0s)).to(dev)
            fo = ops.packed_offsets([f.size for f in f0s], dev, fn)
        f0_in = f0
        if self.f0_refine:
            f0 = ops.f0_refine_batch(wav, wo, f0, fo, self.shift, self.fs, f0_min, f0_max)
        track, vuv, oo = ops.f0_track_device(f0, fo, wo, f0_min, f0_max, self.fs, self.shift, self.dftlen, info=info)
        lspec, columns = frames(wav, wo, track, vuv, oo)
        bands = self.compress_spectrum_device(lspec, log=True)
        CMP = torch.cat([track[:, None], bands] + list(columns), dim=1)
        ops.analysis_status(fn, info)
        CMP = CMP.cpu().numpy()
        CMP[:, 0] = np.log(CMP[:, 0].astype(np.float64)).astype(np.float32)
        out = [np.ascontiguousarray(c) for c in np.split(CMP, oo.off[1:-1])]
        if want_f0:
            return out, [np.ascontiguousarray(f) for f in np.split(f0_in.cpu().numpy(), fo.off[1:-1])]
        return out

    def _analysisf_device(self, label, fwav, f0_in, f0_min, f0_max, streams, kwargs):
        """analysis_device from the wave file fwav to the files `streams`, in the order of write_streams' arguments."""
        if kwargs.get('preproc_hp') is not None:
            raise ValueError('analysisf_device: preproc_hp={!r}: the high-pass pre-processing is not built'.format(kwargs['preproc_hp']))
        if set(kwargs) - {'preproc_hp', 'f0_refine'}:
            raise ValueError('analysisf_device: unknown arguments {}'.format(sorted(set(kwargs) - {'preproc_hp', 'f0_refine'})))
        _check_f0_refine(kwargs.get('f0_refine'))
        print('Extracting {} features from: '.format(label) + fwav)
        wav, fs = wavread(fwav)
        if fs != int(round(self.fs)):
            raise ValueError('analysisf_device: {} is sampled at {} Hz, the vocoder at {} (resampling is not built)'.format(fwav, fs, self.fs))
        f0 = np.fromfile(f0_in, dtype=np.float32) if isinstance(f0_in, str) else f0_in
        with self.f0_refine_as(kwargs.get('f0_refine')):
            CMP = self.analysis_device(wav, f0, f0_min, f0_max)
        return self.write_streams(CMP, *streams)

    def _write_streams(self, CMP, paths_and_columns):
        """Each (path, columns of CMP) pair as a headerless float32 file; missing directories are made.  Returns T."""
        for path, cols in paths_and_columns:
            if os.path.dirname(path) and not os.path.isdir(os.path.dirname(path)):
                os.makedirs(os.path.dirname(path))
            np.ascontiguousarray(cols, dtype=np.float32).tofile(path)
        return CMP.shape[0]

    def _analysisfid_device(self, fid, wav_path, f0in_path, f0_min, f0_max, outputpathdicts, keys, kwargs):
        """analysisf_device with the '*' of every path replaced by fid; keys: those of outputpathdicts in the order of ff0, fspec
        and the streams behind them."""
        f0_in = None if f0in_path is None else f0in_path.replace('*', fid)
        fwav = wav_path.replace('*', fid)
        out = [outputpathdicts[key].replace('*', fid) for key in keys]
        return self.analysisf_device(fwav, f0_in, out[0], f0_min, f0_max, *out[1:], **kwargs)


class VocoderPML(VocoderF0Spec):
    """f0 | spec | noise mask"""
    def __init__(self, fs, shift, spec_size, nm_size, dftlen=4096, mlpg_wins=None, spec_type='fwbnd'):
        # spec_type: a build extension (the reference hard-codes 'fwbnd' although its base class handles 'mcep')
        VocoderF0Spec.__init__(self, 'PML', fs, shift, spec_size, spec_type, dftlen, mlpg_wins=mlpg_wins)
        self.nm_size = nm_size

    def featuressizeraw(self): return 1 + self.spec_size + self.nm_size
    def noisesize(self): return self.nm_size
    def vuvsize(self): return 0

    def objmeasures_add(self, CMP, REF):
        """Generated and target [T, >= raw] de-normalised features of one utterance (vocoders.py:209-218)."""
        self._objmeasures_add_f0spec(CMP, REF)
        self._objmeasures_add_band('NM', CMP, REF, self.nm_size)

    def synthesis_device(self, CMP, pp_mcep=False, pp_f0_smooth=None, noise=None):
        """De-normalised parameters [T, featuressizeraw()] (numpy or a device tensor) -> the waveform, numpy float32
        [round(shift (T-1) fs)], by the build's pulse-and-noise synthesiser: exp(lf0), decompress_spectrum
        (`pp_mcep` passed through), the noise mask, the pulse table on the host, one segment per pulse and their overlap-add
        (csrc/pulsesynth.hip).  `noise`: a [wavlen] fp32 device tensor of N(0,1) samples, used as it is; None draws them from the
        library's generator, so ops.rng_seed makes a waveform reproducible.  Not built: f0 smoothing (`pp_f0_smooth` other than
        None is a ValueError), ener_multT0, nm_cont, pp_atten1stharminsilences."""
        import torch
        from . import ops
        x, T, wavlen = self._synthesis_input(CMP, pp_f0_smooth)
        s1 = 1 + self.spec_size
        f0 = torch.exp(x[:, 0]).contiguous()
        table = ops.pulse_table(f0.cpu().numpy(), self.shift, self.fs, wavlen, self.dftlen)
        SPEC = self.decompress_spectrum(x[:, 1:s1].contiguous(), pp_mcep=pp_mcep)
        mask = ops.noise_mask(x[:, s1:s1 + self.nm_size].contiguous(), f0, self.fs, self.dftlen)
        if noise is None:
            noise = ops.normal((wavlen,), device=x.device, i0=0)
        return ops.pulse_synthesis(SPEC, mask, table, noise, self.fs, self.dftlen, wavlen).cpu().numpy()

    def synthesis_device_batch(self, CMPs, pp_mcep=False, noise=None):
        """synthesis_device over a list of utterances, [T_b, featuressizeraw()] each (numpy or device tensors) -> the list of their
        waveforms, numpy float32, each byte for byte what synthesis_device gives for that utterance alone.  The rows are packed
        once; exp(lf0), decompress_spectrum and the noise mask run once over the packed rows, the pulse table is built on the
        device (ops.pulse_table_device: no f0 comes back to the host, no loop over the pulses), and the segments and the
        overlap-add are one launch each for the whole batch (ops.pulse_synthesis_batch).  `noise`: a list with one [wavlen_b] fp32
        device tensor per utterance; None draws each utterance's by its own call of the library's generator, in utterance order,
        as a loop of synthesis_device calls would (so, as there, an utterance of one frame, which has no samples, needs its empty
        noise given: the generator draws no empty tensor).  An f0 above ops.PULSE_F0_CAP is a ValueError."""
        import torch
        from . import ops
        x, lengths, wavlens, noise = self._synthesis_batch_input(CMPs, noise)
        s1 = 1 + self.spec_size
        f0 = torch.exp(x[:, 0]).contiguous()
        table = ops.pulse_table_device(f0, lengths, self.shift, self.fs, self.dftlen)
        SPEC = self.decompress_spectrum(x[:, 1:s1].contiguous(), pp_mcep=pp_mcep)
        mask = ops.noise_mask(x[:, s1:s1 + self.nm_size].contiguous(), f0, self.fs, self.dftlen)
        noise = self._draw_noise(noise, wavlens, x.device)
        return [w.cpu().numpy() for w in ops.pulse_synthesis_batch(SPEC, mask, table, noise, self.fs, self.dftlen)]

    def analysis_device(self, wav, f0, f0_min, f0_max):
        """A mono waveform at self.fs (any float array) and an F0 track in Hz, one value per frame at shift * i (<= 0: unvoiced;
        None: the track of f0_estimate_device) -> the parameters [T, featuressizeraw()] float32, columns ln f0 | spec bands or
        mel-cepstrum | noise-mask bands, by the build's own analysis
        (DESIGN.md section 3): ops.f0_track on the host, then the harmonic envelope and the phase-distortion phasors of every frame
        (ops.frame_harmonics), their coherence over neighbouring frames as the noise mask (ops.phase_coherence) and the compression
        of the log-envelope by self.spec_type: 'fwbnd' the least-squares band values (ops.fwbnd_compress), 'mcep' the mel-cepstrum
        of order spec_size - 1 (ops.spec2mcep).  The noise mask is on the fwbnd axis either way.  The counterpart of
        synthesis_device.  Where self.f0_refine is true the track, given or estimated, goes through f0_refine_device first."""
        import torch
        from . import backend_hip, ops_offline as ops
        wav, f0, track = self._analysis_input(ops.analysis_check, wav, f0, f0_min, f0_max)
        hcap = ops.analysis_check(self.dftlen, self.fs, self.shift, f0_min, f0_max)
        dev = backend_hip.device()
        w = torch.from_numpy(wav.astype(np.float32)).to(dev)
        f = torch.from_numpy(track).to(dev)
        lspec, u = ops.frame_harmonics(w, f, self.shift, self.fs, self.dftlen, hcap, log=True)
        _, nm = ops.phase_coherence(u, f, self.shift, self.fs, self.dftlen, self.nm_size)
        bands = self.compress_spectrum_device(lspec, log=True)
        lf0 = np.log(track.astype(np.float64)).astype(np.float32)
        return np.concatenate([lf0[:, None], bands.cpu().numpy(), nm.cpu().numpy()], axis=1)

    def analysis_device_batch(self, wavs, f0s, f0_min, f0_max, want_f0=False):
        """analysis_device over a list of utterances: wavs mono waveforms at self.fs (any float arrays), f0s None (every track is
        estimated) or a list with one F0 track per utterance (a list that mixes tracks and None is a ValueError) -> the list of
        their [T_b, featuressizeraw()] float32 matrices, each byte for byte what analysis_device gives for that utterance alone
        (with f0s None: for that utterance and the batch's own estimated track, which `want_f0` returns as a second list, as it
        is in front of the refinement; the waveform's peak is measured by ops.wave_peak, whose last bit may differ from the
        single path's).  The waveforms are uploaded once, every kernel launches once per batch (ops.f0_estimate_batch,
        ops.f0_refine_batch where self.f0_refine is true, ops.f0_track_device, ops.frame_harmonics_batch,
        ops.phase_coherence_batch, the compression), and the host reads the status words and the packed matrix back at the end,
        nothing in between.  What analysis_device refuses is a ValueError that names the utterance's index; nothing is returned
        then."""
        from . import ops_offline as ops
        hcap = ops.analysis_check(self.dftlen, self.fs, self.shift, f0_min, f0_max)

        def frames(wav, wo, track, vuv, oo):
            lspec, u = ops.frame_harmonics_batch(wav, wo, track, oo, self.shift, self.fs, self.dftlen, hcap, log=True)
            _, nm = ops.phase_coherence_batch(u, track, oo, self.shift, self.fs, self.dftlen, self.nm_size)
            return lspec, [nm]
        return self._analysis_device_batch(ops.analysis_check, frames, wavs, f0s, f0_min, f0_max, want_f0)

    def analysisf_device(self, fwav, f0_in, ff0, f0_min, f0_max, fspec, fnm, **kwargs):
        """analysis_device from file to files, where the reference's analysisf writes them (vocoders.py:181-189): fwav a 16-bit mono
        wave file at self.fs, f0_in a headerless float32 file, or an array, of Hz values per frame, or None for the build's own
        estimate; ff0 gets ln f0, fspec the spectral bands, fnm the noise-mask bands, headerless float32 (write_streams).  The
        keyword f0_refine (None, True or False) overrides self.f0_refine for this call.  Another fs and any preproc_hp (the other
        keyword taken, None) stay a ValueError here: a file that needs resampling or the high-pass filter goes through preprocwav
        and analysis_device, as run.features_extraction(..., preproc_hp=) does."""
        return self._analysisf_device('PML', fwav, f0_in, f0_min, f0_max, (ff0, fspec, fnm), kwargs)

    def write_streams(self, CMP, ff0, fspec, fnm):
        """The parameters [T, featuressizeraw()] of analysis_device -> the three headerless float32 files of analysisf_device: ff0
        gets ln f0, fspec the spectral bands, fnm the noise-mask bands; missing directories are made.  Returns T."""
        s1 = 1 + self.spec_size
        return self._write_streams(CMP, ((ff0, CMP[:, 0]), (fspec, CMP[:, 1:s1]), (fnm, CMP[:, s1:])))

    def analysisfid_device(self, fid, wav_path, f0in_path, f0_min, f0_max, outputpathdicts, **kwargs):
        """analysisf_device with the '*' of every path replaced by the file id, as the reference's analysisfid
        (vocoders.py:191-192); outputpathdicts: {'f0': .., 'spec': .., 'noise': ..}; f0in_path None: the build's own F0 estimate."""
        return self._analysisfid_device(fid, wav_path, f0in_path, f0_min, f0_max, outputpathdicts, ('f0', 'spec', 'noise'), kwargs)


class VocoderWORLD(VocoderF0Spec):
    """f0 | spec | aperiodicity | vuv"""
    def __init__(self, fs, shift, spec_size, aper_size, dftlen=4096, mlpg_wins=None, spec_type='fwbnd'):
        VocoderF0Spec.__init__(self, 'WORLD', fs, shift, spec_size, spec_type, dftlen, mlpg_wins=mlpg_wins)
        self.aper_size = aper_size

    def featuressizeraw(self): return 1 + self.spec_size + self.aper_size + 1
    def noisesize(self): return self.aper_size
    def vuvsize(self): return 1

    def objmeasures_add(self, CMP, REF):
        """As VocoderPML's, the aperiodicity bands in place of the noise mask (vocoders.py:333-342; no VUV measure there)."""
        self._objmeasures_add_f0spec(CMP, REF)
        self._objmeasures_add_band('APER[dB]', CMP, REF, self.aper_size)


class VocoderWORLDDevice(VocoderWORLD):
    """VocoderWORLD with the build's own synthesiser for its parameters.  A class of its own because VocoderWORLD carries the
    reference's name and, like the reference's class without pyworld, produces no waveform; the networks and run.features_compose
    treat this one as a WORLD vocoder (isinstance)."""

    def synthesis_device(self, CMP, pp_mcep=False, pp_f0_smooth=None, noise=None):
        """De-normalised parameters [T, featuressizeraw()] (numpy or a device tensor), columns ln f0 | spec | aperiodicity [dB] |
        vuv -> the waveform, numpy float32 [round(shift (T-1) fs)], by the build's periodic-plus-aperiodic synthesiser (DESIGN.md
        section 3): exp(lf0) as it is (the reference writes a continuous ln f0), frames with vuv >= 0.5 voiced, decompress_spectrum
        (`pp_mcep` passed through; an amplitude envelope), the aperiodicity of every bin (ops.aper_rows), the pulse table on the
        host (ops.world_pulse_table), one segment per pulse and their overlap-add (csrc/worldsynth.hip).  `noise`: a [wavlen] fp32
        device tensor of N(0,1) samples, used as it is; None draws them from the library's generator, so ops.rng_seed makes a
        waveform reproducible.  Not built: f0 smoothing (`pp_f0_smooth` other than None is a ValueError, as in the reference's
        WORLD synthesis), WORLD's per-sample spectral interpolation inside a pulse, its safeguards on minimum-phase underflow."""
        import torch
        from . import ops
        x, T, wavlen = self._synthesis_input(CMP, pp_f0_smooth)
        s1 = 1 + self.spec_size
        f0 = torch.exp(x[:, 0])
        vuv = x[:, -1].contiguous()
        table = ops.world_pulse_table(f0.cpu().numpy(), vuv.cpu().numpy() >= 0.5, self.shift, self.fs, wavlen, self.dftlen)
        SPEC = self.decompress_spectrum(x[:, 1:s1].contiguous(), pp_mcep=pp_mcep)
        aper = ops.aper_rows(x[:, s1:s1 + self.aper_size].contiguous(), vuv, self.fs, self.dftlen)
        if noise is None:
            noise = ops.normal((wavlen,), device=x.device, i0=0)
        return ops.world_synthesis(SPEC, aper, table, noise, self.fs, self.dftlen, wavlen).cpu().numpy()

    def synthesis_device_batch(self, CMPs, pp_mcep=False, noise=None):
        """synthesis_device over a list of utterances, [T_b, featuressizeraw()] each (numpy or device tensors) -> the list of their
        waveforms, numpy float32, each byte for byte what synthesis_device gives for that utterance alone: VocoderPML's
        synthesis_device_batch with the WORLD form of the table (ops.pulse_table_device(..., voiced=vuv >= 0.5)), ops.aper_rows
        over the packed rows and ops.world_synthesis_batch."""
        import torch
        from . import ops
        x, lengths, wavlens, noise = self._synthesis_batch_input(CMPs, noise)
        s1 = 1 + self.spec_size
        f0 = torch.exp(x[:, 0]).contiguous()
        vuv = x[:, -1].contiguous()
        table = ops.pulse_table_device(f0, lengths, self.shift, self.fs, self.dftlen, voiced=vuv >= 0.5)
        SPEC = self.decompress_spectrum(x[:, 1:s1].contiguous(), pp_mcep=pp_mcep)
        aper = ops.aper_rows(x[:, s1:s1 + self.aper_size].contiguous(), vuv, self.fs, self.dftlen)
        noise = self._draw_noise(noise, wavlens, x.device)
        return [w.cpu().numpy() for w in ops.world_synthesis_batch(SPEC, aper, table, noise, self.fs, self.dftlen)]


class VocoderWORLDAnalysisDevice(VocoderWORLDDevice):
    """VocoderWORLDDevice with the build's own waveform analysis for its parameters, the counterpart of its synthesis_device.  A
    class of its own because VocoderWORLDDevice, like VocoderWORLD, is known to have no analysis; run.features_extraction takes
    this one (isinstance VocoderWORLD, with analysisfid_device)."""

    def analysis_device(self, wav, f0, f0_min, f0_max):
        """A mono waveform at self.fs (any float array) and an F0 track in Hz, one value per frame at shift * i (<= 0: unvoiced;
        None: the track of f0_estimate_device) -> the parameters [T, featuressizeraw()] float32, columns ln f0 | spec bands or
        mel-cepstrum | aperiodicity bands [dB] | vuv, by the build's own analysis: vuv_i = 1 where f0_i > 0;
        ln of ops.f0_track's continuous track (the reference interpolates before np.log as well); the envelope of every frame at
        the rate f0_i where voiced and ops.WORLD_UNVOICED_RATE where not (ops.world_envelope), compressed by self.spec_type
        (compress_spectrum_device, log=True); the band aperiodicities of the voiced frames, 0 dB in the unvoiced ones
        (ops.world_aperiodicity).  Where self.f0_refine is true the track, given or estimated, goes through f0_refine_device first
        (the StoneMask step of the reference's chain; the voicing pattern does not change).  Not built: D4C's group-delay
        statistics, the reference's linbnd2fwbnd of a per-bin aperiodicity (the bands are estimated directly)."""
        import torch
        from . import backend_hip, ops_offline as ops
        wav, f0, track = self._analysis_input(ops.world_analysis_check, wav, f0, f0_min, f0_max)
        vuv =(np.asarray(f0, dtype=np.float64)[:track.size] > 0).astype(np.float32)
        rate = np.where(vuv > 0, track, np.float32(ops.WORLD_UNVOICED_RATE)).astype(np.float32)
        dev = backend_hip.device()
        w = torch.from_numpy(wav.astype(np.float32)).to(dev)
        lspec = ops.world_envelope(w, torch.from_numpy(rate).to(dev), self.shift, self.fs, self.dftlen, log=True)
        aper = ops.world_aperiodicity(w, torch.from_numpy(track).to(dev), torch.from_numpy(vuv).to(dev), self.shift, self.fs,
                                      self.dftlen, self.aper_size)
        bands = self.compress_spectrum_device(lspec, log=True)
        lf0 = np.log(track.astype(np.float64)).astype(np.float32)
        return np.concatenate([lf0[:, None], bands.cpu().numpy(), aper.cpu().numpy(), vuv[:, None]], axis=1)

    def analysis_device_batch(self, wavs, f0s, f0_min, f0_max, want_f0=False):
        """analysis_device over a list of utterances, as VocoderPML.analysis_device_batch: the list of their [T_b,
        featuressizeraw()] float32 matrices, each byte for byte what analysis_device gives for that utterance alone, with
        ops.world_envelope_batch and ops.world_aperiodicity_batch as the frame kernels; vuv and the rate of every frame (the track
        where voiced, ops.WORLD_UNVOICED_RATE where not) stay on the device."""
        import torch
        from . import ops_offline as ops

        def frames(wav, wo, track, vuv, oo):
            rate = torch.where(vuv > 0, track, torch.full_like(track, ops.WORLD_UNVOICED_RATE))
            lspec = ops.world_envelope_batch(wav, wo, rate, oo, self.shift, self.fs, self.dftlen, log=True)
            aper = ops.world_aperiodicity_batch(wav, wo, track, vuv, oo, self.shift, self.fs, self.dftlen, self.aper_size)
            return lspec, [aper, vuv[:, None]]
        return self._analysis_device_batch(ops.world_analysis_check, frames, wavs, f0s, f0_min, f0_max, want_f0)

    def analysisf_device(self, fwav, f0_in, ff0, f0_min, f0_max, fspec, faper, fvuv, **kwargs):
        """analysis_device from file to files, where the reference's analysisf writes them (vocoders.py:234-284): fwav a 16-bit mono
        wave file at self.fs, f0_in a headerless float32 file, or an array, of Hz values per frame, or None for the build's own
        estimate; ff0 gets ln f0, fspec the spectral bands, faper the aperiodicity bands in dB, fvuv the voicing decisions,
        headerless float32 (write_streams).  The keyword f0_refine (None, True or False) overrides self.f0_refine for this call.
        Another fs and any preproc_hp (the other keyword taken, None) stay a ValueError here, as
        in VocoderPML.analysisf_device: such a file goes through preprocwav and analysis_device, as
        run.features_extraction(..., preproc_hp=) does."""
        return self._analysisf_device('WORLD', fwav, f0_in, f0_min, f0_max, (ff0, fspec, faper, fvuv), kwargs)

    def write_streams(self, CMP, ff0, fspec, faper, fvuv):
        """The parameters [T, featuressizeraw()] of analysis_device -> the four headerless float32 files of analysisf_device: ff0
        gets ln f0, fspec the spectral bands, faper the aperiodicity bands, fvuv the voicing decisions; missing directories are
        made.  Returns T."""
        s1 = 1 + self.spec_size
        s2 = s1 + self.aper_size
        return self._write_streams(CMP, ((ff0, CMP[:, 0]), (fspec, CMP[:, 1:s1]), (faper, CMP[:, s1:s2]), (fvuv, CMP[:, s2:])))

    def analysisfid_device(self, fid, wav_path, f0in_path, f0_min, f0_max, outputpathdicts, **kwargs):
        """analysisf_device with the '*' of every path replaced by the file id, as the reference's analysisfid
        (vocoders.py:297-298); outputpathdicts: {'f0': .., 'spec': .., 'noise': .., 'vuv': ..}; f0in_path None: the build's own F0
        estimate."""
        return self._analysisfid_device(fid, wav_path, f0in_path, f0_min, f0_max, outputpathdicts, ('f0', 'spec', 'noise', 'vuv'), kwargs)


class DurationFeatures(Vocoder):
    """The output features of a duration model (modeltts_common.DurationModel): `nstates` durations per phone, in frames of `shift`
    seconds.  A Vocoder only as far as the model and the optimiser ask one: sizes, the shift, objective measures.  There is no
    f0, spectrum or noise stream, no delta window and no waveform."""

    def __init__(self, shift, nstates=5):
        if int(nstates) != nstates or nstates < 1:
            raise ValueError('DurationFeatures: nstates={!r} is not a positive integer'.format(nstates))
        Vocoder.__init__(self, 'durations', None, shift, mlpg_wins=None)
        self.nstates = int(nstates)

    def featuressizeraw(self): return self.nstates
    def f0size(self): return 0
    def specsize(self): return 0
    def noisesize(self): return 0
    def vuvsize(self): return 0

    def alignment_columns(self):
        raise ValueError('DurationFeatures has no alignment: durations are per phone, and both sides have the same phones')

    def objmeasures_add(self, DUR, REF):
        """DUR, REF [P, nstates] in frames: the RMSE per state in frames, and per phone (the states summed) the RMSE in ms and the
        correlation (left out for an utterance whose generated or reference phone durations are all equal)."""
        DUR, REF = np.asarray(DUR, dtype=np.float64), np.asarray(REF, dtype=np.float64)
        if DUR.ndim != 2 or DUR.shape[1] != self.nstates or DUR.shape != REF.shape or DUR.shape[0] < 1:
            raise ValueError('objmeasures_add: durations {} and reference {} are not [P,{}]'.format(DUR.shape, REF.shape, self.nstates))
        self.features_err.setdefault('DUR_STATE[frames]', []).append(np.sqrt(np.mean((DUR - REF) ** 2)))
        dms, rms = DUR.sum(axis=1) * self.shift * 1e3, REF.sum(axis=1) * self.shift * 1e3
        self.features_err.setdefault('DUR_PHONE[ms]', []).append(np.sqrt(np.mean((dms - rms) ** 2)))
        if dms.std() > 0 and rms.std() > 0:
            self.features_err.setdefault('DUR_PHONE[corr]', []).append(np.corrcoef(dms, rms)[0, 1])
