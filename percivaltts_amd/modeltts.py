"""ModelTTS: the acoustic-model wrapper (reference: percivaltts/modeltts.py:46-205).

Holds `.ctxsize .vocoder .kerasmodel`; `kerasmodel` keeps its name for drop-in compatibility but is a
percivaltts_amd.layers.Model running on HIP kernels.  predict / count_params / save / load follow
modeltts.py:68-130; the model file trio keeps its stems (`.arch.json`, `.weights.npz` in place of `.weights.h5`
because h5py is not part of this image, `.cfgextras.pkl`).  generate_params is generate_wav (modeltts.py:144-205) up to
the vocoder call: de-normalisation, MLPG on the device (csrc/mlpg.hip), parameter files and objective measures.  The
reference's own waveform needs the vocoder DSP it delegates to and stays out of scope; with `wavdir`
generate_params writes the waveform of the build's own synthesiser for the vocoder's parameters instead (VocoderPML: pulse and noise,
csrc/pulsesynth.hip; VocoderWORLDDevice: periodic plus aperiodic, csrc/worldsynth.hip).
"""
from __future__ import print_function

import os
import pickle
import sys

import numpy as np
import torch

from . import backend_hip
from . import data
from . import networktts
from . import ops


class ModelTTS:

    ctxsize = -1
    vocoder = None
    kerasmodel = None

    def __init__(self, ctxsize, vocoder, kerasmodel=None):
        print("Building the TTS-dedicated model")
        self.ctxsize = ctxsize
        self.vocoder = vocoder
        if kerasmodel is not None:
            self.kerasmodel = kerasmodel
            self.kerasmodel.summary()

    def to_device(self):
        dev = backend_hip.device()
        p = next(self.kerasmodel.parameters(), None)
        if p is None or p.device != dev:
            self.kerasmodel.to(dev)
        return dev

    def predict_device(self, x):
        """predict() without the copy back: numpy [B,T,ctx] -> float32 device tensor [B,T,out]."""
        dev = self.to_device()
        with torch.no_grad():
            xt = torch.as_tensor(np.ascontiguousarray(x), dtype=torch.float32).to(dev)
            return ops.as_tensor(self.kerasmodel(xt, training=False))

    def predict(self, x):
        """Inference forward (BatchNorm uses its moving statistics): numpy [B,T,ctx] -> numpy [B,T,out]."""
        return self.predict_device(x).cpu().numpy()

    def predict_device_batch(self, xs):
        """Ragged inference: `xs` is a list of [T_i, ctx] arrays or tensors of unequal lengths; returns the list of [T_i, out]
        float32 device tensors.  The utterances are zero-padded to the longest and go through ONE forward with a length per row:
        every layer that reads across time (Conv1D, Conv2D, LSTM, GRU) sees zeros behind each row's end, which is what 'same'
        padding shows a lone utterance, and the recurrences walk each row over its own length (layers.ragged_input,
        ops.lstm_infer / gru_infer).  Each result is what predict_device gives for that utterance alone up to the rounding of
        products that run at another row count."""
        if len(xs) == 0:
            return []
        y, _, lens = self.predict_device_padded(xs)
        return [y[i, :lens[i]] for i in range(len(lens))]

    def predict_device_padded(self, xs):
        """predict_device_batch before the results are cut out: (the padded result [B, Tmax, out] with zero pad rows, the lengths as
        the int32 device tensor [B] the forward was given, the same lengths as a list)."""
        dev = self.to_device()
        with torch.no_grad():
            xpad, lengths, lens = data.pad_to_device(xs, dev, 'predict_device_batch')
            return self.kerasmodel(xpad, training=False, memo={'lengths': lengths}), lengths, lens

    def predict_batch(self, xs):
        """predict_device_batch with the results copied back: a list of numpy [T_i, out]."""
        return [y.cpu().numpy() for y in self.predict_device_batch(xs)]

    def count_params(self):
        return self.kerasmodel.count_params()

    def save(self, fmodel, cfg=None, extras=None, printfn=print, infostr=''):
        if extras is None: extras = dict()
        printfn('    saving parameters in {} ...'.format(fmodel), end='')
        sys.stdout.flush()
        with open(fmodel + '.arch.json', 'w') as f:
            f.write(self.kerasmodel.to_json())
        ws = self.kerasmodel.weights()
        np.savez(fmodel + '.weights.npz', **{'w{:04d}'.format(i): t.detach().cpu().numpy() for i, (_, t) in enumerate(ws)})
        with open(fmodel + '.cfgextras.pkl', 'wb') as f:
            pickle.dump([cfg, extras], f)
        print(' done ' + infostr)
        sys.stdout.flush()

    def load(self, fmodel, printfn=print, compile=True):
        printfn('    reloading parameters from {} ...'.format(fmodel), end='')
        sys.stdout.flush()
        if self.kerasmodel is None:
            raise ValueError('the architecture has to be rebuilt from source before loading weights '
                             '(the .arch.json of this build is descriptive only)')
        with np.load(fmodel + '.weights.npz') as z:
            arrays = [z['w{:04d}'.format(i)] for i in range(len(z.files))]
        self.kerasmodel.set_weights(arrays)
        with open(fmodel + '.cfgextras.pkl', 'rb') as f:
            DATA = pickle.load(f)
        print(' done')
        sys.stdout.flush()
        return DATA

    def generate_cmp(self, inpath, outpath, fid_lst):
        """Write the raw network output of each file as headerless float32 [T,out] (modeltts.py:133-141)."""
        if not os.path.isdir(os.path.dirname(outpath)): os.mkdir(os.path.dirname(outpath))
        X = data.load(inpath, fid_lst, verbose=1, label='Context labels: ')
        for vi in range(len(fid_lst)):
            CMP = self.predict(np.reshape(X[vi], [1] + [s for s in X[vi].shape]))[0,]
            CMP.astype('float32').tofile(outpath.replace('*', fid_lst[vi]))

    def _nb_mlpg_wins(self):
        wins = self.vocoder.mlpg_wins
        return len(wins) if wins is not None else 0

    def denormalise(self, CMP, Ymean, Ystd, mlpg_ignore=False):
        """The nested denormalise() of the reference's generate_wav (modeltts.py:163-179): numpy [T, featuressize()] ->
        numpy float32 [T, featuressizeraw()].  CMP*Ystd + Ymean, then, for a vocoder with `mlpg_wins`, either the static columns
        (`mlpg_ignore`: pure numpy) or MLPG with var = Ystd**2 at every frame, solved on the device (ops.mlpg; the
        de-normalisation is then done in fp64 inside the kernel).  Without windows the width is unchanged and no device is
        needed."""
        CMP = np.asarray(CMP, dtype=np.float32)
        Ymean, Ystd = np.asarray(Ymean, dtype=np.float32), np.asarray(Ystd, dtype=np.float32)
        if CMP.ndim != 2 or CMP.shape[1] != self.vocoder.featuressize() or Ymean.shape != (CMP.shape[1],) or Ystd.shape != Ymean.shape:
            raise ValueError('denormalise: CMP {} / mean {} / std {} do not match the vocoder\'s {} features'.format(
                CMP.shape, Ymean.shape, Ystd.shape, self.vocoder.featuressize()))
        if self._nb_mlpg_wins() == 0:
            return CMP * Ystd + Ymean
        ops.mlpg_windows(self.vocoder.mlpg_wins)        # ValueError for windows MLPG cannot use, whichever branch follows
        if mlpg_ignore:
            return (CMP * Ystd + Ymean)[:, :self.vocoder.featuressizeraw()]
        dev = backend_hip.device()
        mean, std = torch.from_numpy(Ymean).to(dev), torch.from_numpy(Ystd).to(dev)
        out = ops.mlpg(torch.from_numpy(np.ascontiguousarray(CMP)).to(dev), self.vocoder.mlpg_wins, std * std, mean=mean, std=std)
        return out.cpu().numpy()

    def _synthesise(self, CMPs, pp_mcep):
        """The waveforms of one batch's generated parameters (device tensors): one synthesis_device_batch call where the vocoder
        has it, its synthesis_device utterance by utterance otherwise.  The two give the same bytes."""
        if hasattr(self.vocoder, 'synthesis_device_batch'):
            return self.vocoder.synthesis_device_batch(CMPs, pp_mcep=pp_mcep)
        return [self.vocoder.synthesis_device(c, pp_mcep=pp_mcep) for c in CMPs]

    def generate_params(self, inpath, outpath, fid_lst, gendir, do_objmeas=True, batch_size=8, pp_mcep=False, specdir=None,
                        *, predict_batched=False, group_by_length=False, objmeas_align=None, wavdir=None):
        """The reference's generate_wav (modeltts.py:144-205) up to the vocoder call: read mean4norm.dat / std4norm.dat beside
        `outpath`, predict each file of `fid_lst`, de-normalise (with MLPG when the vocoder has `mlpg_wins`), write
        `gendir/<fid>.cmp` as headerless float32 [T, featuressizeraw()], and, with `do_objmeas`, feed the vocoder's objective
        measures with (generated, de-normalised target statics), print their statistics and return them (None otherwise).

        With MLPG the network's output tensor stays on the device: it goes into ptts_mlpg with mean / std given, so the
        de-normalisation is fused into the solve's loads, and up to `batch_size` utterances share one launch (zero-padded to
        the longest, each solved over its own length).  The network itself still sees ONE utterance per predict, as in the
        reference: padding would change what a context Conv1D or a BLSTM computes for an utterance's real frames wherever it
        looks across the pad, and the files must not depend on how they were batched.  Only the MLPG launch is batched; its
        systems are independent, so the files are bit-identical for every `batch_size`.

        With `predict_batched` the utterances of each `batch_size` group go through the network together as well
        (predict_device_batch: one forward over the zero-padded group with a length per row, no layer looking across a row's end).
        Each utterance's result is then the lone one up to rounding only -- the products run at another row count and may pick
        another kernel or summation split -- so the files agree with the default's to about 5e-4 relative (times std4norm per
        column), they are not bit-identical, and they can depend on `batch_size`.  Off by default.

        With `group_by_length` (beside `predict_batched`) the groups are made of utterances of similar length (data.length_groups:
        runs of the stable sort by length) instead of consecutive ones, which spares the padded frames of a group whose lengths are
        far apart; the files are written group by group and agree with the consecutive groups' to the same bound.  Off by default.

        With `specdir` each utterance's spectral columns also go through the vocoder's decompress_spectrum(pp_mcep=pp_mcep) while
        they are on the device (csrc/spectrum.hip) and `specdir/<fid>.spec` is written as headerless float32 [T, dftlen/2+1]:
        the envelope a waveform generator reads.  The .cmp files and the measures are what they are without it (the reference,
        too, measures before the post-filter); without `specdir` no spectrum kernel is launched.

        With `wavdir` each batch's generated parameters also go through the vocoder's synthesis_device_batch(pp_mcep=pp_mcep), or
        utterance by utterance through its synthesis_device where it has no batched form (the files are the same either way), while
        they are on the device (csrc/pulsesynth.hip for VocoderPML, csrc/worldsynth.hip for VocoderWORLDDevice) and `wavdir/<fid>.wav` is written as 16-bit PCM at the vocoder's fs; the noise
        comes from the library's generator (ops.rng_seed).  The .cmp and .spec files are what they are without it.  A vocoder
        without synthesis_device (VocoderWORLD itself among them) is a ValueError.

        With `objmeas_align='dtw'` (and `do_objmeas`) the inputs and the targets keep their own lengths -- no data.croplen, so the
        generated files are bit for bit those of do_objmeas=False -- and each utterance is measured along its DTW path to its target:
        the generated parameters of a batch group (still on the device where MLPG leaves them there) and the de-normalised targets
        go through ONE ops.dtw_align per group, over the vocoder's alignment_columns() (csrc/dtw.hip), and the
        measures are fed through objmeasures_add_aligned(..., path=...): the keys of objmeasures_add, now along the path, plus
        'DTW[cost/step]' and 'DTW[len ratio]'.  This is what measures inputs whose lengths are not the targets', e.g. those
        expanded from predicted durations.  None: as ever, croplen included.  Any other value is a ValueError."""
        if objmeas_align not in (None, 'dtw'):
            raise ValueError('objmeas_align={!r} is not None or \'dtw\''.format(objmeas_align))
        align = objmeas_align == 'dtw' and do_objmeas
        if align:
            a0, a1, ascale = self.vocoder.alignment_columns()      # ValueError for features without an alignment
        Ymean = np.fromfile(os.path.join(os.path.dirname(outpath), 'mean4norm.dat'), dtype='float32')
        Ystd = np.fromfile(os.path.join(os.path.dirname(outpath), 'std4norm.dat'), dtype='float32')
        nout, nraw = self.vocoder.featuressize(), self.vocoder.featuressizeraw()
        if Ymean.shape != (nout,) or Ystd.shape != (nout,):
            raise ValueError('mean4norm.dat / std4norm.dat hold {} / {} values, the vocoder has {} features'.format(
                Ymean.size, Ystd.size, nout))
        use_mlpg = self._nb_mlpg_wins() > 0
        if use_mlpg: ops.mlpg_windows(self.vocoder.mlpg_wins)
        if batch_size < 1: raise ValueError('batch_size has to be at least 1')

        X_test = data.load(inpath, fid_lst, verbose=1, label='Context labels: ')
        if do_objmeas:
            y_test = data.load(outpath, fid_lst, verbose=1, label='Output features: ')
            if not align:
                X_test, y_test = data.croplen((X_test, y_test))
            self.vocoder.objmeasures_clear()
        if not os.path.isdir(gendir): os.makedirs(gendir)
        if specdir is not None:
            if not hasattr(self.vocoder, 'decompress_spectrum'):
                raise ValueError('specdir given, but the vocoder {} has no spectral envelope to decompress'.format(self.vocoder.name()))
            if not os.path.isdir(specdir): os.makedirs(specdir)
            s0, s1 = 1, 1 + self.vocoder.specsize()
        if wavdir is not None:
            if not hasattr(self.vocoder, 'synthesis_device'):
                raise ValueError('wavdir given, but the vocoder {} has no waveform synthesis in this build'.format(self.vocoder.name()))
            from . import vocoders
            if not os.path.isdir(wavdir): os.makedirs(wavdir)

        if use_mlpg:
            dev = self.to_device()
            mean, std = torch.from_numpy(Ymean).to(dev), torch.from_numpy(Ystd).to(dev)
            var = std * std                 # "Simplification!" (modeltts.py:176): the global variance at every frame
        if group_by_length and not predict_batched:
            raise ValueError('group_by_length groups the batches of predict_batched: set both')
        for vis in data.length_groups([x.shape[0] for x in X_test], batch_size, sort=bool(group_by_length)):
            if predict_batched:
                print('Generating {}-{}/{} ...'.format(1 + vis[0], 1 + vis[-1], len(fid_lst)))
                ys = self.predict_device_batch([X_test[vi] for vi in vis])
            else:
                ys = []
                for vi in vis:
                    print('Generating {}/{} fid={} ...'.format(1 + vi, len(fid_lst), fid_lst[vi]))
                    ys.append(self.predict_device(np.reshape(X_test[vi], [1] + [s for s in X_test[vi].shape]))[0])
            for y in ys:
                if y.shape[-1] != nout:
                    raise ValueError('the model predicts {} features, the vocoder expects {}'.format(y.shape[-1], nout))
            if use_mlpg:
                lens = [int(y.shape[0]) for y in ys]
                if len(ys) == 1:
                    gen = ops.mlpg(ys[0].contiguous(), self.vocoder.mlpg_wins, var, mean=mean, std=std).unsqueeze(0)
                else:
                    ypad = torch.zeros((len(ys), max(lens), nout), dtype=torch.float32, device=dev)
                    for i, y in enumerate(ys): ypad[i, :lens[i]] = y
                    gen = ops.mlpg(ypad, self.vocoder.mlpg_wins, var, mean=mean, std=std,
                                   lengths=torch.tensor(lens, dtype=torch.int32, device=dev))
                if specdir is not None:
                    specs = [self.vocoder.decompress_spectrum(gen[i, :lens[i], s0:s1], pp_mcep=pp_mcep) for i in range(len(ys))]
                if wavdir is not None:
                    wavs = self._synthesise([gen[i, :lens[i]] for i in range(len(ys))], pp_mcep)
                if align:
                    gen_rows = torch.cat([gen[i, :lens[i]] for i in range(len(ys))])
                gen = gen.cpu().numpy()
                CMPs = [gen[i, :lens[i]] for i in range(len(ys))]
            else:
                CMPs = [self.denormalise(y.cpu().numpy(), Ymean, Ystd) for y in ys]
                if specdir is not None:     # the .cmp values themselves, back on the device
                    specs = [self.vocoder.decompress_spectrum(torch.from_numpy(np.ascontiguousarray(c[:, s0:s1])).to(self.to_device()),
                                                              pp_mcep=pp_mcep) for c in CMPs]
                if wavdir is not None:
                    wavs = self._synthesise([torch.from_numpy(np.ascontiguousarray(c, dtype=np.float32)).to(self.to_device()) for c in CMPs],
                                            pp_mcep)
                if align:
                    gen_rows = torch.from_numpy(np.ascontiguousarray(np.concatenate(CMPs), dtype=np.float32)).to(self.to_device())
            if align:                       # one alignment for the group; the paths and costs come back with two downloads
                REFs = [self.denormalise(y_test[vi], Ymean, Ystd, mlpg_ignore=True) for vi in vis]
                ref_rows = torch.from_numpy(np.ascontiguousarray(np.concatenate(REFs), dtype=np.float32)).to(gen_rows.device)
                ali = ops.dtw_align(gen_rows.contiguous(), ref_rows, [c.shape[0] for c in CMPs], [r.shape[0] for r in REFs],
                                    cols=(a0, a1), scale=ascale)
                paths, costs = ali.host(), ali.cost.cpu().numpy()
            if specdir is not None:
                for vi, spec in zip(vis, specs):
                    spec.cpu().numpy().tofile(os.path.join(specdir, fid_lst[vi] + '.spec'))
            if wavdir is not None:
                for vi, wav in zip(vis, wavs):
                    vocoders.wavwrite(os.path.join(wavdir, fid_lst[vi] + '.wav'), wav, self.vocoder.fs)
            for gi, (vi, CMP) in enumerate(zip(vis, CMPs)):
                CMP = np.ascontiguousarray(CMP, dtype=np.float32)
                assert CMP.shape[1] == nraw
                CMP.tofile(os.path.join(gendir, fid_lst[vi] + '.cmp'))
                if align:
                    self.vocoder.objmeasures_add_aligned(CMP, REFs[gi], path=paths[gi] + (costs[gi],))
                elif do_objmeas:
                    self.vocoder.objmeasures_add(CMP, self.denormalise(y_test[vi], Ymean, Ystd, mlpg_ignore=True))
        stats = self.vocoder.objmeasures_stats() if do_objmeas else None
        print('Generation finished')
        sys.stdout.flush()
        return stats

    def generate_wav(self, *args, **kwargs):
        """The reference's name promises pulsemodel's (or pyworld's) waveform, which this build does not have.  The build's own
        synthesiser is reached through generate_params(..., wavdir=...)."""
        raise NotImplementedError('waveform synthesis needs the vocoder DSP (pulsemodel/pyworld), outside this build; '
                                  'generate_params writes the de-normalised (MLPG) parameters a vocoder would read')
