"""The acoustic models of the reference (percivaltts/modeltts_common.py:36-126) on the HIP layer graph."""
from __future__ import print_function

from . import layers as kl
from . import modeltts
from . import networktts


class Generic(modeltts.ModelTTS):
    """Stack of `network_generic` layers + the vocoder's output heads (modeltts_common.py:36-58)."""
    def __init__(self, ctxsize, vocoder, fmodel=None, layertypes=['FC', 'FC', 'FC'], nameprefix=None, cfgarch=None):
        modeltts.ModelTTS.__init__(self, ctxsize, vocoder)
        if nameprefix is None: nameprefix = ''
        l_in = kl.Input(shape=(None, ctxsize), name=nameprefix + 'input.conditional')
        l_out = networktts.network_generic(l_in, layertypes=layertypes, cfgarch=cfgarch)
        l_out = networktts.network_final(l_out, vocoder, mlpg_wins=vocoder.mlpg_wins)
        self.kerasmodel = kl.Model(inputs=l_in, outputs=l_out)
        if fmodel is not None:
            self.load(fmodel)
        self.kerasmodel.summary()


class DCNNF0SpecNoiseFeatures(modeltts.ModelTTS):
    """The PercivalTTS model (modeltts_common.py:61-126): context Conv1D + 2 FC, then
    f0: BLSTM -> Dense(1);  spec: Dense(F) -> L x (Conv2D + BN + LeakyReLU) -> Conv2D(1);  noise: L//2 FC -> sigmoid."""
    def __init__(self, ctxsize, vocoder, cfgarch, nameprefix=None):
        modeltts.ModelTTS.__init__(self, ctxsize, vocoder)
        if nameprefix is None: nameprefix = ''

        l_in = kl.Input(shape=(None, ctxsize), name=nameprefix + 'input.conditional')

        l_ctx = l_in
        for _ in range(cfgarch.arch_ctx_nbcnnlayers):
            l_ctx = networktts.pCNN1D(l_ctx, cfgarch.arch_hiddenwidth, cfgarch.arch_ctx_winlen)
        l_ctx = networktts.pFC(l_ctx, cfgarch.arch_hiddenwidth)
        l_ctx = networktts.pFC(l_ctx, cfgarch.arch_hiddenwidth)

        # F0
        l_f0 = networktts.pBLSTM(l_ctx, width=cfgarch.arch_hiddenwidth)
        l_f0.stream = 1           # independent, latency-bound branch: may run on a side HIP stream (layers.Model._run)
        l_f0 = kl.Dense(1, activation=None, use_bias=True)(l_f0)
        l_f0.stream = 1

        # Spec
        l_spec = kl.Dense(vocoder.specsize(), use_bias=True)(l_ctx)   # projection
        l_spec = kl.Reshape([vocoder.specsize(), 1])(l_spec)          # channels after the spectral dimension
        gated = bool(getattr(cfgarch, 'arch_gen_gated', False))       # build extension (BASELINE config 5)
        dils = getattr(cfgarch, 'arch_gen_dilations', None)
        for li in range(cfgarch.arch_gen_nbcnnlayers):
            if gated:
                kw = {'dil_t': dils[li % len(dils)] if dils else 1, 'causal': bool(getattr(cfgarch, 'arch_gen_causal', False))}
                l_spec = networktts.pGCNN2D(l_spec, cfgarch.arch_gen_nbfilters, cfgarch.arch_gen_winlen, cfgarch.arch_spec_freqlen, **kw)
            else:
                l_spec = networktts.pCNN2D(l_spec, cfgarch.arch_gen_nbfilters, cfgarch.arch_gen_winlen, cfgarch.arch_spec_freqlen)
        # (the causal variant keeps its output layer causal too, so that the whole spectral stack looks only backwards)
        l_spec = kl.Conv2D(1, [cfgarch.arch_gen_winlen, cfgarch.arch_spec_freqlen], use_bias=True, activation=None,
                           causal=gated and bool(getattr(cfgarch, 'arch_gen_causal', False)))(l_spec)
        l_spec = kl.Reshape([l_spec.shape[-2]])(l_spec)

        # NM
        l_nm = l_ctx
        for _ in range(cfgarch.arch_gen_nbcnnlayers // 2):   # integer division as in the Python-2 reference (:119)
            l_nm = networktts.pFC(l_nm, cfgarch.arch_hiddenwidth)
        l_nm = kl.Dense(vocoder.noisesize(), activation='sigmoid')(l_nm)

        heads = [l_f0, l_spec, l_nm]
        # Build extension: the reference's DCNN has no delta heads, so with a vocoder built with `mlpg_wins` its output would be
        # narrower than the composed features.  Here the delta (and delta-delta) streams get the heads network_final gives the
        # Generic model (networktts.py:201-208), fed by the context: linear f0+spec, tanh resp. 2*tanh noise mask.
        nwins = len(vocoder.mlpg_wins) if vocoder.mlpg_wins is not None else 0
        for wi, (prefix, nm_act) in enumerate((('lo_delta', 'tanh'), ('lo_deltadelta', ('tanh_saturated', 2.0)))[:nwins]):
            heads.append(kl.Dense(1 + vocoder.specsize(), activation=None, name=prefix + '_f0spec')(l_ctx))
            heads.append(kl.Dense(vocoder.noisesize(), activation=nm_act, name=prefix + '_nm')(l_ctx))
        l_out = kl.Concatenate()(heads)

        # handles for the critic step, which only needs the spectral branch (the critic slices it, networks_critic.py:58)
        self.node_spec, self.node_f0, self.node_nm = l_spec, l_f0, l_nm

        self.kerasmodel = kl.Model(inputs=l_in, outputs=l_out)
        self.kerasmodel.summary()


class DurationModel(modeltts.ModelTTS):
    """Duration model: a `network_generic` stack and one linear Dense(nstates) over phone-level inputs
    (label_normalisation.HTSDurationLabelNormalisation).  The time axis is the phone index, so everything that trains or runs an
    acoustic model on [B,T,ctx] batches (OptimizerTTS, 'randshiftpad' included; predict_device_batch) takes it as it is; the
    output features are vocoders.DurationFeatures: `nstates` durations per phone, mean/std normalised, in frames of
    cfgarch.vocoder_shift seconds (5 ms when cfgarch has none)."""

    def __init__(self, ctxsize, cfgarch, layertypes=['FC', 'BLSTM'], nstates=5, nameprefix=None):
        from . import vocoders
        modeltts.ModelTTS.__init__(self, ctxsize, vocoders.DurationFeatures(getattr(cfgarch, 'vocoder_shift', 0.005), nstates))
        if nameprefix is None: nameprefix = ''
        l_in = kl.Input(shape=(None, ctxsize), name=nameprefix + 'input.phones')
        l_out = networktts.network_generic(l_in, layertypes=layertypes, cfgarch=cfgarch)
        l_out = kl.Dense(nstates, activation=None, use_bias=True, name='lo_durations')(l_out)
        self.kerasmodel = kl.Model(inputs=l_in, outputs=l_out)
        self.kerasmodel.summary()

    def generate_durations(self, inpath, outpath, fid_lst, durdir, do_objmeas=True, batch_size=8, min_frames=1, max_frames=None):
        """Predict the durations of every file of `fid_lst` in batches of `batch_size` utterances (predict_device_batch: one
        forward over the padded batch with a length per row), de-normalise them with mean4norm.dat / std4norm.dat beside
        `outpath`, round them to whole frames -- at least `min_frames`, by the rule and in the kernel of ops.labels_segments, so
        that the rows label_normalisation.normalise_with_durations expands are these durations' -- and write `durdir/<fid>.dur`
        as headerless float32 [P, nstates].  With `do_objmeas` the de-normalised targets of `outpath` feed the measures
        (vocoders.DurationFeatures.objmeasures_add); their statistics are printed and returned (None otherwise).  `nstates` is 5
        or 1 here, the widths the kernel takes."""
        import os

        import numpy as np
        import torch

        from . import data, ops
        from .external.merlin import label_normalisation
        nst = self.vocoder.nstates
        if nst not in (ops.LABELS_SEG_STATES, 1):
            raise ValueError('generate_durations: durations of {} states; ops.labels_segments takes {} or 1'.format(nst, ops.LABELS_SEG_STATES))
        if batch_size < 1: raise ValueError('batch_size has to be at least 1')
        max_frames = label_normalisation.DUR_MAX_FRAMES if max_frames is None else max_frames
        Ymean = np.fromfile(os.path.join(os.path.dirname(outpath), 'mean4norm.dat'), dtype='float32')
        Ystd = np.fromfile(os.path.join(os.path.dirname(outpath), 'std4norm.dat'), dtype='float32')
        if Ymean.shape != (nst,) or Ystd.shape != (nst,):
            raise ValueError('mean4norm.dat / std4norm.dat hold {} / {} values, the model predicts {} durations'.format(Ymean.size, Ystd.size, nst))
        X_test = data.load(inpath, fid_lst, verbose=1, label='Phone labels: ')
        if do_objmeas:
            y_test = data.load(outpath, fid_lst, verbose=1, label='Durations: ')
            self.vocoder.objmeasures_clear()
        if not os.path.isdir(durdir): os.makedirs(durdir)
        dev = self.to_device()
        mean, std = torch.from_numpy(Ymean).to(dev), torch.from_numpy(Ystd).to(dev)
        for vis in data.length_groups([x.shape[0] for x in X_test], batch_size, sort=False):
            print('Generating durations {}-{}/{} ...'.format(1 + vis[0], 1 + vis[-1], len(fid_lst)))
            ys = self.predict_device_batch([X_test[vi] for vi in vis])
            dur = (torch.cat(ys) * std + mean).contiguous()
            off = np.zeros(len(vis) + 1, dtype=np.int64)
            np.cumsum([int(y.shape[0]) for y in ys], out=off[1:])
            seg, _, _ = ops.labels_segments(dur, torch.from_numpy(off.astype(np.int32)).to(dev), min_frames, max_frames)
            frames = seg[:, 2].reshape(-1, nst).to(torch.float32).cpu().numpy()
            for i, vi in enumerate(vis):
                DUR = np.ascontiguousarray(frames[off[i]:off[i + 1]])
                DUR.tofile(os.path.join(durdir, fid_lst[vi] + '.dur'))
                if do_objmeas:
                    n = min(len(DUR), len(y_test[vi]))
                    self.vocoder.objmeasures_add(DUR[:n], y_test[vi][:n] * Ystd + Ymean)
        stats = self.vocoder.objmeasures_stats() if do_objmeas else None
        print('Duration generation finished')
        return stats
