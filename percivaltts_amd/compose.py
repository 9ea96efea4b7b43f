"""Feature composition -- the forward counterpart of generation: concatenate the feature streams of every utterance, append
delta windows, estimate the corpus statistics, normalise, and write what `data.load` reads and what
`ModelTTS.generate_params` de-normalises (mean4norm.dat / std4norm.dat).

Same function names, arguments and files as the reference's percivaltts/compose.py:34-455.  The reference sweeps the files three
times in numpy, one column at a time through scipy.signal.convolve; here each sweep over a chunk of utterances is one launch of
csrc/compose.hip (ops.compose_windows, ops.compose_sqdev, ops.compose_normalise).  There is no CPU path: without a device
`compose` and the normalisers raise HipLibraryError.  The time-weight functions are per-frame scalar work and stay host numpy,
like data.py.

Data flow of `compose`: every raw file is read once and concatenated on the host into a pinned staging buffer, a chunk of
utterances (CHUNK_BYTES of composed rows) goes to the device packed row-wise with an offsets array, and the composed chunk stays
there.  If the whole composed corpus fits under DEVICE_CAP_BYTES (the *resident* route) the standard-deviation pass and the
normaliser run from device memory and, with one of this module's normalisers, only the final files are written.  Above the cap
(the *streamed* route) the reference's own sequence is followed through the files in chunks: write composed, re-read for the
standard deviation, re-read for the normalisation.  Both routes write byte-identical files: the kernels' statistics are added
in utterance order from per-utterance partials, so they do not depend on where the chunks were cut.
"""
from __future__ import print_function

import datetime
import os
import re

import numpy as np

from . import data
from .percivaltts import makedirs, print_tty, readids

DEVICE_CAP_BYTES = 8 << 30      # a composed corpus up to this size is kept in device memory between the passes
CHUNK_BYTES = 256 << 20         # composed bytes of one staged chunk of utterances (never more than DEVICE_CAP_BYTES)


# ---------------------------------------------------------------------------------------------------------------------------
# device plumbing
# ---------------------------------------------------------------------------------------------------------------------------
def _device():
    import torch
    from . import _hip
    if not torch.cuda.is_available():
        raise _hip.HipLibraryError('compose runs on the device (csrc/compose.hip) and no device is available; there is no CPU path')
    _hip.lib()
    return torch.device('cuda', torch.cuda.current_device())


class _Stage(object):
    """One growing pinned host buffer: files are read into it, the chunk goes to the device from it."""

    def __init__(self):
        self.buf = None

    def rows(self, R, W):
        import torch
        n = max(int(R) * int(W), 1)
        if self.buf is None or self.buf.numel() < n:
            self.buf = torch.empty(n, dtype=torch.float32).pin_memory()
        return self.buf[:int(R) * int(W)].view(int(R), int(W))


def _to_device(host, dev):
    """Pinned [R,W] -> device; the stream is synchronised so that the staging buffer can be refilled."""
    import torch
    t = torch.empty(host.shape, dtype=torch.float32, device=dev)
    t.copy_(host, non_blocking=True)
    torch.cuda.current_stream().synchronize()
    return t


def _offsets(lens, dev):
    import torch
    offs = np.zeros(len(lens) + 1, dtype=np.int64)
    np.cumsum(lens, out=offs[1:])
    if offs[-1] >= 1 << 31:
        raise ValueError('a chunk of {} frames exceeds the int32 offsets: lower compose.CHUNK_BYTES'.format(offs[-1]))
    return offs, torch.from_numpy(offs.astype(np.int32)).to(dev)


def _chunks(lens, rowbytes, budget):
    """Consecutive file ranges [i0, i1) whose rows fit `budget` bytes (one file at least)."""
    out, i0, used = [], 0, 0
    for i, n in enumerate(lens):
        need = int(n) * rowbytes
        if i > i0 and used + need > budget:
            out.append((i0, i))
            i0, used = i, 0
        used += need
    if i0 < len(lens):
        out.append((i0, len(lens)))
    return out


def _budget():
    return max(1, min(CHUNK_BYTES, DEVICE_CAP_BYTES))


def _write_rows(rows, offs, outfilepath, fids):
    for i, fid in enumerate(fids):
        rows[offs[i]:offs[i + 1]].tofile(outfilepath.replace('*', fid))


def _file_rows(path, width):
    nbytes = os.path.getsize(path)
    if nbytes % (4 * width) != 0:
        raise ValueError('{}: {} bytes is not a whole number of float32 rows of {}'.format(path, nbytes, width))
    return nbytes // (4 * width)


def _load_files(filepath, fids, width, stage, dev):
    """Headerless float32 [*, width] files of `fids` -> packed device rows, host offsets, device offsets."""
    lens = [_file_rows(filepath.replace('*', fid), width) for fid in fids]
    offs, offs_d = _offsets(lens, dev)
    host = stage.rows(offs[-1], width)
    hv = host.numpy()
    for i, fid in enumerate(fids):
        hv[offs[i]:offs[i + 1]] = np.fromfile(filepath.replace('*', fid), dtype='float32').reshape(-1, width)
    return _to_device(host, dev), offs, offs_d


# ---------------------------------------------------------------------------------------------------------------------------
# normalisers (compose.py:34-183)
# ---------------------------------------------------------------------------------------------------------------------------
def _as_keepidx(keepidx, n):
    """None when `keepidx` is absent or the identity (no gather needed), else an int32 array."""
    if keepidx is None:
        return None
    keepidx = np.asarray(keepidx)
    if len(keepidx) == n and (keepidx == np.arange(n)).all():
        return None
    return keepidx.astype(np.int32)


def _plan_minmax(mins, maxs, outdir, nrange, keepidx, zerovarstozeros):
    from . import ops_offline as ops
    if nrange is None: nrange = [-1, 1]
    orisize = len(maxs)
    kidx = np.arange(len(mins)) if keepidx is None else np.asarray(keepidx)
    mins = mins[kidx].astype('float32')
    maxs = maxs[kidx].astype('float32')
    # the statistics the normalisation uses, as they are BEFORE the dead dimensions are patched
    mins.tofile(os.path.join(outdir, 'min4norm.dat'))
    maxs.tofile(os.path.join(outdir, 'max4norm.dat'))
    diff = maxs - mins
    if zerovarstozeros:
        mins[diff == 0.0] = 0.0         # a dead column is centred and scaled from its own value, not pinned to the range's low end
    diff[diff == 0.0] = 1.0
    return dict(width=orisize, mode=ops.NORM_MINMAX, a=mins, b=diff, scale=(nrange[1] - nrange[0]) / 2.0,
                offset=0.5 * (nrange[0] + nrange[1]), keepidx=_as_keepidx(keepidx, orisize))


def _plan_meanstd(means, stds, outdir, noise_slices=()):
    from . import ops_offline as ops
    means = means.astype('float32')
    stds = stds.astype('float32')
    for sl in noise_slices:             # _nmnoscale: the noise columns pass through untouched
        means[sl] = 0.0
        stds[sl] = 1.0
    means.tofile(os.path.join(outdir, 'mean4norm.dat'))
    stds.tofile(os.path.join(outdir, 'std4norm.dat'))
    stds = stds.copy()
    stds[stds == 0.0] = 1.0             # divide a constant column by 1; the saved std stays 0 (de-normalisation crushes it)
    return dict(width=len(means), mode=ops.NORM_MEANSTD, a=means, b=stds, scale=1.0, offset=0.0, keepidx=None)


def _noise_slices(featurepaths, n):
    """Column ranges of the third feature (the PML noise mask) in the statics and in up to two window streams."""
    f0size, specsize, nmsize = (data.getlastdim(featurepaths[i]) for i in range(3))
    raw = f0size + specsize + nmsize
    print('    sizes f0:{} spec:{} noise:{}'.format(f0size, specsize, nmsize))
    out = [slice(f0size + specsize, raw)]
    if n > raw:
        out.append(slice(raw + f0size + specsize, 2 * raw))
        if n > 2 * raw:
            out.append(slice(2 * raw + f0size + specsize, 3 * raw))
    return out


def _plan_device(plan, dev):
    import torch
    t = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    return t(plan['a']), t(plan['b']), t(plan['keepidx'])


def _normalise_files(plan, filepath, fids, outfilepath):
    """The files of `fids` through ptts_compose_normalise, a chunk at a time."""
    from . import ops_offline as ops
    dev = _device()
    a, b, kidx = _plan_device(plan, dev)
    width = plan['width']
    lens = [_file_rows(filepath.replace('*', fid), width) for fid in fids]
    stage = _Stage()
    for i0, i1 in _chunks(lens, 4 * width, _budget()):
        print_tty('\r    Write normed data files {}-{}/{}                '.format(1 + i0, i1, len(fids)))
        if sum(lens[i0:i1]) == 0:
            for fid in fids[i0:i1]: np.zeros(0, dtype='float32').tofile(outfilepath.replace('*', fid))
            continue
        y, offs, _ = _load_files(filepath, fids[i0:i1], width, stage, dev)
        out = ops.compose_normalise(y, a, b, mode=plan['mode'], scale=plan['scale'], offset=plan['offset'], keepidx=kidx,
                                    out=y if kidx is None else None)
        _write_rows(out.cpu().numpy(), offs, outfilepath, fids[i0:i1])
    print_tty('\r                                                           \r')


def _normalise_entry(what, filepath, outfilepath):
    print('Normalise data using {} (in={}, out={})'.format(what, filepath, outfilepath))
    if outfilepath is None:
        outfilepath = filepath
        print('Overwrite files in {}'.format(filepath))
    _device()
    if not os.path.isdir(os.path.dirname(outfilepath)): os.mkdir(os.path.dirname(outfilepath))
    return outfilepath


def _stat(filepath, name):
    return np.fromfile(os.path.join(os.path.dirname(filepath), name), dtype='float32')


def normalise_minmax(filepath, fids, outfilepath=None, featurepaths=None, nrange=None, keepidx=None, zerovarstozeros=True, verbose=1):
    """Normalisation function for compose(.): [min, max] of every column (min.dat, max.dat beside `filepath`) to `nrange`
    ([-1, 1] by default), with the column selection `keepidx`; writes min4norm.dat / max4norm.dat beside `outfilepath`."""
    outfilepath = _normalise_entry('min and max values to {}'.format([-1, 1] if nrange is None else nrange), filepath, outfilepath)
    plan = _plan_minmax(_stat(filepath, 'min.dat'), _stat(filepath, 'max.dat'), os.path.dirname(outfilepath), nrange, keepidx,
                        zerovarstozeros)
    _normalise_files(plan, filepath, fids, outfilepath)


def normalise_meanstd(filepath, fids, outfilepath=None, featurepaths=None, keepidx=None, verbose=1):
    """Normalisation function for compose(.): mean and standard deviation of every column to 0 and 1 (mean.dat, std.dat beside
    `filepath`); writes mean4norm.dat / std4norm.dat.  As in the reference, `keepidx` is accepted and not used."""
    outfilepath = _normalise_entry('mean and standard-deviation', filepath, outfilepath)
    plan = _plan_meanstd(_stat(filepath, 'mean.dat'), _stat(filepath, 'std.dat'), os.path.dirname(outfilepath))
    _normalise_files(plan, filepath, fids, outfilepath)


def normalise_meanstd_nmnoscale(filepath, fids, outfilepath=None, featurepaths=None, keepidx=None, verbose=1):
    """As normalise_meanstd, except that the third feature of `featurepaths` (the noise mask of the PML vocoder) is left in
    [0, 1]: its mean is forced to 0 and its std to 1, in the statics and in every window stream (up to two)."""
    outfilepath = _normalise_entry('mean and standard-deviation (without normalising the 3rd feature)', filepath, outfilepath)
    means = _stat(filepath, 'mean.dat')
    plan = _plan_meanstd(means, _stat(filepath, 'std.dat'), os.path.dirname(outfilepath), _noise_slices(featurepaths, len(means)))
    _normalise_files(plan, filepath, fids, outfilepath)


def normalise_minmax_stored(rows, statsdir, nrange=None, zerovarstozeros=True):
    """Device rows [T, W] through the min-max normalisation whose statistics normalise_minmax stored in `statsdir` (min4norm.dat,
    max4norm.dat): what that call wrote for its own files, for rows that were not among them -- context rows built at generation
    time.  The statistics are read, never recomputed or rewritten.  Returns a new device tensor."""
    from . import ops_offline as ops
    import torch
    mins, maxs = _stat(os.path.join(statsdir, 'x'), 'min4norm.dat'), _stat(os.path.join(statsdir, 'x'), 'max4norm.dat')
    if rows.dim() != 2 or mins.shape != (rows.shape[1],) or maxs.shape != mins.shape:
        raise ValueError('min4norm.dat / max4norm.dat of {} hold {} / {} values, the rows are {}'.format(statsdir, mins.size, maxs.size, tuple(rows.shape)))
    if nrange is None: nrange = [-1, 1]
    diff = maxs - mins
    if zerovarstozeros:
        mins[diff == 0.0] = 0.0
    diff[diff == 0.0] = 1.0
    if rows.shape[0] == 0:
        return rows.clone()
    return ops.compose_normalise(rows, torch.from_numpy(mins).to(rows.device), torch.from_numpy(diff).to(rows.device), mode=ops.NORM_MINMAX,
                                 scale=(nrange[1] - nrange[0]) / 2.0, offset=0.5 * (nrange[0] + nrange[1]))


# ---------------------------------------------------------------------------------------------------------------------------
# compose (compose.py:186-362)
# ---------------------------------------------------------------------------------------------------------------------------
def _feature_specs(featurepaths):
    specs = []
    for featurepath in featurepaths:
        path, shape = data.getpathandshape(featurepath)
        if shape is None: shape = (-1, 1)
        width = 1
        for d in shape[1:]: width *= int(d)
        specs.append((path, width))
    return specs


def _scan_lengths(specs, fids, minframes):
    """Frames of every utterance: the shortest of its streams, from the file sizes alone."""
    lens = []
    for fid in fids:
        n, short = None, None
        for path, width in specs:
            f = path.replace('*', fid)
            if not os.path.isfile(f):
                raise ValueError('{} does not exists'.format(f))
            rows = _file_rows(f, width)
            if n is None or rows < n: n, short = rows, f
        if n < minframes:
            raise ValueError('{} has {} frames: {}'.format(short, n, 'a three-tap window needs at least 3' if minframes > 1
                                                            else 'an utterance needs at least one'))
        lens.append(int(n))
    return lens


def _load_raw(specs, fids, lens, stage, dev):
    """Each raw file once: streams cropped to the utterance's length and laid side by side in the staging buffer."""
    D = sum(w for _, w in specs)
    offs, offs_d = _offsets(lens, dev)
    host = stage.rows(offs[-1], D)
    hv = host.numpy()
    for i, fid in enumerate(fids):
        c0, T = 0, lens[i]
        for path, width in specs:
            a = np.fromfile(path.replace('*', fid), dtype='float32').reshape(-1, width)
            hv[offs[i]:offs[i + 1], c0:c0 + width] = a[:T]
            c0 += width
    return _to_device(host, dev), offs, offs_d


def _device_stats(chunks_of, nbframes, W, dev):
    """Statistics of packed device chunks [(rows, device offsets, utterances that count)] through the composition kernels:
    min, max (fp32), mean and sum of squared deviations (fp64)."""
    import torch
    from . import ops_offline as ops
    stats = ops.compose_stats_buffers(W, dev)
    for rows, offs_d, ns in chunks_of():
        if ns > 0: ops.compose_windows(rows, offs_d, None, stats=stats, n_stat_utts=ns)
    means = stats[2].cpu().numpy() / nbframes
    mean_d = torch.from_numpy(means).to(dev)
    sq = torch.zeros(W, dtype=torch.float64, device=dev)
    for rows, offs_d, ns in chunks_of():
        if ns > 0: ops.compose_sqdev(rows, offs_d, mean_d, sq, ns)
    return stats[0].cpu().numpy(), stats[1].cpu().numpy(), means, sq.cpu().numpy()


def compose(featurepaths, fids, outfilepath, wins=None, id_valid_start=-1, normfn=None, shift=0.005, dropzerovardims=False,
            do_finalcheck=False, verbose=1, win_convention='reference'):
    """For each file id of `fids`, concatenate the features of `featurepaths` (cropped to the shortest; a path without a shape is
    `(-1,1)`), append one stream per window of `wins`, and write one headerless float32 file `outfilepath` (a shape suffix is
    ignored), normalised by `normfn` from the statistics of the first `id_valid_start` files.  Beside the files: min.dat,
    max.dat, mean.dat, std.dat (unbiased, all float32), keepidx.dat (int32, with `dropzerovardims`) and what the normaliser
    writes (*4norm.dat).

    wins : three-tap windows, e.g. Merlin's [[-0.5, 0.0, 0.5], [1.0, -2.0, 1.0]].
    win_convention : 'reference' (default) reproduces the reference: stream[t] = -scipy.signal.convolve(y, w), i.e.
        -(w[0]*y[t+1] + w[1]*y[t] + w[2]*y[t-1]).  This equals the operator W_k y that MLPG (external/merlin/mlpg_fast.py,
        csrc/mlpg.hip) inverts ONLY for an antisymmetric window such as [-0.5, 0, 0.5]; for [1, -2, 1] it is its negative, for an
        asymmetric window its negated mirror.  'mlpg' applies W_k itself, w[0]*y[t-1] + w[1]*y[t] + w[2]*y[t+1]: it is the
        convention whose output `ops.mlpg` / `ModelTTS.generate_params` turn back into the static trajectory.
        In both, frame 0 repeats frame 1 and the last frame repeats the one before it.
    normfn : None, one of this module's normalisers, or any callable with the reference's protocol: it finds the composed files
        and statistics on disk and is called as normfn(outfilepath, fids, featurepaths=..., keepidx=..., verbose=...).

    Where the reference would crash this raises ValueError: id_valid_start <= 0 (the default -1 included), a window that has
    not three taps, an utterance shorter than 3 frames when there are windows.  A column counts as zero-variance when its
    float32 min and max are equal.

    Returns a dict: 'min', 'max' (float32), 'mean', 'std' (the float64 values before the cast to the files), 'sqdev' (the
    float64 sum of squared deviations under 'std'), 'nbframes',
    'keepidx', 'size', 'resident' and, with `do_finalcheck`, 'finalcheck': the statistics of what was written for the first
    `id_valid_start` files, recomputed with the same kernels ('verif_min', 'verif_max', 'verif_means', and 'verif_stds', which
    as in the reference is the unbiased VARIANCE)."""
    from . import ops_offline as ops
    print('Compose data (id_valid_start={})'.format(id_valid_start))
    if id_valid_start <= 0:
        raise ValueError('id_valid_start has to be greater than zero, i.e. training set has to contain at least one sample, '
                         'otherwise data statistics cannot be estimated.')
    if win_convention not in ('reference', 'mlpg'):
        raise ValueError("win_convention is 'reference' or 'mlpg', got {!r}".format(win_convention))
    wins = [] if wins is None else [list(w) for w in wins]
    ops.compose_window_taps(wins)
    fids = list(fids)
    if len(fids) == 0:
        raise ValueError('no file ids to compose')
    outfilepath = re.sub(r':[^:]+$', '', outfilepath)
    outdir = os.path.dirname(outfilepath)
    specs = _feature_specs(featurepaths)
    lens = _scan_lengths(specs, fids, 3 if wins else 1)
    dev = _device()
    import torch
    if not os.path.isdir(outdir): os.mkdir(outdir)

    D = sum(w for _, w in specs)
    K = 1 + len(wins)
    W = K * D
    nstat = min(int(id_valid_start), len(fids))
    nbframes = int(sum(lens[:nstat]))
    resident = sum(lens) * W * 4 <= DEVICE_CAP_BYTES
    chunks = _chunks(lens, 4 * W, _budget())
    stage = _Stage()

    # ---- first sweep: windows + min / max / sum -----------------------------------------------------------------------
    stats = ops.compose_stats_buffers(W, dev)
    kept = []
    for i0, i1 in chunks:
        print_tty('\r    Composing files {}-{}/{}               '.format(1 + i0, i1, len(fids)))
        y, offs, offs_d = _load_raw(specs, fids[i0:i1], lens[i0:i1], stage, dev)
        ns = max(0, min(i1, nstat) - i0)
        comp = ops.compose_windows(y, offs_d, wins, stats=stats, n_stat_utts=ns, mlpg_order=(win_convention == 'mlpg'))
        if resident: kept.append((comp, offs, offs_d, i0, i1, ns))
        else:        _write_rows(comp.cpu().numpy(), offs, outfilepath, fids[i0:i1])
    print_tty('\r                                                           \r')
    mins, maxs = stats[0].cpu().numpy(), stats[1].cpu().numpy()
    means = stats[2].cpu().numpy() / nbframes
    zerovaridx = np.where((maxs - mins) == 0.0)[0]
    mins.astype('float32').tofile(os.path.join(outdir, 'min.dat'))
    maxs.astype('float32').tofile(os.path.join(outdir, 'max.dat'))
    means.astype('float32').tofile(os.path.join(outdir, 'mean.dat'))
    if verbose > 1:                                         # pragma: no cover
        print('    mins={}\n    maxs={}\n    means={}'.format(mins, maxs, means))

    # ---- second sweep: centred sum of squares ------------------------------------------------------------------------
    mean_d = torch.from_numpy(means).to(dev)
    sq = torch.zeros(W, dtype=torch.float64, device=dev)
    if resident:
        for comp, offs, offs_d, i0, i1, ns in kept:
            ops.compose_sqdev(comp, offs_d, mean_d, sq, ns)
    else:
        for i0, i1 in chunks:
            if i0 >= nstat: break
            rows, _, offs_d = _load_files(outfilepath, fids[i0:min(i1, nstat)], W, stage, dev)
            ops.compose_sqdev(rows, offs_d, mean_d, sq, min(i1, nstat) - i0)
    with np.errstate(divide='ignore', invalid='ignore'):
        sqdev = sq.cpu().numpy()
        stds = np.sqrt(sqdev / (nbframes - 1))              # unbiased variance estimator
    stds.astype('float32').tofile(os.path.join(outdir, 'std.dat'))
    if verbose > 1: print('    stds={}'.format(stds))       # pragma: no cover

    keepidx = np.arange(W)
    size = W
    if dropzerovardims:
        keepidx = np.setdiff1d(np.arange(W), zerovaridx)
        size = len(keepidx)
        keepidx.astype('int32').tofile(os.path.join(outdir, 'keepidx.dat'))
        print('Dropped dimensions with zero variance. Remains {} dims'.format(size))

    print('{} files'.format(len(fids)))
    print('{} frames ({}s assuming {}s time shift)'.format(nbframes, datetime.timedelta(seconds=nbframes * shift), shift))
    strsize = '+'.join(str(w) for _, w in specs)
    if dropzerovardims: strsize += '-' + str(len(zerovaridx))
    print('nb dimensions={} (features: ({})x{})'.format(size, strsize, K))
    print('{} dimensions with zero-variance ({}){}'.format(len(zerovaridx), zerovaridx,
                                                           ', which have been dropped' if dropzerovardims else ', which have been kept'))
    print('normalisation done using: {}'.format(getattr(normfn, '__name__', repr(normfn))) if normfn is not None else 'no normalisation called')
    print('output path: {} ({} route)'.format(outfilepath, 'device-resident' if resident else 'streamed'))

    # ---- third sweep: normalisation ------------------------------------------------------------------------------------
    own = normfn in (normalise_minmax, normalise_meanstd, normalise_meanstd_nmnoscale)
    if resident and own:
        f32 = lambda a: a.astype('float32')
        if normfn is normalise_minmax:
            plan = _plan_minmax(f32(mins), f32(maxs), outdir, None, keepidx, True)
        elif normfn is normalise_meanstd:
            plan = _plan_meanstd(f32(means), f32(stds), outdir)
        else:
            plan = _plan_meanstd(f32(means), f32(stds), outdir, _noise_slices(featurepaths, W))
        a, b, kidx = _plan_device(plan, dev)
        for comp, offs, offs_d, i0, i1, ns in kept:
            out = ops.compose_normalise(comp, a, b, mode=plan['mode'], scale=plan['scale'], offset=plan['offset'], keepidx=kidx,
                                        out=comp if kidx is None else None)
            _write_rows(out.cpu().numpy(), offs, outfilepath, fids[i0:i1])
    else:
        if resident:
            for comp, offs, offs_d, i0, i1, ns in kept:
                _write_rows(comp.cpu().numpy(), offs, outfilepath, fids[i0:i1])
        if normfn is not None:
            normfn(outfilepath, fids, featurepaths=featurepaths, keepidx=keepidx, verbose=verbose)
    del kept

    result = dict(min=mins, max=maxs, mean=means, std=stds, sqdev=sqdev, nbframes=nbframes, keepidx=keepidx, size=size, resident=resident)
    if do_finalcheck:
        print('Check data final statistics')
        # the width of what was written: the mean/std normalisers do not honour keepidx (the reference reshapes by `size`
        # regardless and cannot check such files)
        wcheck = W if normfn in (None, normalise_meanstd, normalise_meanstd_nmnoscale) else size
        cfids = fids[:nstat]
        clens = [_file_rows(outfilepath.replace('*', fid), wcheck) for fid in cfids]
        def chunks_of():
            for i0, i1 in _chunks(clens, 4 * wcheck, _budget()):
                rows, _, offs_d = _load_files(outfilepath, cfids[i0:i1], wcheck, stage, dev)
                yield rows, offs_d, i1 - i0
        vmin, vmax, vmeans, vsq = _device_stats(chunks_of, sum(clens), wcheck, dev)
        with np.errstate(divide='ignore', invalid='ignore'):
            check = dict(verif_min=vmin, verif_max=vmax, verif_means=vmeans, verif_stds=vsq / (sum(clens) - 1))
        if verbose > 0:                                     # pragma: no cover
            for k in ('verif_min', 'verif_max', 'verif_means', 'verif_stds'): print('{}={}'.format(k, check[k]))
        result['finalcheck'] = check
    return result


# ---------------------------------------------------------------------------------------------------------------------------
# time weights (compose.py:365-455): one scalar per frame, host numpy
# ---------------------------------------------------------------------------------------------------------------------------
def create_weights_spec(specfeaturepath, fids, outfilepath, thresh=-32, dftlen=4096, spec_type='fwlspec'):
    """One weight per frame from the spectral energy: 1 where the frame's energy, relative to the loudest frame of the file, is
    at least `thresh` dB, 0 below (training drops the silent frames at both ends).  spec_type 'fwlspec': energy from the mean of
    the log spectrum; 'mcep' / 'fwcep': from the first cepstral coefficient."""
    if spec_type not in ('fwlspec', 'mcep', 'fwcep'):
        raise ValueError('unknown spec_type {!r}'.format(spec_type))
    outfilepath = re.sub(r':[^:]+$', '', outfilepath)
    if not os.path.isdir(os.path.dirname(outfilepath)): os.mkdir(os.path.dirname(outfilepath))
    infilepath, shape = data.getpathandshape(specfeaturepath)
    if shape is None: shape = (-1, 1)
    for nf, fid in enumerate(fids):
        print_tty('\r    Processing feature files {} for {}                '.format(nf, fid))
        Y = np.fromfile(infilepath.replace('*', fid), dtype='float32').reshape(shape)
        logamp = np.mean(Y, axis=1) if spec_type == 'fwlspec' else Y[:, 0]
        ener = 20.0 * np.log10(np.abs(np.exp(logamp)))
        ener -= np.max(ener)
        weight = ener.copy()
        weight[ener >= thresh] = 1.0
        weight[ener < thresh] = 0.0
        weight.astype('float32').tofile(outfilepath.replace('*', fid))
    print_tty('\r                                                           \r')


def create_weights_lab(labpath, fids, outfilepath, lineheadregexp=r'([^\^]+)\^([^-]+)-([^\+]+)\+([^=]+)=([^@]+)@(.+)',
                       silencesymbol='sil', shift=0.005):
    """One weight per frame from an HTS label file: 0 over the segments whose centre phone is `silencesymbol`, 1 elsewhere.
    `fids` is the path of the file-id list (or the list of ids itself).  Some label formats use r'([^\\~]+)\\~([^-]+)-([^\\+]+)\\+([^=]+)=([^:]+):(.+)'."""
    makedirs(os.path.dirname(outfilepath))
    outfilepath, _ = data.getpathandshape(outfilepath)
    segment = re.compile(r'([0-9]+)\s+([0-9]+)\s+(.+)')
    for fid in (readids(fids) if isinstance(fids, str) else fids):
        print_tty('\r    Processing feature file {}                '.format(fid))
        with open(labpath.replace('*', fid)) as f:
            lines = f.readlines()
        tend = float(segment.findall(lines[-1])[0][1]) * 1e-7
        weight = np.ones(int(np.ceil(tend / shift)), dtype='float32')
        for line in lines:
            start, end, head = segment.findall(line)[0]
            tstart, tend = float(start) * 1e-7, float(end) * 1e-7
            if re.findall(lineheadregexp, head)[0][2] == silencesymbol:
                weight[int(np.floor(tstart / shift)):int(np.ceil(tend / shift))] = 0.0
        weight.astype('float32').tofile(outfilepath.replace('*', fid))
    print_tty('\r                                                           \r')
