"""Host-side batch loading and cost helpers (numpy only) -- the callers' side of the hot path.

Same function names, arguments and results as the reference's percivaltts/data.py:34-406 for what the
training driver uses: `path:(shape)` selectors (:34-76), load (:96-133), croplen (:143-171),
croplen_weight (:173-231), batching with random-shift windows (:234-284), load_inoutset (:297-322) and
the cost helpers (:327-406).  Files are headerless float32.
"""
from __future__ import print_function

import copy
import os
import re
import time

import numpy as np

from .percivaltts import is_int, print_tty

_SEL = re.compile(r'(.*):\((.*)\)')


def getpath(path):
    m = _SEL.findall(path)
    return m[0][0] if m else path


def getpathandshape(path, shape=None):
    """'/dir/*.spec:(-1,60)' -> ('/dir/*.spec', (-1, 60)); a non-integer selector names a file whose length is used."""
    m = _SEL.findall(path)
    if not m:
        return path, shape
    path = m[0][0]
    sel = ()
    for s in m[0][1].split(','):
        if is_int(s):
            sel += (int(s),)
        else:
            sel += (np.fromfile(os.path.join(os.path.dirname(path), s), dtype=np.float32).shape[0],)
    if shape is not None:
        print('WARNING: shape has been set both as argument ({}) of the getpathandshape(.) function and in the file '
              'selector ({}) (at the end of path); The one set as argument will be used: {}'.format(shape, sel, shape))
        return path, shape
    return path, sel


def getlastdim(path):
    _, size = getpathandshape(path)
    return 1 if size is None else size[-1]


def _read(fpath, shape):
    if not os.path.isfile(fpath):
        raise ValueError('{} does not exists'.format(fpath))
    X = np.fromfile(fpath, dtype='float32')
    if shape is not None:
        X = X.reshape(shape)
    if np.isnan(X).any(): raise ValueError('ERROR: There are nan in {}'.format(fpath))
    if np.isinf(X).any(): raise ValueError('ERROR: There are inf in {}'.format(fpath))
    return X


def loadfile(fpath, fbase=None, shape=None):
    if fbase is not None:
        fpath = fpath.replace('*', fbase)
    fpath, shape = getpathandshape(fpath, shape)
    return _read(fpath, shape)


def load(dirpath, fbases, shape=None, frameshift=0.005, verbose=0, label=''):
    """List of matrices, one per file id."""
    dirpath, shape = getpathandshape(dirpath, shape)
    Xs, totlen, memsize = [], 0, 0.0
    for n, fbase in enumerate(fbases):
        if verbose > 0:
            print_tty('\r    {}Loading file {}/{} {}: ({:.2f}% done)        '.format(label, 1 + n, len(fbases), fbase, 100.0 * n / len(fbases)))
        X = _read(dirpath.replace('*', fbase), shape)
        Xs.append(X)
        totlen += X.shape[0]
        memsize += X.size * 4 / float(1024 ** 2)
    if verbose > 0:
        print_tty('\r                                                                 \r')
        print('    {}{} sentences, frames={} ({}), {} MB                     '.format(
            label, len(fbases), totlen, time.strftime('%H:%M:%S', time.gmtime(totlen * frameshift)), memsize))
    return Xs


def gettotallen(Xs, axis=0):
    return sum(x.shape[axis] for x in Xs)


def croplen(xs, axis=0):
    """Crop, sample by sample, every list of `xs` to the shortest length found among the lists (in place)."""
    if axis > 2:
        raise ValueError('Do not manage axis values bigger than 2')
    if len(set(len(x) for x in xs)) > 1:
        raise ValueError('the size of the data sets are not identical ({})'.format([len(x) for x in xs]))
    for ki in range(len(xs[0])):
        siz = min(x[ki].shape[axis] for x in xs)
        idx = [slice(None)] * axis + [slice(0, siz)]
        for x in xs:
            x[ki] = x[ki][tuple(idx)]
    return xs


def croplen_weight(xs, w, thresh=0.5, cropmode='begend', cropsize=int(0.750 / 0.005)):
    """Drop frames whose weight is below `thresh`: at both ends ('begend'), also inside when the silent gap is longer
    than `cropsize` frames ('begendbigger'), or everywhere ('all')."""
    if len(set([len(w)] + [len(x) for x in xs])) > 1:
        raise ValueError('the size of the data sets are not identical ({})'.format([len(x) for x in xs]))
    for ki in range(len(w)):
        wk = w[ki][:, 0] if w[ki].ndim > 1 else w[ki]
        keep = wk > thresh
        if cropmode == 'begend':
            on = np.where(keep)[0]
            sel = slice(int(on.min()), int(on.max()))
        elif cropmode == 'begendbigger':
            on = np.where(keep)[0]
            gaps = np.diff(on)
            for gi in np.where(gaps > 1)[0]:
                if gaps[gi] < int(cropsize):
                    keep[on[gi]:on[gi + 1]] = True
            sel = np.where(keep)[0]
        elif cropmode == 'all':
            sel = np.where(keep)[0]
        else:
            raise ValueError('unknown cropmode ' + str(cropmode))
        for x in xs:
            x[ki] = x[ki][sel,]
        w[ki] = w[ki][sel,]
    return xs, w


def batching(xs, length=None, lengthmax=None, padtype='randshift', outmask=False, rand=None):
    """Stack 2-D matrices into [B, length, feat] batches.  'randshift' takes a random window of `length` frames from
    every sample (np.random.randint, so the numpy seed makes it repeatable); 'padright' zero-pads on the right.
    'randshiftpad' does both (masked training): `length` is the given one or the LONGEST sample's, capped by lengthmax; a
    sample longer than that gives a random window, a shorter one all its frames, zero-padded on the right.  It takes one
    np.random.randint(0, max(len - length, 0) + 1) draw per row, in row order, whatever the row's length, so the numbers a
    batch consumes depend on its size alone.
    `rand` (optional, one uniform number in [0, 1) per sample): the shift of sample b is floor(rand[b] * (number of possible
    shifts)) instead of a fresh np.random.randint draw -- what data parallelism uses, so that a rank that loads only its
    shard of the files takes the same windows as the process that loads the whole batch (load_inoutset)."""
    if len(set(len(x) for x in xs)) > 1:
        raise ValueError('the size of the data sets are not identical ({})'.format([len(x) for x in xs]))
    nb = len(xs[0])
    if length is None:
        lens = [xs[0][b].shape[0] for b in range(nb)]
        length = max(lens) if padtype in ('padright', 'randshiftpad') else min(lens)
    if lengthmax is not None and length > lengthmax:
        length = lengthmax
    xbs = []
    for x in xs:
        feat = 1 if x[0].ndim == 1 else x[0].shape[1]
        xbs.append(np.zeros((len(x), length, feat), dtype='float32'))
    MB = np.zeros((nb, length), dtype='float32') if outmask else None
    shift = 0
    for b in range(nb):
        samplelen = xs[0][b].shape[0]
        minlen = min(samplelen, length)
        if padtype == 'randshift':
            if rand is not None:
                shift = min(int(rand[b] * ((samplelen - length) + 1)), samplelen - length)
            else:
                shift = np.random.randint(0, (samplelen - length) + 1)
        elif padtype == 'randshiftpad':
            nshift = max(samplelen - length, 0) + 1
            shift = min(int(rand[b] * nshift), nshift - 1) if rand is not None else np.random.randint(0, nshift)
        for xi, x in enumerate(xs):
            seg = x[b][shift:shift + minlen]
            xbs[xi][b, :minlen, :] = seg.reshape(minlen, -1)
        if outmask: MB[b, :minlen] = 1
    return xbs, MB


def addstop(X, value=1.0):
    X = copy.deepcopy(X)
    stop = np.zeros(X[0].shape[1] + 1)
    stop[-1] = value
    for xi in range(len(X)):
        X[xi] = np.vstack((np.concatenate((X[xi], np.zeros((X[xi].shape[0], 1))), axis=1), stop))
    return X


def _kept_len(wk, thresh, cropmode, cropsize):
    """Number of frames croplen_weight keeps of a weight track (same selection rules, no data moved)."""
    keep = wk > thresh
    if cropmode == 'begend':
        on = np.where(keep)[0]
        return int(on.max()) - int(on.min())
    if cropmode == 'begendbigger':
        on = np.where(keep)[0]
        gaps = np.diff(on)
        for gi in np.where(gaps > 1)[0]:
            if gaps[gi] < int(cropsize):
                keep[on[gi]:on[gi + 1]] = True
        return int(keep.sum())
    if cropmode == 'all':
        return int(keep.sum())
    raise ValueError('unknown cropmode ' + str(cropmode))


def batch_window_length(indir, outdir, outwdir, fid_lst, length=None, lengthmax=None, maskpadtype='padright', cropmode='begend',
                        thresh=0.5, cropsize=int(0.750 / 0.005)):
    """The window length T load_inoutset would choose for the batch `fid_lst` (reference data.py:297-322 -> croplen,
    croplen_weight, batching: with length=None it is the min ('randshift') or max ('padright', 'randshiftpad') of the cropped sample lengths,
    clipped by lengthmax), found WITHOUT reading the wide files: the frame counts of the inputs and outputs come from the file
    sizes, only the one-column time-weight files are read.  Data parallelism needs it before sharding: a rank that loads only its
    shard must window it to the GLOBAL batch's T -- the shard's own min / max can differ, and with it every random shift."""
    if length is not None:
        return int(min(length, lengthmax)) if lengthmax is not None else int(length)
    lens = []
    ipath, ishape = getpathandshape(indir)
    opath, oshape = getpathandshape(outdir)
    wpath, wshape = getpathandshape(outwdir)
    def frames(path, shape, fid):
        f = path.replace('*', fid)
        if not os.path.isfile(f):
            raise ValueError('{} does not exists'.format(f))
        dim = 1
        if shape is not None:
            for d in shape[1:]: dim *= int(d)
        return os.path.getsize(f) // (4 * dim)
    for fid in fid_lst:
        w = _read(wpath.replace('*', fid), wshape)
        n = min(frames(ipath, ishape, fid), frames(opath, oshape, fid), w.shape[0])
        wk = (w[:, 0] if w.ndim > 1 else w)[:n]
        lens.append(_kept_len(wk, thresh, cropmode, cropsize))
    T = max(lens) if maskpadtype in ('padright', 'randshiftpad') else min(lens)
    if lengthmax is not None and T > lengthmax:
        T = lengthmax
    return int(T)


def load_inoutset(indir, outdir, outwdir, fid_lst, inouttimesync=True, length=None, lengthmax=None,
                  maskpadtype='padright', cropmode='begend', verbose=0, rand=None, outlengths=False):
    """Load one batch of inputs, outputs and time weights, cropped and windowed: X [B,T,ctx], Y [B,T,out], W [B,T,1]
    (reference data.py:297-322).  `rand`: see batching -- the per-sample uniforms of the random window shifts, drawn by the
    caller for the WHOLE global batch so that every rank can load its shard of `fid_lst` alone.  outlengths: also return
    n [B] int32, the real frames of every row (min of the cropped length and T; the frames behind them are zero padding),
    as a fourth value; time-synchronous sets only."""
    if outlengths and not inouttimesync:
        raise ValueError('outlengths needs inouttimesync=True')
    X = load(indir, fid_lst, verbose=verbose, label='Context labels: ')
    Y = load(outdir, fid_lst, verbose=verbose, label='Output features: ')
    W = load(outwdir, fid_lst, verbose=verbose, label='Time weights: ')
    if inouttimesync:
        X, Y, W = croplen([X, Y, W])
        [X, Y], W = croplen_weight([X, Y], W, cropmode=cropmode)
        lens = [x.shape[0] for x in X]
        [X, Y, W], _ = batching([X, Y, W], length=length, lengthmax=lengthmax, padtype=maskpadtype, rand=rand)
        if outlengths:
            return X, Y, W, np.minimum(lens, X.shape[1]).astype(np.int32)
    else:
        X = addstop(X)
        Y, W = croplen([Y, W])
        [Y], W = croplen_weight([Y], W, cropmode=cropmode)
        Y = addstop(Y)
        [X], _ = batching([X], length=length, lengthmax=lengthmax, padtype=maskpadtype)
        [Y], _ = batching([Y], length=length, lengthmax=lengthmax, padtype=maskpadtype)
    return X, Y, W


class DeviceCorpusTooLarge(ValueError):
    """The packed training set needs more device memory than DeviceCorpus was allowed (`needed` and `maxbytes`, in bytes)."""

    def __init__(self, needed, maxbytes):
        ValueError.__init__(self, 'the packed corpus needs {} bytes of device memory, {} are allowed'.format(needed, maxbytes))
        self.needed, self.maxbytes = int(needed), int(maxbytes)


class DeviceCorpus(object):
    """A training set read, cropped and uploaded ONCE: what load_inoutset(inouttimesync=True) does for every batch, up to the
    windowing.  The three files of every id are loaded, croplen cuts them to their common length and croplen_weight drops the
    silences (`cropmode`) -- the functions above, one utterance at a time -- and the cropped utterances are packed row-wise into
    X [N,ctx], Y [N,out], W [N,1] on `device` (upload), utterance u in the rows row_off[u] .. row_off[u+1]-1.  A batch is then
    a window plan made on the host (plan: the very shifts batching would draw, from the same numpy generator) and ONE gather
    launch (ops.batch_windows); no file is read and no frame crosses the host interface again.

    lens: the kept lengths, raw_out_frames: the frames of each output file as read; both stay on the host.  `ids` of the
    methods are file ids of fid_lst or indices into it.  maxbytes: the device memory the packed set may take, None for half of
    what is free on `device` now; a larger set raises DeviceCorpusTooLarge before anything is uploaded.  device None: the current
    HIP device, the host without one (plan, window_length and the packed rows work there; batch needs the device)."""

    def __init__(self, indir, outdir, outwdir, fid_lst, cropmode='begend', device=None, maxbytes=None):
        Xs, Ys, Ws, raw = [], [], [], []
        for fid in fid_lst:
            X, Y, W = load(indir, [fid]), load(outdir, [fid]), load(outwdir, [fid])
            raw.append(int(Y[0].shape[0]))
            X, Y, W = croplen([X, Y, W])
            [X, Y], W = croplen_weight([X, Y], W, cropmode=cropmode)
            Xs.append(X[0]); Ys.append(Y[0]); Ws.append(W[0])
        self.cropmode, self.raw_out_frames = cropmode, raw
        self._pack(Xs, Ys, Ws, fid_lst, device, maxbytes)

    @classmethod
    def from_utterances(cls, Xs, Ys, Ws, fid_lst=None, device=None, maxbytes=None):
        """The corpus of utterances that are cropped already: three lists of [T_u, D] arrays, of equal T_u across the lists."""
        self = cls.__new__(cls)
        self.cropmode, self.raw_out_frames = None, [int(y.shape[0]) for y in Ys]
        self._pack(list(Xs), list(Ys), list(Ws), fid_lst if fid_lst is not None else [str(u) for u in range(len(Xs))], device, maxbytes)
        return self

    def _pack(self, Xs, Ys, Ws, fid_lst, device, maxbytes):
        import torch
        if device is None:
            device = torch.device('cuda', torch.cuda.current_device()) if torch.cuda.is_available() else 'cpu'
        self.device = torch.device(device)
        self.fid_lst = list(fid_lst)
        self._index = dict((fid, u) for u, fid in enumerate(self.fid_lst))
        if not (len(Xs) == len(Ys) == len(Ws) == len(self.fid_lst) >= 1) or any(not (x.shape[0] == y.shape[0] == w.shape[0]) for x, y, w in zip(Xs, Ys, Ws)):
            raise ValueError('the size of the data sets are not identical')
        self.lens = np.array([x.shape[0] for x in Xs], dtype=np.int64)
        self.row_off = np.concatenate(([0], np.cumsum(self.lens))).astype(np.int64)
        pack = lambda xs: np.ascontiguousarray(np.concatenate([x.reshape(x.shape[0], -1) for x in xs], axis=0), dtype=np.float32)
        self.nbytes = 4 * int(self.row_off[-1]) * sum(int(np.prod(xs[0].shape[1:])) for xs in (Xs, Ys, Ws))
        if maxbytes is None and self.device.type == 'cuda':
            maxbytes = torch.cuda.mem_get_info(self.device)[0] // 2
        if maxbytes is not None and self.nbytes > maxbytes:
            raise DeviceCorpusTooLarge(self.nbytes, maxbytes)
        self.maxbytes = maxbytes
        streams = []
        for xs in (Xs, Ys, Ws):            # one stream at a time: the host holds one packed copy beside the utterances
            streams.append(upload(torch.from_numpy(pack(xs)), self.device))
            del xs[:]
        self.X, self.Y, self.W = streams
        self._row_off_host = torch.from_numpy(self.row_off)
        self._row_off_dev = upload(self._row_off_host, self.device)

    def __len__(self):
        return len(self.fid_lst)

    def _utts(self, ids):
        return np.array([self._index[i] if isinstance(i, str) else int(i) for i in ids], dtype=np.int64)

    def window_length(self, ids, length=None, lengthmax=None, padtype='randshift'):
        """The T of the batch `ids`: what batch_window_length finds for them, from the kept lengths (no file is touched)."""
        if length is None:
            lens = self.lens[self._utts(ids)]
            length = lens.max() if padtype in ('padright', 'randshiftpad') else lens.min()
        if lengthmax is not None and length > lengthmax:
            length = lengthmax
        return int(length)

    def plan(self, ids, length=None, lengthmax=None, padtype='randshift', rand=None):
        """(T, utt, shift, n) of the batch `ids` (int32 arrays [B]), exactly as batching chooses them: 'randshift' draws one
        np.random.randint(0, len - T + 1) per row, in row order -- the global numpy generator is left as load_inoutset leaves it
        -- or takes floor(rand[b] * number of shifts); 'padright' draws nothing; 'randshiftpad' draws one
        np.random.randint(0, max(len - T, 0) + 1) per row, a row shorter than T included.  n[b] = min(len, T) real frames.  Host only."""
        utt = self._utts(ids)
        T = self.window_length(utt, length, lengthmax, padtype)
        shift = np.zeros(len(utt), dtype=np.int32)
        n = np.minimum(self.lens[utt], T).astype(np.int32)
        if padtype == 'randshift':
            for b, samplelen in enumerate(self.lens[utt]):
                samplelen = int(samplelen)
                if rand is None:
                    shift[b] = np.random.randint(0, (samplelen - T) + 1)       # (raises for an utterance shorter than `length`, as in batching)
                elif samplelen < T:
                    raise ValueError('utterance {} has {} frames, fewer than the window of {}'.format(self.fid_lst[utt[b]], samplelen, T))
                else:
                    shift[b] = min(int(rand[b] * ((samplelen - T) + 1)), samplelen - T)
        elif padtype == 'randshiftpad':
            for b, samplelen in enumerate(self.lens[utt]):
                nshift = max(int(samplelen) - T, 0) + 1
                shift[b] = min(int(rand[b] * nshift), nshift - 1) if rand is not None else np.random.randint(0, nshift)
        return T, utt.astype(np.int32), shift, n

    def batch(self, ids, length=None, lengthmax=None, padtype='randshift', rand=None, rows=None, want_w=False, want_lengths=False):
        """The batch load_inoutset(..., fid_lst=ids, length, lengthmax, maskpadtype=padtype, rand) gives, as device tensors
        X [B,T,ctx], Y [B,T,out] (and W [B,T,1] with want_w): the plan, its three small tables uploaded asynchronously, one
        gather launch on the current stream.  rows=(lo, hi): only these rows of the planned batch (a rank's shard; the plan, and
        with it every random draw, is the whole batch's).  want_lengths: n [B] (int32, on the host: the plan's real frames per
        row) as the last value."""
        import torch
        from . import ops
        T, utt, shift, n = self.plan(ids, length, lengthmax, padtype, rand)
        if rows is not None:
            utt, shift, n = (a[rows[0]:rows[1]] for a in (utt, shift, n))
        srcs = [self.X, self.Y] + ([self.W] if want_w else [])
        out = tuple(ops.batch_windows(srcs, self._row_off_host, torch.from_numpy(np.ascontiguousarray(utt)), torch.from_numpy(np.ascontiguousarray(shift)),
                                      torch.from_numpy(np.ascontiguousarray(n)), T, row_off_dev=self._row_off_dev))
        return out + (np.ascontiguousarray(n),) if want_lengths else out


# ---- evaluation helpers ----------------------------------------------------------------------------------
def cost_0pred_rmse(Y_val):
    """RMSE of the all-zero prediction (the worst predictor)."""
    if isinstance(Y_val, list):
        return float(np.sqrt(sum(np.sum(y ** 2) for y in Y_val) / float(sum(y.size for y in Y_val))))
    return float(np.sqrt(np.mean(Y_val ** 2)))


def _one_by_one(Xs):
    for xi in range(len(Xs[0])):
        yield xi, [np.reshape(inp[xi], [1] + list(inp[xi].shape)) for inp in Xs]


def cost_model_mfn(fn, Xs):
    """Average of fn over the samples, one utterance at a time."""
    if not isinstance(Xs[0], list):
        return 0.0
    cost = 0.0
    for _, ins in _one_by_one(Xs):
        cost += fn(*ins)
    return cost / len(Xs[0])


def upload(t, dev):
    """A host tensor on the device `dev` without making the host wait for the device: staged in pinned memory, copied
    asynchronously on the current stream (the pinned block is recycled only once that copy has run)."""
    import torch
    if t.is_cuda or torch.device(dev).type != 'cuda':
        return t.to(dev)
    return t.contiguous().pin_memory().to(dev, non_blocking=True)


def pad_to_device(xs, dev, what='pad_to_device'):
    """A list of [T_i >= 1, D] arrays or tensors -> (zero-padded float32 device tensor [B, max T_i, D], the lengths as an int32 device
    tensor [B], the lengths as a list): the form ragged inference takes (memo['lengths']).  Host utterances are padded on the host
    and go up in one asynchronous copy (`upload`)."""
    import torch
    ts = [torch.as_tensor(x if torch.is_tensor(x) else np.ascontiguousarray(x), dtype=torch.float32) for x in xs]
    for t in ts:
        if t.dim() != 2 or t.shape[0] < 1 or t.shape[1] != ts[0].shape[1]:
            raise ValueError('{}: every utterance has to be [T >= 1, ctx], got {}'.format(what, tuple(t.shape)))
    lens = [int(t.shape[0]) for t in ts]
    on_host = not any(t.is_cuda for t in ts)
    xpad = torch.zeros((len(ts), max(lens), ts[0].shape[1]), dtype=torch.float32, device='cpu' if on_host else dev)
    for i, t in enumerate(ts):
        xpad[i, :lens[i]] = t if on_host else t.to(dev)
    return upload(xpad, dev), upload(torch.tensor(lens, dtype=torch.int32), dev), lens


def _padding(lens, groups):
    return sum(len(g) * max(lens[i] for i in g) - sum(lens[i] for i in g) for g in groups)


def length_groups(lens, batch_size, sort=True):
    """Index groups of at most `batch_size` utterances for ragged batches: every index of range(len(lens)) once.  Without `sort`
    the groups are consecutive runs of the input order.  With it they are runs of the stable sort by length, so that utterances of
    similar length share a group and the frames spent on padding (group size x longest - frames, summed) are as few as groups of
    these sizes allow; the one short group (when batch_size does not divide the count) stands where that sum is least, the first
    such place.  The caller scatters its results back to input order."""
    n, k = len(lens), int(batch_size)
    if k < 1:
        raise ValueError('batch_size has to be at least 1')
    chunk = lambda order, sizes: [[order.pop(0) for _ in range(s)] for s in sizes]
    sizes = [k] * (n // k) + ([n % k] if n % k else [])
    if not sort:
        return chunk(list(range(n)), sizes)
    order = [int(i) for i in np.argsort(np.asarray(lens, dtype=np.int64), kind='stable')]
    if n % k == 0 or n < k:
        return chunk(order, sizes)
    best = None
    for pos in range(len(sizes)):
        s = [k] * pos + [n % k] + [k] * (len(sizes) - 1 - pos)
        groups = chunk(list(order), s)
        pad = _padding(lens, groups)
        if best is None or pad < best[0]:
            best = (pad, groups)
    return best[1]


def cost_model_prediction_rmse(mod, Xs, Y_val, inouttimesync=True, batch_size=None, sort=True):
    """sqrt(sum of squared errors / number of values) over the whole set.  `batch_size`: the utterances are predicted in ragged
    batches (data.length_groups(lengths, batch_size, sort): of similar length; mod.predict_device_padded) and the squared errors are summed on the device (ptts_wlse_rows), one
    download at the end; None: one utterance at a time through mod.predict, as the reference does."""
    if not isinstance(Xs[0], list):
        return 0.0
    if batch_size is not None:
        import torch
        from . import ops
        sq, nbel = [], 0
        for g in length_groups([x.shape[0] for x in Xs[0]], batch_size, sort=sort):
            ypred, lengths, lens = mod.predict_device_padded([Xs[0][i] for i in g])
            ypad, _, ylens = pad_to_device([Y_val[i] for i in g], ypred.device, 'cost_model_prediction_rmse')
            if ylens != lens or ypad.shape != ypred.shape:
                raise ValueError('cost_model_prediction_rmse: inputs and targets differ in shape')
            sq.append(ops.wlse_rows(ypad, ypred, None, lengths, want_ls=False)[1])
            nbel += sum(lens) * int(ypred.shape[-1])
        return float(np.sqrt(float(torch.cat(sq).sum().item()) / nbel))
    cost, nbel = 0.0, 0
    for xi, ins in _one_by_one(Xs):
        ypred = mod.predict(*ins)
        cost += np.sum((Y_val[xi] - ypred[0,]) ** 2)
        nbel += ypred[0,].size
    return float(np.sqrt(cost / nbel))


def prediction_mstd(mod, Xs):
    if not isinstance(Xs[0], list):
        return 0.0
    s = 0.0
    for _, ins in _one_by_one(Xs):
        s += np.std(mod.predict(*ins)[0,])
    return s / len(Xs[0])


def prediction_rms(mod, Xs):
    if not isinstance(Xs[0], list):
        return 0.0
    s, nbel = 0.0, 0
    for _, ins in _one_by_one(Xs):
        ypred = mod.predict(*ins)
        s += np.sum(ypred[0,] ** 2)
        nbel += ypred[0,].size
    return float(np.sqrt(s / nbel))


class BatchPrefetcher(object):
    """Double-buffered batch pipeline in front of `train_on_batch`.

    The reference loads the files of a batch, builds the numpy arrays and only then trains on them, every batch
    (optimizertts.py:230-232), so a sub-15 ms device step would wait on numpy I/O and on a synchronous host-to-device
    copy.  Here a worker thread calls `make_batch(i)` (any function returning a tuple of float32 numpy arrays, e.g.
    `load_inoutset` of the i-th list of file ids) for i = 0..n-1 and issues the host-to-device copies on a dedicated
    HIP copy stream; the consumer iterates over device tensors and its stream waits on the copy's event, not on the
    host.  `depth` batches are in flight (2 = double buffering).  stage_pinned=True first copies each array into a
    reusable pinned buffer (a slot is rewritten only after its DMA completed) -- useful when the loader can fill such
    a buffer directly; for numpy arrays that already exist it measured slower than letting the runtime stage them.

    host_items: positions of the batch tuple handed through unconverted, on the host (default: none).

    device=None (or a CPU device) gives the same iterator without pinning or streams (host tests).
    """

    _END = object()

    def __init__(self, make_batch, n, device=None, depth=2, stage_pinned=False, host_items=()):
        import threading
        try:
            import queue
        except ImportError:      # pragma: no cover
            import Queue as queue
        import torch
        self._torch = torch
        self._make, self._n, self._depth = make_batch, int(n), max(1, int(depth))
        self._device = torch.device(device) if device is not None else torch.device('cpu')
        self._cuda = self._device.type == 'cuda'
        if self._cuda and self._device.index is None:
            self._device = torch.device('cuda', torch.cuda.current_device())
        self._stage = bool(stage_pinned)
        self._host_items = frozenset(int(k) for k in host_items)
        self._q = queue.Queue(maxsize=self._depth)
        self._slots = [None] * (self._depth + 1)      # pinned buffers (+1: one is being filled while `depth` are queued)
        self._events = [None] * (self._depth + 1)
        self._copy_stream = torch.cuda.Stream(device=self._device) if self._cuda else None
        self._stop = False
        self.load_seconds = 0.0
        self._thread = threading.Thread(target=self._work, name='ptts-prefetch')
        self._thread.daemon = True
        self._thread.start()

    def _pinned(self, slot, k, shape):
        torch = self._torch
        bufs = self._slots[slot]
        if bufs is None:
            bufs = self._slots[slot] = {}
        need = int(np.prod(shape))
        b = bufs.get(k)
        if b is None or b.numel() < need:
            b = bufs[k] = torch.empty(need, dtype=torch.float32).pin_memory()
        return b[:need].view(*shape)

    def _work(self):
        torch = self._torch
        try:
            if self._cuda:
                torch.cuda.set_device(self._device)
            for i in range(self._n):
                if self._stop:
                    break
                t0 = time.time()
                arrays = self._make(i)
                self.load_seconds += time.time() - t0
                if not isinstance(arrays, (tuple, list)):
                    arrays = (arrays,)
                # host_items: the positions of a batch that stay on the host as they are (the lengths of a 'randshiftpad' batch: the
                # step uploads them and takes the number of real frames from them without asking the device)
                ints = [k in self._host_items for k in range(len(arrays))]
                if not self._cuda:
                    item = tuple(a if i else torch.as_tensor(np.ascontiguousarray(a, dtype=np.float32)) for a, i in zip(arrays, ints))
                    self._q.put((item, None))
                    continue
                slot = i % len(self._slots)
                outs = []
                with torch.cuda.stream(self._copy_stream):
                    for k, a in enumerate(arrays):
                        if ints[k]:
                            outs.append(a)
                            continue
                        a = np.ascontiguousarray(a, dtype=np.float32)
                        d = torch.empty(a.shape, dtype=torch.float32, device=self._device)
                        if self._stage:
                            if self._events[slot] is not None:
                                self._events[slot].synchronize()      # the copy that last read this pinned slot is done
                            pin = self._pinned(slot, k, a.shape)
                            np.copyto(pin.numpy(), a)                 # single-threaded memcpy, interpreter lock released
                            d.copy_(pin, non_blocking=True)
                        else:
                            # pageable source: the HIP runtime stages it through its own pinned chunks, pipelined with the
                            # DMA (measured 1.1 ms for 61 MB, against 10 ms for a host-side copy into a pinned buffer plus the
                            # DMA); the call blocks this loader thread only
                            d.copy_(torch.from_numpy(a))
                        outs.append(d)
                    ev = self._copy_stream.record_event()
                self._events[slot] = ev
                self._q.put((tuple(outs), ev))
            self._q.put((self._END, None))
        except BaseException as e:       # hand the failure to the consumer instead of dying silently
            self._q.put((e, None))

    def __iter__(self):
        return self

    def __next__(self):
        item, ev = self._q.get()
        if item is self._END:
            self._q.put((self._END, None))
            raise StopIteration
        if isinstance(item, BaseException):
            raise item
        if ev is not None:
            cur = self._torch.cuda.current_stream(self._device)
            cur.wait_event(ev)
            for t in item:
                if self._torch.is_tensor(t):
                    t.record_stream(cur)       # allocated on the copy stream, consumed here
        return item

    next = __next__

    def close(self):
        self._stop = True
        try:
            while True:
                self._q.get_nowait()
        except Exception:
            pass
        self._thread.join(timeout=10.0)
