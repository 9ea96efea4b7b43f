"""Wrappers of the offline pipeline over the HIP kernels of libpercival_hip.so: parameter generation (MLPG), feature
composition, spectral envelope decompression, pulse-and-noise synthesis (PML) and periodic-plus-aperiodic synthesis (WORLD), each per
utterance with a host pulse table or over a batch with the table built on the device, waveform analysis (PML and WORLD), F0 estimation,
both per utterance or over a packed batch in one launch per kernel, waveform pre-processing and the label front end (questions,
frame expansion, and the segment table from durations).

Argument checks, scratch memory and one C-ABI call (include/percival_hip.h) each; no autograd nodes, no switches, nothing
of the training path (ops.py, which re-exports the names of __all__).  There is no CPU path.
"""
import ctypes
import math

import numpy as np
import torch

from . import _hip
from ._hip import call, ptr, stream, f32c, _workspace

__all__ = [
    'MLPG_WORKSPACE_CAP', 'mlpg_windows', 'mlpg',
    'NORM_MEANSTD', 'NORM_MINMAX', 'COMPOSE_MAX_WINS', 'compose_window_taps', 'compose_stats_buffers', 'compose_windows',
    'compose_sqdev', 'compose_normalise',
    'SPECTRUM_MAX_M1', 'SPECTRUM_MAX_NB', 'SPECTRUM_MAX_DFTLEN', 'spectrum_check', 'bark_alpha', 'mcep_postfilter', 'mcep2spec',
    'fwbnd2spec', 'SPEC2MCEP_MAX_TABLE_BYTES', 'spec2mcep_order_limit', 'spec2mcep_table_bytes', 'spec2mcep_check', 'spec2mcep',
    'PULSE_MIN_DFTLEN', 'PULSE_MAX_DFTLEN', 'PULSE_F0_FLOOR', 'PULSE_INT_ROWS', 'pulse_check', 'pulse_table', 'noise_mask',
    'pulse_synthesis',
    'WORLD_UNVOICED_RATE', 'WORLD_INT_ROWS', 'world_pulse_table', 'aper_rows', 'world_synthesis',
    'PULSE_F0_CAP', 'PULSE_MAX_UTTS', 'pulse_table_cap', 'PulseTableDevice', 'pulse_table_device', 'pulse_synthesis_batch',
    'world_synthesis_batch',
    'COMPRESS_MEAN', 'COMPRESS_LSQ', 'ANALYSIS_NOISY_BELOW', 'analysis_check', 'f0_track', 'frame_harmonics', 'phase_coherence',
    'fwbnd_compress_check', 'fwbnd_compress',
    'world_analysis_check', 'world_envelope', 'world_aperiodicity',
    'F0_MIN_NCAND', 'F0_MAX_NCAND', 'F0_MAX_FRAMES', 'F0_CONSTANTS', 'f0_check', 'f0_frame_count', 'f0_window_table', 'f0_candidates',
    'f0_viterbi', 'f0_estimate', 'F0_REFINE_MAX_WINDOW', 'f0_refine_check', 'f0_refine',
    'ANALYSIS_MAX_UTTS', 'PackedOffsets', 'packed_offsets', 'analysis_status', 'wave_peak', 'f0_track_lengths', 'f0_track_device',
    'f0_candidates_batch', 'f0_viterbi_batch', 'f0_estimate_batch', 'f0_refine_batch', 'frame_harmonics_batch',
    'phase_coherence_batch', 'world_envelope_batch', 'world_aperiodicity_batch',
    'DTW_WORKSPACE_CAP', 'dtw_max_frames', 'dtw_status', 'dtw_check', 'DtwAlignment', 'dtw_align',
    'ALIGN_WORKSPACE_CAP', 'ALIGN_FLAGS', 'align_max_states', 'align_status', 'align_check', 'AlignResult', 'align_viterbi',
    'align_occurrences', 'align_accumulate', 'align_update', 'align_uniform', 'AlignModel', 'forced_align_train',
    'RESAMPLE_MAX_UP', 'RESAMPLE_MAX_TABLE_BYTES', 'HIGHPASS_PADLEN', 'HIGHPASS_MAX_PADLEN', 'PREPROC_MAX_UTTS', 'preproc_check',
    'resample_length', 'resample_table', 'resample', 'highpass_tile', 'highpass_zerophase',
    'LABELS_MAX_LABEL', 'LABELS_CC_POINTS', 'LABELS_ANCHOR_START', 'LABELS_ANCHOR_END', 'LABELS_WILD', 'LABELS_CAPTURE_DIGITS',
    'LABELS_CAPTURE_DECIMAL', 'LABELS_ERR_DIGITS', 'LABELS_ERR_FORMAT', 'LABELS_MODES', 'LABELS_FEATURES', 'labels_match',
    'labels_expand', 'LABELS_SEG_STATES', 'LABELS_SEG_CLAMPED', 'LABELS_SEG_MAX_FRAMES', 'labels_segments',
]


def _dev_tensor(t, dtype, name, shape=None):
    if not (torch.is_tensor(t) and t.is_cuda and t.dtype == dtype and t.is_contiguous()):
        raise _hip.HipLibraryError('{}: expected a contiguous {} device tensor'.format(name, dtype))
    if shape is not None and tuple(t.shape) != tuple(shape):
        raise ValueError('{}: shape {} is not {}'.format(name, tuple(t.shape), tuple(shape)))
    return t


def _no_backward(fn, *tensors):
    if any(t.requires_grad for t in tensors):
        raise ValueError('ops.{} has no backward pass: detach its input'.format(fn))


def _rows2d(t, fn, arg, dims):
    """A contiguous fp32 device matrix with no empty side, e.g. y [R,W] -> its shape."""
    f32c(t, '{}.{}'.format(fn, arg))
    if t.dim() != 2 or min(t.shape) < 1:
        raise ValueError('ops.{}: {} {} is not [{}]'.format(fn, arg, tuple(t.shape), dims))
    return t.shape


def _offsets(t, fn, arg, n):
    """Contiguous int32 device offsets [n+1] of n >= 1 packed items -> n."""
    _dev_tensor(t, torch.int32, '{}.{}'.format(fn, arg))
    if t.dim() != 1 or t.numel() < 2:
        raise ValueError('ops.{}: {} {} is not [{}+1]'.format(fn, arg, tuple(t.shape), n))
    return t.numel() - 1


# ----------------------------------------------------------------------------------------------
# parameter generation (modeltts.py:163-179 -> external/merlin/mlpg_fast.py:95-135)
# ----------------------------------------------------------------------------------------------
MLPG_WORKSPACE_CAP = 256 << 20      # bytes of workspace one ptts_mlpg launch may use; larger batches are split along B


def mlpg_windows(wins):
    """Validate delta windows (one or two, three taps each) -> flat list of 3*len(wins) floats."""
    if wins is None or not 1 <= len(wins) <= 2:
        raise ValueError('MLPG needs one or two delta windows, got {}'.format(0 if wins is None else len(wins)))
    flat = []
    for w in wins:
        if len(w) != 3:
            raise ValueError('an MLPG window has three taps, got {}'.format(list(w)))
        flat.extend(float(c) for c in w)
    return flat


def mlpg(y, wins, var, mean=None, std=None, lengths=None):
    """Maximum-likelihood parameter generation on the device (csrc/mlpg.hip): y [B,T,K*D] (or [T,K*D], treated as B = 1) means,
    or the normalised network output when mean / std [K*D] are given (mu = y*std + mean in fp64); var [K*D] (every frame the
    same) or the shape of y; wins: K-1 three-tap windows; lengths [B] int32 (frames behind an utterance's end come back as 0,
    a length is clamped to [0, T]).  Returns [B,T,D] ([T,D] for a 2-D y).  No autograd node."""
    flat = mlpg_windows(wins)
    K = 1 + len(flat) // 3
    for t in (y, var, mean, std):
        if t is not None and t.requires_grad:
            raise ValueError('ops.mlpg has no backward pass: detach its inputs')
    if (mean is None) != (std is None):
        raise ValueError('ops.mlpg: mean and std go together (both or neither)')
    f32c(y, 'mlpg.y'); f32c(var, 'mlpg.var'); f32c(mean, 'mlpg.mean'); f32c(std, 'mlpg.std')
    squeeze = y.dim() == 2
    y3 = y.unsqueeze(0) if squeeze else y
    if y3.dim() != 3 or y3.shape[-1] % K != 0 or min(y3.shape) < 1:
        raise ValueError('ops.mlpg: y {} is not [B,T,{}*D]'.format(tuple(y.shape), K))
    B, T, KD = y3.shape
    D = KD // K
    per_frame = var.dim() > 1
    if per_frame:
        if squeeze and var.dim() == 2: var = var.unsqueeze(0)
        if var.shape != y3.shape:
            raise ValueError('ops.mlpg: per-frame var {} does not match y {}'.format(tuple(var.shape), tuple(y3.shape)))
    elif var.shape != (KD,):
        raise ValueError('ops.mlpg: var {} is neither [{}] nor the shape of y'.format(tuple(var.shape), KD))
    for t, name in ((mean, 'mean'), (std, 'std')):
        if t is not None and t.shape != (KD,):
            raise ValueError('ops.mlpg: {} {} is not [{}]'.format(name, tuple(t.shape), KD))
    if lengths is not None:
        if not (lengths.is_cuda and lengths.dtype == torch.int32 and lengths.is_contiguous() and lengths.shape == (B,)):
            raise _hip.HipLibraryError('mlpg.lengths: expected a contiguous int32 device tensor of shape [{}]'.format(B))
    wbuf = (ctypes.c_float * len(flat))(*flat)
    out = torch.empty((B, T, D), dtype=torch.float32, device=y.device)
    l = _hip.lib()
    nb = B
    while nb > 1 and l.ptts_mlpg_workspace_bytes(nb, T, D) > MLPG_WORKSPACE_CAP:
        nb = (nb + 1) // 2
    for b0 in range(0, B, nb):
        n = min(nb, B - b0)
        ws = _workspace(l.ptts_mlpg_workspace_bytes(n, T, D), y.device)
        call('ptts_mlpg', ptr(y3[b0:b0 + n]), ptr(mean), ptr(std), ptr(var[b0:b0 + n] if per_frame else var), int(per_frame),
             wbuf, ptr(lengths[b0:b0 + n]) if lengths is not None else None, ptr(out[b0:b0 + n]), ptr(ws), ws.numel(),
             n, T, D, K, stream(), tag=(n, T, D, K))
    return out[0] if squeeze else out


# ----------------------------------------------------------------------------------------------
# feature composition (compose.py:34-183, 239-298): csrc/compose.hip
# ----------------------------------------------------------------------------------------------
NORM_MEANSTD, NORM_MINMAX = 0, 1
COMPOSE_MAX_WINS = 7


def compose_window_taps(wins):
    """Validate composition windows (none .. seven, three taps each) -> flat list of 3*len(wins) floats (fp64 taps)."""
    wins = [] if wins is None else list(wins)
    if len(wins) > COMPOSE_MAX_WINS:
        raise ValueError('compose takes at most {} windows, got {}'.format(COMPOSE_MAX_WINS, len(wins)))
    flat = []
    for w in wins:
        if len(w) != 3:
            raise ValueError('a composition window has three taps, got {}'.format(list(w)))
        flat.extend(float(c) for c in w)
    return flat


def compose_stats_buffers(W, device):
    """Running (min, max, sum) [W] for compose_windows, initialised to (+inf, -inf, 0)."""
    return (torch.full((W,), float('inf'), dtype=torch.float32, device=device),
            torch.full((W,), float('-inf'), dtype=torch.float32, device=device),
            torch.zeros(W, dtype=torch.float64, device=device))


def compose_windows(y, offsets, wins, stats=None, n_stat_utts=0, mlpg_order=False, out=None):
    """y [R,D] fp32 rows of N packed utterances, offsets [N+1] int32 (device) -> [R,K*D]: the statics and one stream per window
    (csrc/compose.hip; `mlpg_order` picks W_k y instead of the reference's -convolve).  stats = (run_min, run_max, run_sum) from
    compose_stats_buffers is updated in place with the rows of the first `n_stat_utts` utterances.  No autograd node."""
    flat = compose_window_taps(wins)
    K = 1 + len(flat) // 3
    R, D = _rows2d(y, 'compose_windows', 'y', 'R,D')
    _no_backward('compose_windows', y)
    if R >= 1 << 31:
        raise ValueError('ops.compose_windows: {} rows exceed the int32 offsets'.format(R))
    N = _offsets(offsets, 'compose_windows', 'offsets', 'N')
    n_stat = min(int(n_stat_utts), N)
    if n_stat < 0 or (n_stat > 0 and stats is None):
        raise ValueError('ops.compose_windows: n_stat_utts={} with stats={}'.format(n_stat_utts, 'None' if stats is None else 'given'))
    W = K * D
    if out is None:
        out = torch.empty((R, W), dtype=torch.float32, device=y.device)
    else:
        f32c(out, 'compose_windows.out')
        if out.shape != (R, W):
            raise ValueError('ops.compose_windows: out {} is not [{},{}]'.format(tuple(out.shape), R, W))
    rmin = rmax = rsum = ws = None
    nws = 0
    if n_stat > 0:
        rmin = _dev_tensor(stats[0], torch.float32, 'compose_windows.run_min', (W,))
        rmax = _dev_tensor(stats[1], torch.float32, 'compose_windows.run_max', (W,))
        rsum = _dev_tensor(stats[2], torch.float64, 'compose_windows.run_sum', (W,))
        nws = _hip.lib().ptts_compose_windows_workspace_bytes(n_stat, D, K)
        ws = _workspace(nws, y.device)
    wbuf = (ctypes.c_double * max(len(flat), 1))(*flat)
    call('ptts_compose_windows', ptr(y), ptr(offsets), wbuf if flat else None, int(bool(mlpg_order)), ptr(out), ptr(rmin), ptr(rmax),
         ptr(rsum), n_stat, ptr(ws), nws, N, R, D, K, stream(), tag=(N, R, D, K))
    return out


def compose_sqdev(y, offsets, mean, run_sq, n_stat_utts):
    """run_sq [W] fp64 += sum over the rows of the first `n_stat_utts` utterances of (double(y) - mean)^2; y [R,W] fp32,
    mean [W] fp64 (device).  The centred second pass of the standard deviation (compose.py:289-296)."""
    R, W = _rows2d(y, 'compose_sqdev', 'y', 'R,W')
    N = _offsets(offsets, 'compose_sqdev', 'offsets', 'N')
    _dev_tensor(mean, torch.float64, 'compose_sqdev.mean', (W,))
    _dev_tensor(run_sq, torch.float64, 'compose_sqdev.run_sq', (W,))
    n_stat = min(int(n_stat_utts), N)
    if n_stat < 0:
        raise ValueError('ops.compose_sqdev: n_stat_utts={}'.format(n_stat_utts))
    if n_stat == 0:
        return run_sq
    nws = _hip.lib().ptts_compose_sqdev_workspace_bytes(n_stat, W)
    ws = _workspace(nws, y.device)
    call('ptts_compose_sqdev', ptr(y), ptr(offsets), ptr(mean), ptr(run_sq), n_stat, ptr(ws), nws, N, R, W, stream(), tag=(N, R, W))
    return run_sq


def compose_normalise(y, a, b, mode=NORM_MEANSTD, scale=1.0, offset=0.0, keepidx=None, out=None):
    """out[r,j] = f(y[r, keepidx[j]]) in fp32 and numpy's operation order: (y - a)/b (NORM_MEANSTD) or
    ((((y - a)/b) - 0.5)*2)*scale + offset (NORM_MINMAX); a, b [Wout] fp32, keepidx [Wout] int32 or None.  out=y runs in place
    (without keepidx)."""
    R, Win = _rows2d(y, 'compose_normalise', 'y', 'R,W')
    if mode not in (NORM_MEANSTD, NORM_MINMAX):
        raise ValueError('ops.compose_normalise: unknown mode {}'.format(mode))
    Wout = Win
    if keepidx is not None:
        _dev_tensor(keepidx, torch.int32, 'compose_normalise.keepidx')
        if keepidx.dim() != 1 or keepidx.numel() < 1:
            raise ValueError('ops.compose_normalise: keepidx {} is not [Wout]'.format(tuple(keepidx.shape)))
        Wout = keepidx.numel()
    _dev_tensor(a, torch.float32, 'compose_normalise.a', (Wout,))
    _dev_tensor(b, torch.float32, 'compose_normalise.b', (Wout,))
    if out is None:
        out = torch.empty((R, Wout), dtype=torch.float32, device=y.device)
    else:
        f32c(out, 'compose_normalise.out')
        if out.shape != (R, Wout):
            raise ValueError('ops.compose_normalise: out {} is not [{},{}]'.format(tuple(out.shape), R, Wout))
        if keepidx is not None and out.data_ptr() == y.data_ptr():
            raise ValueError('ops.compose_normalise: a column gather cannot run in place')
    call('ptts_compose_normalise', ptr(y), ptr(keepidx), ptr(a), ptr(b), int(mode), float(scale), float(offset), ptr(out), R, Win,
         Wout, stream(), tag=(R, Win, Wout, mode))
    return out


# ----------------------------------------------------------------------------------------------
# spectral envelope decompression and the mel-cepstral post-filter (vocoders.py:147-166,
# external/merlin/generate_pp.py): csrc/spectrum.hip
# ----------------------------------------------------------------------------------------------
SPECTRUM_MAX_M1, SPECTRUM_MAX_NB, SPECTRUM_MAX_DFTLEN = 512, 1024, 1 << 20
_spectrum_tables = {}       # (kind, device, parameters) -> device table; a function of its key only, so never stale


def spectrum_check(dftlen, alpha, pf_coef):
    """ValueError for a dftlen / alpha / pf_coef the spectrum kernels do not take.  Touches no device."""
    if int(dftlen) != dftlen or dftlen < 8 or dftlen % 2 != 0 or dftlen > SPECTRUM_MAX_DFTLEN:
        raise ValueError('dftlen={} has to be even, at least 8 and at most {}'.format(dftlen, SPECTRUM_MAX_DFTLEN))
    if not -1.0 < float(alpha) < 1.0:
        raise ValueError('|alpha|={} has to be below 1'.format(alpha))
    if not 0.0 < float(pf_coef) < 1e6:
        raise ValueError('pf_coef={} has to be positive'.format(pf_coef))


def _spectrum_rows(x, name, lo, hi, what):
    """[T,W] or [B,T,W] fp32 device rows -> (x, T_total, W); ValueError for a shape or width that cannot be, before f32c looks at
    the device."""
    if not torch.is_tensor(x) or x.dim() not in (2, 3):
        raise ValueError('ops.{}: expected a [T,{w}] or [B,T,{w}] tensor'.format(name, w=what))
    W = x.shape[-1]
    if not lo <= W <= hi:
        raise ValueError('ops.{}: {}={} outside [{}, {}]'.format(name, what, W, lo, hi))
    _no_backward(name, x)
    rows = x.numel() // W
    if rows >= 1 << 31:
        raise ValueError('ops.{}: {} frames exceed the int32 frame count'.format(name, rows))
    f32c(x, name)
    return x, rows, W


def _device_table(kind, device, params, dtype, size_args, args=None):
    """(table, bytes) of ptts_<kind>_table(table, bytes, *args) on `device`, made once per (kind, device, params): a flat `dtype`
    tensor of ptts_<kind>_table_bytes(*size_args) bytes.  params = (order or bands, .., dftlen); args: params unless given."""
    key = (kind, device) + params
    tab = _spectrum_tables.get(key)
    if tab is None:
        n = getattr(_hip.lib(), 'ptts_{}_table_bytes'.format(kind))(*size_args)
        tab = torch.empty(n // dtype.itemsize, dtype=dtype, device=device)
        call('ptts_{}_table'.format(kind), ptr(tab), n, *(params if args is None else args), stream(), tag=(params[0], params[-1]))
        _spectrum_tables[key] = tab
    return tab, tab.numel() * dtype.itemsize


def _mcep_table(device, M1, alpha, dftlen):
    return _device_table('mcep', device, (M1, float(alpha), dftlen), torch.float32, (M1, dftlen))


def _fwbnd_table(device, nb, fs, alpha, dftlen):
    return _device_table('fwbnd', device, (nb, float(fs), float(alpha), dftlen), torch.float64, (dftlen,))


def bark_alpha(fs):
    """The all-pass coefficient that approximates the Bark scale at sampling frequency fs (the reference's sp.bark_alpha)."""
    return 0.8517 * math.sqrt(math.atan(0.06583 * fs / 1000.0)) - 0.1916


def mcep_postfilter(mcep, alpha, dftlen=4096, pf_coef=1.4):
    """Merlin's formant-enhancing post-filter on mel-cepstra (csrc/spectrum.hip): mcep [T,M1] or [B,T,M1] fp32 device ->
    same shape.  Coefficients 2.. are scaled by pf_coef; c_0 is corrected so that the frame's energy r0 is kept."""
    spectrum_check(dftlen, alpha, pf_coef)
    mcep, T, M1 = _spectrum_rows(mcep, 'mcep_postfilter', 2, SPECTRUM_MAX_M1, 'M1')
    out = torch.empty_like(mcep)
    if T == 0:
        return out
    tab, nb = _mcep_table(mcep.device, M1, alpha, dftlen)
    call('ptts_mcep_postfilter', ptr(mcep), ptr(out), T, M1, float(alpha), int(dftlen), float(pf_coef), ptr(tab), nb, stream(),
         tag=(T, M1, dftlen))
    return out


def mcep2spec(mcep, alpha, dftlen=4096, log=False, pp=False, pf_coef=1.4):
    """Mel-cepstra [T,M1] or [B,T,M1] fp32 device -> amplitude envelope [.., dftlen/2+1] (`log`: its logarithm); `pp`: of the
    post-filtered cepstrum, which is never stored (csrc/spectrum.hip)."""
    spectrum_check(dftlen, alpha, pf_coef)
    mcep, T, M1 = _spectrum_rows(mcep, 'mcep2spec', 2, SPECTRUM_MAX_M1, 'M1')
    out = torch.empty(tuple(mcep.shape[:-1]) + (dftlen // 2 + 1,), dtype=torch.float32, device=mcep.device)
    if T == 0:
        return out
    tab, nb = _mcep_table(mcep.device, M1, alpha, dftlen)
    call('ptts_mcep2spec', ptr(mcep), ptr(out), T, M1, float(alpha), int(dftlen), int(bool(log)), int(bool(pp)), float(pf_coef),
         ptr(tab), nb, stream(), tag=(T, M1, dftlen))
    return out


def fwbnd2spec(fw, fs, dftlen=4096, log=False, pp=False, pf_coef=1.4):
    """Log-amplitudes of nb frequency-warped bands [T,nb] or [B,T,nb] fp32 device -> amplitude envelope [.., dftlen/2+1] (`log`:
    its logarithm) by linear interpolation between the band centres; `pp`: with the spectral-domain post-filter
    (csrc/spectrum.hip)."""
    if not 0.0 < float(fs) < 1e9:
        raise ValueError('fs={} has to be positive'.format(fs))
    alpha = bark_alpha(fs)
    spectrum_check(dftlen, alpha, pf_coef)
    fw, T, nbands = _spectrum_rows(fw, 'fwbnd2spec', 2, SPECTRUM_MAX_NB, 'nb')
    out = torch.empty(tuple(fw.shape[:-1]) + (dftlen // 2 + 1,), dtype=torch.float32, device=fw.device)
    if T == 0:
        return out
    tab, nbytes = _fwbnd_table(fw.device, nbands, fs, alpha, dftlen)
    call('ptts_fwbnd2spec', ptr(fw), ptr(out), T, nbands, float(fs), float(alpha), int(dftlen), int(bool(log)), int(bool(pp)),
         float(pf_coef), ptr(tab), nbytes, stream(), tag=(T, nbands, dftlen))
    return out


SPEC2MCEP_MAX_TABLE_BYTES = 32 << 20      # the table of one (M1, alpha, dftlen): W and the scratch of its build


def spec2mcep_order_limit(alpha, dftlen):
    """The largest M1 = order + 1 whose fit is well conditioned: floor((dftlen/2) (1 - |alpha|) / (1 + |alpha|)).  Beyond it the
    widest node spacing on the warped axis no longer resolves cos(m wt) and the normal matrix turns singular."""
    return int(math.floor(float(dftlen // 2) * (1.0 - abs(float(alpha))) / (1.0 + abs(float(alpha)))))


def spec2mcep_table_bytes(M1, dftlen):
    """What ptts_spec2mcep_table_bytes returns, on the host: fp64 W [K][M1p], nodes [2][Kp], sums [2 M1p], factor [M1][M1]."""
    K, Kp, M1p = dftlen // 2 + 1, (dftlen // 2 + 1 + 3) // 4 * 4, (M1 + 3) // 4 * 4
    return (8 * (K * M1p + 2 * Kp + 2 * M1p + M1 * M1) + 255) // 256 * 256


def spec2mcep_check(order, alpha, dftlen):
    """ValueError for an (order, alpha, dftlen) the mel-cepstral fit does not take, the conditions of ptts_spec2mcep: dftlen and
    alpha as spectrum_check, 2 <= order + 1 <= SPECTRUM_MAX_M1, order + 1 within spec2mcep_order_limit, the table within
    SPEC2MCEP_MAX_TABLE_BYTES.  Touches no device."""
    spectrum_check(dftlen, alpha, 1.4)
    if int(order) != order or not 1 <= order <= SPECTRUM_MAX_M1 - 1:
        raise ValueError('order={} outside [1, {}]'.format(order, SPECTRUM_MAX_M1 - 1))
    M1, limit = int(order) + 1, spec2mcep_order_limit(alpha, dftlen)
    if M1 > limit:
        raise ValueError('order={}: order + 1 is above floor((dftlen/2) (1 - |alpha|) / (1 + |alpha|)) = {} at alpha={}, dftlen={}; '
                         'the fit is singular beyond it'.format(order, limit, alpha, dftlen))
    if spec2mcep_table_bytes(M1, int(dftlen)) > SPEC2MCEP_MAX_TABLE_BYTES:
        raise ValueError('order={} at dftlen={}: the table takes {} bytes, above {}'.format(
            order, dftlen, spec2mcep_table_bytes(M1, int(dftlen)), SPEC2MCEP_MAX_TABLE_BYTES))


def _spec2mcep_table(device, M1, alpha, dftlen):
    return _device_table('spec2mcep', device, (M1, float(alpha), dftlen), torch.float64, (M1, dftlen))


def spec2mcep(spec, alpha, order, log=False):
    """Amplitude envelope [T,K] or [B,T,K] fp32 device, K = dftlen/2 + 1 bins (`log`: its logarithm) -> mel-cepstra [.., order+1]:
    the least-squares fit of sum_m c_m cos(m wt_k) to ln max(|spec|, FLT_MIN) under the trapezoid weights of the warped axis
    (csrc/spectrum.hip), so that spec2mcep(mcep2spec(c)) = c up to rounding.  The argument order is the
    reference's sp.spec2mcep(SPEC, alpha, order); dftlen is read off K.  The reference's call scales the envelope by fs first
    (vocoders.py:141), which adds ln fs to c_0 and which its own decompress_spectrum does not undo; that is not reproduced: this
    is the inverse of the build's mcep2spec."""
    if not torch.is_tensor(spec) or spec.dim() not in (2, 3):
        raise ValueError('ops.spec2mcep: expected a [T,K] or [B,T,K] tensor')
    K = spec.shape[-1]
    if K < 5 or K > SPECTRUM_MAX_DFTLEN // 2 + 1:
        raise ValueError('ops.spec2mcep: K={} is not dftlen/2 + 1 of a dftlen in [8, {}]'.format(K, SPECTRUM_MAX_DFTLEN))
    dftlen = 2 * (K - 1)
    spec2mcep_check(order, alpha, dftlen)
    spec, T, K = _spectrum_rows(spec, 'spec2mcep', 5, SPECTRUM_MAX_DFTLEN // 2 + 1, 'K')
    M1 = int(order) + 1
    out = torch.empty(tuple(spec.shape[:-1]) + (M1,), dtype=torch.float32, device=spec.device)
    if T == 0:
        return out
    tab, nbytes = _spec2mcep_table(spec.device, M1, alpha, dftlen)
    call('ptts_spec2mcep', ptr(spec), ptr(out), T, M1, float(alpha), dftlen, int(bool(log)), ptr(tab), nbytes, stream(),
         tag=(T, M1, dftlen))
    return out


# ----------------------------------------------------------------------------------------------
# pulse-and-noise waveform synthesis of the PML vocoder (the step behind vocoders.py:194-206): csrc/pulsesynth.hip
# ----------------------------------------------------------------------------------------------
PULSE_MIN_DFTLEN, PULSE_MAX_DFTLEN = 256, 8192
PULSE_F0_FLOOR = 50.0
PULSE_INT_ROWS = ('start', 'winlen', 'lb', 'rb', 'fr')


def pulse_check(dftlen, fs):
    """ValueError for a dftlen / fs the synthesis kernels do not take.  Touches no device."""
    if int(dftlen) != dftlen or not PULSE_MIN_DFTLEN <= dftlen <= PULSE_MAX_DFTLEN or dftlen & (dftlen - 1):
        raise ValueError('dftlen={} has to be a power of two in [{}, {}]'.format(dftlen, PULSE_MIN_DFTLEN, PULSE_MAX_DFTLEN))
    if not 0.0 < float(fs) < 1e9:
        raise ValueError('fs={} has to be positive'.format(fs))


def _rnd(x):
    return int(math.floor(x + 0.5))


def _pulse_table(fn, world, f0, voiced, shift, fs, wavlen, dftlen):
    """ops.pulse_table and, with `world`, ops.world_pulse_table.  The two differ in the rate at t (the interpolated f0 everywhere,
    or WORLD_UNVOICED_RATE where the nearest frame is unvoiced), in the lead of a pulse over its window (a quarter of the pulse's
    window, or of the 50-ms window for every pulse) and in the rows 'w', 'i0', 'i1', 'v' that only WORLD has."""
    pulse_check(dftlen, fs)
    f0 = np.ascontiguousarray(f0, dtype=np.float64)
    if f0.ndim != 1 or f0.size < 1 or not (np.isfinite(f0).all() and (f0 > 0).all()):
        raise ValueError('ops.{}: f0 has to be [T] positive finite Hz values'.format(fn))
    if world:
        voiced = np.asarray(voiced)
        if voiced.shape != f0.shape or voiced.dtype.kind not in 'biu':
            raise ValueError('ops.{}: voiced has to be [T] booleans'.format(fn))
        voiced = voiced.astype(bool)
    if not 0.0 < float(shift) < 1e3:
        raise ValueError('ops.{}: shift={}'.format(fn, shift))
    T, fs, shift = f0.size, float(fs), float(shift)
    if int(wavlen) != int(round(shift * (T - 1) * fs)) or wavlen >= 1 << 31:
        raise ValueError('ops.{}: wavlen={} is not round(shift (T-1) fs) = {}'.format(fn, wavlen, int(round(shift * (T - 1) * fs))))
    wavlen = int(wavlen)
    times = shift * np.arange(T)
    frame = lambda x: min(max(_rnd(x / shift), 0), T - 1)
    f0_at = lambda x: max(float(np.interp(x, times, f0)), PULSE_F0_FLOOR)
    rate = (lambda x: f0_at(x) if voiced[frame(x)] else WORLD_UNVOICED_RATE) if world else f0_at
    t = [0.0]
    while t[-1] < wavlen / fs:
        t.append(t[-1] + 1.0 / rate(t[-1]))
    P = len(t)
    tab = {'t': np.array(t, dtype=np.float64)}
    for key in ('delay', 'f0', 'w') if world else ('delay', 'f0'):
        tab[key] = np.zeros(P, dtype=np.float64)
    for key in WORLD_INT_ROWS if world else PULSE_INT_ROWS:
        tab[key] = np.zeros(P, dtype=np.int32)
    for n in range(P):
        f0n = rate(t[n])
        winlen = 2 * int(max(0.050 * fs, 4.0 * fs / f0n) / 2) + 1
        if winlen > dftlen:
            raise ValueError('ops.{}: the window of pulse {} ({} samples at f0 = {:.1f} Hz) does not fit dftlen={}'.format(
                fn, n, winlen, f0n, dftlen))
        pos = int((2 * int(0.050 * fs / 2) + 1) / 4) if world else int(winlen / 4)
        c = _rnd(fs * t[n])
        lb = _rnd(fs * (t[n - 1] + t[n]) / 2) if n > 0 else _rnd(fs * (t[n] - 0.5 / f0n))
        rb = _rnd(fs * (t[n] + t[n + 1]) / 2) if n < P - 1 else _rnd(fs * (t[n] + 0.5 / f0n))
        tab['start'][n], tab['winlen'][n] = c - pos, winlen
        tab['lb'][n], tab['rb'][n] = min(max(lb, 0), wavlen), min(max(rb, 0), wavlen)
        tab['fr'][n] = frame(t[n])
        tab['delay'][n], tab['f0'][n] = pos + (fs * t[n] - c), f0n
        if world:
            i0 = min(int(t[n] / shift), T - 1)
            tab['i0'][n], tab['i1'][n] = i0, min(i0 + 1, T - 1)
            tab['w'][n] = t[n] / shift - i0 if i0 < T - 1 else 0.0
            tab['v'][n] = int(voiced[tab['fr'][n]])
    return tab


def pulse_table(f0, shift, fs, wavlen, dftlen):
    """The pulse positions of one utterance and everything the kernels need per pulse, on the host in fp64:
    f0 [T] in Hz at the frame times shift * i (values below 50 Hz are synthesised at 50 Hz), wavlen = round(shift (T-1) fs).
    Returns a dict of numpy arrays, one entry per pulse: 't' fp64 (t_0 = 0, t_{n+1} = t_n + 1 / f0(t_n), the last one at or beyond
    the end), the int32 rows 'start', 'winlen', 'lb', 'rb', 'fr' and the fp64 rows 'delay', 'f0'.  The noise segments [lb, rb) tile
    [0, wavlen).  ValueError when a window does not fit dftlen."""
    return _pulse_table('pulse_table', False, f0, None, shift, fs, wavlen, dftlen)


def _pulse_table_rows(table, T, dftlen, wavlen, fn='pulse_synthesis', maker='pulse_table', int_rows=PULSE_INT_ROWS,
                      dbl_rows=('delay', 'f0')):
    """(itab [len(int_rows),P] int32, dtab [len(dbl_rows),P] fp64, W) of a pulse table after the checks that keep the kernels inside
    their buffers; the first five int rows are PULSE_INT_ROWS, the first two fp64 rows delay and f0."""
    try:
        rows = [np.asarray(table[k]) for k in int_rows + dbl_rows]
    except (KeyError, TypeError, IndexError):
        raise ValueError('ops.{}: table is what ops.{} returns'.format(fn, maker))
    ni, nd = len(int_rows), len(dbl_rows)
    P = rows[0].shape[0] if rows[0].ndim == 1 else -1
    if any(r.shape != (P,) for r in rows):
        raise ValueError('ops.{}: the rows of the table are not all [P]'.format(fn))
    itab = np.ascontiguousarray(np.stack(rows[:ni]) if P else np.zeros((ni, 0)), dtype=np.int64)
    dtab = np.ascontiguousarray(np.stack(rows[ni:]) if P else np.zeros((nd, 0)), dtype=np.float64)
    if P == 0:
        return itab.astype(np.int32), dtab, 1
    start, winlen, lb, rb, fr = itab[:5]
    if winlen.min() < 1 or winlen.max() > dftlen:
        raise ValueError('ops.{}: a window of {} samples does not fit dftlen={}'.format(fn, winlen.max(), dftlen))
    if (np.diff(start) < 0).any():
        raise ValueError('ops.{}: the pulses\' start samples have to ascend (f0 falls too fast between two pulses)'.format(fn))
    filled = rb > lb
    if lb.min() < 0 or rb.max() > wavlen or (rb < lb).any() or (filled & ((lb < start) | (rb - start > dftlen))).any():
        raise ValueError('ops.{}: a noise segment lies outside the waveform or its pulse\'s frame'.format(fn))
    if fr.min() < 0 or fr.max() >= T:
        raise ValueError('ops.{}: frame {} of the table is outside the {} frames given'.format(fn, fr.max(), T))
    if not (np.isfinite(dtab).all() and (dtab[1] > 0).all()):
        raise ValueError('ops.{}: delay / f0 of the table are not finite and positive'.format(fn))
    if np.abs(start).max() >= 1 << 30:
        raise ValueError('ops.{}: a start sample exceeds the int32 table'.format(fn))
    return itab.astype(np.int32), dtab, int(winlen.max())


def _band_rows(fn, bands, bands_name, width, per_frame, per_frame_name, fs, dftlen):
    """ops.noise_mask and ops.aper_rows: bands [T,width] and one value per frame [T] (fp32 device) -> [T, dftlen/2+1] from
    ptts_<fn>, which reads the band axis of fwbnd2spec."""
    pulse_check(dftlen, fs)
    if not torch.is_tensor(bands) or bands.dim() != 2 or not 2 <= bands.shape[1] <= SPECTRUM_MAX_NB:
        raise ValueError('ops.{}: expected a [T,{w}] tensor with {w} in [2, {}]'.format(fn, SPECTRUM_MAX_NB, w=width))
    T, nbands = bands.shape
    if not torch.is_tensor(per_frame) or tuple(per_frame.shape) != (T,):
        raise ValueError('ops.{}: {} is not [{}]'.format(fn, per_frame_name, T))
    _no_backward(fn, bands, per_frame)
    f32c(bands, '{}.{}'.format(fn, bands_name)); f32c(per_frame, '{}.{}'.format(fn, per_frame_name))
    out = torch.empty((T, dftlen // 2 + 1), dtype=torch.float32, device=bands.device)
    if T == 0:
        return out
    tab, nbytes = _fwbnd_table(bands.device, nbands, fs, bark_alpha(fs), dftlen)
    call('ptts_' + fn, ptr(bands), ptr(per_frame), ptr(out), T, nbands, float(fs), int(dftlen), ptr(tab), nbytes, stream(),
         tag=(T, nbands, dftlen))
    return out


def _segments_synthesis(fn, segments, maker, int_rows, dbl_rows, spec, rows, rows_name, table, noise, fs, dftlen, wavlen,
                        check_table=None):
    """ops.pulse_synthesis and ops.world_synthesis: the argument checks, the table of ops.<maker> on the device, the kernel
    `segments` (one workgroup per pulse), then the overlap-add.  rows: the [T,K] input beside spec; check_table(itab, dtab, T):
    what a synthesiser asks of its own table rows."""
    pulse_check(dftlen, fs)
    K = dftlen // 2 + 1
    if not torch.is_tensor(spec) or spec.dim() != 2 or spec.shape[1] != K:
        raise ValueError('ops.{}: spec is not [T,{}]'.format(fn, K))
    T = spec.shape[0]
    if not torch.is_tensor(rows) or tuple(rows.shape) != (T, K):
        raise ValueError('ops.{}: {} is not [{},{}]'.format(fn, rows_name, T, K))
    wavlen = int(wavlen)
    if wavlen < 0 or not torch.is_tensor(noise) or tuple(noise.shape) != (wavlen,):
        raise ValueError('ops.{}: noise is not [wavlen={}]'.format(fn, wavlen))
    _no_backward(fn, spec, rows, noise)
    f32c(spec, '{}.spec'.format(fn)); f32c(rows, '{}.{}'.format(fn, rows_name)); f32c(noise, '{}.noise'.format(fn))
    itab, dtab, W = _pulse_table_rows(table, T, dftlen, wavlen, fn, maker, int_rows, dbl_rows)
    if check_table is not None:
        check_table(itab, dtab, T)
    P = itab.shape[1]
    wav = torch.empty(wavlen, dtype=torch.float32, device=spec.device)
    if wavlen == 0:
        return wav
    if P == 0 or T == 0:
        return wav.zero_()
    it = torch.from_numpy(itab).to(spec.device)
    dt = torch.from_numpy(dtab).to(spec.device)
    seg = torch.empty((P, W), dtype=torch.float32, device=spec.device)
    call(segments, ptr(spec), ptr(rows), ptr(noise), ptr(it), ptr(dt), P, T, int(dftlen), float(fs), wavlen, ptr(seg), W, stream(),
         tag=(P, dftlen, W))
    call('ptts_pulse_overlap_add', ptr(seg), ptr(it), P, W, ptr(wav), wavlen, stream(), tag=(P, W, wavlen))
    return wav


def noise_mask(nmb, f0, fs, dftlen=4096):
    """Noise-mask bands [T,nb] in [0,1] and f0 [T] in Hz (fp32 device) -> the binary mask smoothed along frequency, [T, dftlen/2+1]
    (csrc/pulsesynth.hip): interpolation at k fs / dftlen on the band axis of fwbnd2spec, zero below the second harmonic, threshold at
    0.5, a forward-backward pass of hanning(9), clip."""
    return _band_rows('noise_mask', nmb, 'nmb', 'nb', f0, 'f0', fs, dftlen)


def pulse_synthesis(spec, mask, table, noise, fs, dftlen, wavlen):
    """The waveform [wavlen] (fp32 device) of one utterance: spec and mask [T, dftlen/2+1] fp32 device, table from
    ops.pulse_table (host), noise [wavlen] N(0,1) fp32 device.  One workgroup per pulse builds its segment (minimum-phase envelope
    times the mix of a delayed pulse and the pulse's stretch of the noise), then one lane per sample adds the segments that cover
    it, in pulse order (csrc/pulsesynth.hip).  Same input, same bytes."""
    return _segments_synthesis('pulse_synthesis', 'ptts_pulse_segments', 'pulse_table', PULSE_INT_ROWS, ('delay', 'f0'), spec, mask, 'mask',
                               table, noise, fs, dftlen, wavlen)


# ----------------------------------------------------------------------------------------------
# periodic-plus-aperiodic synthesis for the WORLD parameters (the step behind vocoders.py:300-330, which calls pyworld; the
# definition is the build's own): csrc/worldsynth.hip
# ----------------------------------------------------------------------------------------------
WORLD_UNVOICED_RATE = 500.0         # pulses per second through an unvoiced frame (WORLD's default F0): noise in 2-ms pieces
WORLD_INT_ROWS = PULSE_INT_ROWS + ('i0', 'i1', 'v')


def world_pulse_table(f0, voiced, shift, fs, wavlen, dftlen):
    """The pulse table of ops.pulse_table for the WORLD synthesiser, on the host in fp64: f0 [T] in Hz
    (continuous: positive in unvoiced frames too) and voiced [T] booleans at the frame times shift * i.  The rate at t is
    max(interp(t), 50) where the frame nearest to t is voiced and 500 Hz where it is not; every pulse leads its window by the same
    pos = int((2 int(0.050 fs / 2) + 1) / 4) samples, whatever its winlen, so start ascends with t.  Returns ops.pulse_table's
    entries ('f0' is the rate at the pulse) and, per pulse, the frames 'i0', 'i1' (int32) whose rows are blended with the weight
    'w' (fp64) on i1, and 'v' (int32), 1 where frame 'fr' is voiced.  ValueError when a window does not fit dftlen."""
    return _pulse_table('world_pulse_table', True, f0, voiced, shift, fs, wavlen, dftlen)


def aper_rows(aper_db, vuv, fs, dftlen=4096):
    """Band aperiodicities [T,A] in dB and vuv [T] (fp32 device) -> the aperiodicity of every bin, [T, dftlen/2+1] in [0, 1]
    (csrc/worldsynth.hip): 10^(x/20) per band, those values interpolated at k fs / dftlen on the band axis of fwbnd2spec, clipped;
    the row of an unvoiced frame (vuv < 0.5) is 1 throughout."""
    return _band_rows('aper_rows', aper_db, 'aper_db', 'A', vuv, 'vuv', fs, dftlen)


def world_synthesis(spec, aper, table, noise, fs, dftlen, wavlen):
    """The waveform [wavlen] (fp32 device) of one utterance: spec (amplitude envelope) and aper (ops.aper_rows) [T, dftlen/2+1] fp32
    device, table from ops.world_pulse_table (host), noise [wavlen] N(0,1) fp32 device.  One workgroup per pulse blends the rows of
    its two frames and builds its segment (the minimum-phase periodic filter times a delayed pulse, for a voiced pulse, plus the
    minimum-phase aperiodic filter times the pulse's stretch of the noise), then ops.pulse_synthesis's overlap-add sums the
    segments in pulse order (csrc/worldsynth.hip, csrc/pulsesynth.hip).  Same input, same bytes."""
    def frames_and_weight(itab, dtab, T):
        if itab.shape[1] and (itab[5:7].min() < 0 or itab[5:7].max() >= T or not ((dtab[2] >= 0) & (dtab[2] <= 1)).all()):
            raise ValueError('ops.world_synthesis: the frames i0 / i1 or the weight w of the table are outside the {} frames given'.format(T))
    return _segments_synthesis('world_synthesis', 'ptts_world_segments', 'world_pulse_table', WORLD_INT_ROWS, ('delay', 'f0', 'w'), spec, aper,
                               'aper', table, noise, fs, dftlen, wavlen, frames_and_weight)


# ----------------------------------------------------------------------------------------------
# the pulse table on the device and both synthesisers over a batch of utterances: csrc/pulsetable.hip
# ----------------------------------------------------------------------------------------------
PULSE_F0_CAP = 1000.0               # the default f0_cap of pulse_table_device
PULSE_MAX_UTTS = 65535              # utterances of one launch
# (status bit of include/percival_hip.h, what the ValueError says); the first four are set by the walk, the others by the rows
_PULSE_STATUS = tuple((_hip._define('PTTS_PULSE_' + name), text) for name, text in (
    ('BAD_F0', 'f0 has to be [T] positive finite Hz values'),
    ('WINDOW', 'the window of a pulse ({maxwin} samples) does not fit dftlen={dftlen}'),
    ('TOO_MANY', 'more than cap={cap} pulses'),
    ('RATE', 'a rate above f0_cap={f0_cap} Hz'),
    ('DESCENDING', 'the pulses\' start samples have to ascend (f0 falls too fast between two pulses)'),
    ('SEGMENT', 'a noise segment lies outside the waveform or its pulse\'s frame'),
    ('START_RANGE', 'a start sample exceeds the int32 table')))


def pulse_table_cap(T_max, shift, f0_cap=PULSE_F0_CAP):
    """Pulse slots per utterance of pulse_table_device: ceil(shift (T_max - 1) max(f0_cap, WORLD_UNVOICED_RATE)) + 2.  Touches no
    device."""
    if int(T_max) != T_max or T_max < 1 or not 0.0 < float(shift) < 1e3 or not 0.0 < float(f0_cap) < 1e9:
        raise ValueError('ops.pulse_table_cap: T_max={} shift={} f0_cap={}'.format(T_max, shift, f0_cap))
    return int(math.ceil(float(shift) * (int(T_max) - 1) * max(float(f0_cap), WORLD_UNVOICED_RATE))) + 2


def _pulse_batch_layout(fn, lengths, shift, fs, dftlen, f0_cap):
    """The checks of pulse_table_device that need no device -> (lengths, wavlens, frame_off, sample_off, cap)."""
    pulse_check(dftlen, fs)
    try:
        lengths = [int(n) for n in lengths]
    except (TypeError, ValueError):
        raise ValueError('ops.{}: lengths has to be the utterances\' frame counts'.format(fn))
    if not 1 <= len(lengths) <= PULSE_MAX_UTTS or min(lengths) < 1:
        raise ValueError('ops.{}: lengths has to hold 1 to {} frame counts of at least 1'.format(fn, PULSE_MAX_UTTS))
    if not 0.0 < float(shift) < 1e3:
        raise ValueError('ops.{}: shift={}'.format(fn, shift))
    if not 0.0 < float(f0_cap) < 1e9:
        raise ValueError('ops.{}: f0_cap={} has to be positive'.format(fn, f0_cap))
    fs, shift = float(fs), float(shift)
    wavlens = [int(round(shift * (T - 1) * fs)) for T in lengths]
    frame_off = np.concatenate([[0], np.cumsum(lengths, dtype=np.int64)])
    sample_off = np.concatenate([[0], np.cumsum(wavlens, dtype=np.int64)])
    cap = pulse_table_cap(max(lengths), shift, f0_cap)
    if frame_off[-1] >= 1 << 30 or sample_off[-1] >= 1 << 30 or cap * len(lengths) >= 1 << 28:
        raise ValueError('ops.{}: {} frames, {} samples or {} pulse slots exceed the int32 tables'.format(
            fn, frame_off[-1], sample_off[-1], cap * len(lengths)))
    return lengths, wavlens, frame_off, sample_off, cap


class PulseTableDevice(object):
    """What pulse_table_device returns.  On the device: t [B,cap] fp64 (utterance b's pulse times in t[b, :counts[b]]); itab
    [5,P] or [8,P] int32 and dtab [2,P] or [3,P] fp64, the rows of ops.pulse_table / ops.world_pulse_table with all utterances one
    after the other along P, every value relative to its own utterance; itab_packed, the same with fr / i0 / i1 shifted by the
    utterance's first frame and start / lb / rb by its first sample, which the segment kernels read on packed buffers (winlen is 0
    there for the one pulse of an utterance without samples); offs [2,B+1] int64 and pulse_off_dev [B+1] int32.  On the host:
    world, lengths, wavlens, counts, pulse_off, frame_off, sample_off (numpy int64, offsets [B+1]), P, W (the largest winlen), cap,
    shift, fs, dftlen."""

    def rows(self, b):
        """Utterance b's table as the dict of numpy arrays that ops.pulse_table / ops.world_pulse_table return."""
        if not 0 <= b < len(self.lengths):
            raise IndexError('utterance {} of {}'.format(b, len(self.lengths)))
        p0, p1 = int(self.pulse_off[b]), int(self.pulse_off[b + 1])
        itab, dtab = self.itab[:, p0:p1].cpu().numpy(), self.dtab[:, p0:p1].cpu().numpy()
        tab = {'t': self.t[b, :p1 - p0].cpu().numpy()}
        for key, row in zip(('delay', 'f0', 'w') if self.world else ('delay', 'f0'), dtab):
            tab[key] = np.ascontiguousarray(row)
        for key, row in zip(WORLD_INT_ROWS if self.world else PULSE_INT_ROWS, itab):
            tab[key] = np.ascontiguousarray(row)
        return tab


def pulse_table_device(f0, lengths, shift, fs, dftlen, voiced=None, f0_cap=PULSE_F0_CAP):
    """ops.pulse_table, or with `voiced` ops.world_pulse_table, of a batch of utterances, built by two kernels
    (csrc/pulsetable.hip) and bit for bit the host's: f0 [sum T] fp32 device in Hz, the utterances one after the other, lengths
    their frame counts T_b (wavlen_b = round(shift (T_b - 1) fs)), voiced [sum T] bool or uint8 device.  One wave per utterance
    walks t_{n+1} = t_n + 1 / rate(t_n), one lane per pulse fills the rows; the host reads the counts, the largest window and the
    status words back once and does nothing per pulse.  Returns a PulseTableDevice.

    f0_cap bounds the table's memory: an utterance gets cap = ops.pulse_table_cap(max T, shift, f0_cap) pulse slots, and a
    voiced rate above f0_cap is refused.  The default, 1000 Hz, lies above any f0_max a vocoder of this build is configured with.

    What ops.pulse_table refuses is a ValueError here too, raised after the read-back; it names the utterance's index in the
    batch.  Nothing of such a batch is to be synthesised."""
    fn = 'pulse_table_device'
    lengths, wavlens, frame_off, sample_off, cap = _pulse_batch_layout(fn, lengths, shift, fs, dftlen, f0_cap)
    B, total = len(lengths), int(frame_off[-1])
    f32c(f0, fn + '.f0')
    if tuple(f0.shape) != (total,):
        raise ValueError('ops.{}: f0 {} is not [sum(lengths)={}]'.format(fn, tuple(f0.shape), total))
    _no_backward(fn, f0)
    world = voiced is not None
    if world:
        if not (torch.is_tensor(voiced) and voiced.is_cuda and voiced.dtype in (torch.bool, torch.uint8) and voiced.is_contiguous()):
            raise _hip.HipLibraryError('{}.voiced: expected a contiguous bool or uint8 device tensor'.format(fn))
        if tuple(voiced.shape) != (total,):
            raise ValueError('ops.{}: voiced {} is not [sum(lengths)={}]'.format(fn, tuple(voiced.shape), total))
    dev = f0.device
    ni, nd = (len(WORLD_INT_ROWS), 3) if world else (len(PULSE_INT_ROWS), 2)
    tab = PulseTableDevice()
    tab.world, tab.lengths, tab.wavlens, tab.frame_off, tab.sample_off = world, lengths, wavlens, frame_off, sample_off
    tab.cap, tab.shift, tab.fs, tab.dftlen = cap, float(shift), float(fs), int(dftlen)
    tab.offs = torch.from_numpy(np.stack([frame_off, sample_off])).to(dev)
    tab.t = torch.empty((B, cap), dtype=torch.float64, device=dev)
    tab.pulse_off_dev = torch.empty(B + 1, dtype=torch.int32, device=dev)
    info = torch.empty((B, 4), dtype=torch.int32, device=dev)
    irel = torch.empty(ni * B * cap, dtype=torch.int32, device=dev)
    ioff = torch.empty(ni * B * cap, dtype=torch.int32, device=dev)
    dbl = torch.empty(nd * B * cap, dtype=torch.float64, device=dev)
    args = (ptr(f0), ptr(voiced), ptr(tab.offs), B, tab.shift, tab.fs, tab.dftlen, cap)
    call('ptts_pulse_walk', *args, float(f0_cap), ptr(tab.t), ptr(info), stream(), tag=(B, total, cap))
    call('ptts_pulse_rows', *args, ptr(tab.t), ptr(info), ptr(tab.pulse_off_dev), ptr(irel), ptr(ioff), ptr(dbl), stream(),
         tag=(B, cap))
    info = info.cpu().numpy()
    for b in range(B):
        for bit, text in _PULSE_STATUS:
            if (info[b, 2] | info[b, 3]) & bit:
                raise ValueError('ops.{}: utterance {}: {}'.format(fn, b, text.format(maxwin=info[b, 1], dftlen=dftlen, cap=cap,
                                                                                      f0_cap=f0_cap)))
    tab.counts = info[:, 0].astype(np.int64)
    tab.pulse_off = np.concatenate([[0], np.cumsum(tab.counts)])
    tab.P, tab.W = int(tab.pulse_off[-1]), int(info[:, 1].max())
    P = tab.P
    tab.itab, tab.itab_packed, tab.dtab = irel[:ni * P].view(ni, P), ioff[:ni * P].view(ni, P), dbl[:nd * P].view(nd, P)
    return tab


def _segments_synthesis_batch(fn, segments, world, spec, rows, rows_name, table, noise, fs, dftlen):
    """ops.pulse_synthesis_batch and ops.world_synthesis_batch: the argument checks of _segments_synthesis, the kernel `segments`
    once over all pulses of the batch on the packed rows, then the overlap-add over the packed waveform."""
    pulse_check(dftlen, fs)
    K = dftlen // 2 + 1
    if not isinstance(table, PulseTableDevice) or table.world != world:
        raise ValueError('ops.{}: table is what ops.pulse_table_device returns {} voiced'.format(fn, 'with' if world else 'without'))
    if table.dftlen != int(dftlen) or table.fs != float(fs):
        raise ValueError('ops.{}: the table was built for fs={} dftlen={}'.format(fn, table.fs, table.dftlen))
    T, total, B = int(table.frame_off[-1]), int(table.sample_off[-1]), len(table.lengths)
    if not torch.is_tensor(spec) or tuple(spec.shape) != (T, K):
        raise ValueError('ops.{}: spec is not [sum T={},{}]'.format(fn, T, K))
    if not torch.is_tensor(rows) or tuple(rows.shape) != (T, K):
        raise ValueError('ops.{}: {} is not [{},{}]'.format(fn, rows_name, T, K))
    if torch.is_tensor(noise):
        if tuple(noise.shape) != (total,):
            raise ValueError('ops.{}: noise is not [sum wavlen={}]'.format(fn, total))
        pieces = [noise]
    else:
        pieces = list(noise)
        if len(pieces) != B or any(not torch.is_tensor(g) or tuple(g.shape) != (n,) for g, n in zip(pieces, table.wavlens)):
            raise ValueError('ops.{}: noise is not one [wavlen] tensor per utterance, wavlen = {}'.format(fn, table.wavlens))
    _no_backward(fn, spec, rows, *pieces)
    f32c(spec, '{}.spec'.format(fn)); f32c(rows, '{}.{}'.format(fn, rows_name))
    for g in pieces:
        f32c(g, '{}.noise'.format(fn))
    wav = torch.empty(total, dtype=torch.float32, device=spec.device)
    if total > 0:
        noise = pieces[0] if len(pieces) == 1 else torch.cat(pieces)
        P, W = table.P, table.W
        seg = torch.empty((P, W), dtype=torch.float32, device=spec.device)
        call(segments, ptr(spec), ptr(rows), ptr(noise), ptr(table.itab_packed), ptr(table.dtab), P, T, int(dftlen), float(fs), total,
             ptr(seg), W, stream(), tag=(P, dftlen, W))
        call('ptts_pulse_overlap_add_batch', ptr(seg), ptr(table.itab_packed), ptr(table.pulse_off_dev), ptr(table.offs[1]), B, P, W,
             ptr(wav), total, stream(), tag=(B, P, W, total))
    return list(wav.split(table.wavlens))


def pulse_synthesis_batch(spec, mask, table, noise, fs, dftlen):
    """ops.pulse_synthesis of a batch of utterances in one launch per kernel: spec and mask [sum T, dftlen/2+1] fp32 device, the
    utterances' rows one after the other, table from ops.pulse_table_device(f0, lengths, ...), noise a list of [wavlen_b] N(0,1)
    fp32 device tensors or one packed [sum wavlen] tensor.  Returns the list of [wavlen_b] fp32 device waveforms (views of one
    buffer), each byte for byte what ops.pulse_synthesis gives for that utterance alone; an utterance of one frame yields an empty
    tensor and no pulse work."""
    return _segments_synthesis_batch('pulse_synthesis_batch', 'ptts_pulse_segments', False, spec, mask, 'mask', table, noise, fs, dftlen)


def world_synthesis_batch(spec, aper, table, noise, fs, dftlen):
    """ops.world_synthesis of a batch of utterances in one launch per kernel: as ops.pulse_synthesis_batch, with aper
    (ops.aper_rows of the packed rows) and a table from ops.pulse_table_device(..., voiced=...)."""
    return _segments_synthesis_batch('world_synthesis_batch', 'ptts_world_segments', True, spec, aper, 'aper', table, noise, fs, dftlen)


# ----------------------------------------------------------------------------------------------
# waveform analysis for the PML parameters (the first half of run.py:146-153 features_extraction): csrc/analysis.hip
# ----------------------------------------------------------------------------------------------
COMPRESS_MEAN, COMPRESS_LSQ = 0, 1                      # PTTS_COMPRESS_MEAN / PTTS_COMPRESS_LSQ
ANALYSIS_NOISY_BELOW = math.exp(-0.75 ** 2 / 2)         # a harmonic is noisy where its phase coherence R lies below this
_COMPRESS_MODES = {'mean': COMPRESS_MEAN, 'lsq': COMPRESS_LSQ}
_band_weight_sums = {}      # (nb, fs, dftlen) -> the smallest sum_k W[k,b], on the host


def analysis_check(dftlen, fs, shift, f0_min, f0_max):
    """ValueError for parameters the analysis kernels do not take: dftlen / fs as pulse_check, a positive
    shift, 0 < f0_min <= f0_max <= fs/6 (every frame has two harmonics) and a window at f0_min, 2 int(1.5 fs / f0_min) + 1 samples,
    that fits dftlen.  Returns Hcap = floor((fs/2 - f0_min/2) / f0_min) - 1, the phasor columns of a frame.  Touches no device."""
    pulse_check(dftlen, fs)
    if not 0.0 < float(shift) < 1e3:
        raise ValueError('shift={} has to be positive'.format(shift))
    fs, f0_min, f0_max = float(fs), float(f0_min), float(f0_max)
    if not 0.0 < f0_min <= f0_max:
        raise ValueError('f0_min={} and f0_max={} have to be positive and ordered'.format(f0_min, f0_max))
    if f0_max > fs / 6.0:
        raise ValueError('f0_max={} above fs/6 = {}: a frame needs two harmonics'.format(f0_max, fs / 6.0))
    if 2 * int(1.5 * fs / f0_min) + 1 > dftlen:
        raise ValueError('the window at f0_min={} ({} samples) does not fit dftlen={}'.format(
            f0_min, 2 * int(1.5 * fs / f0_min) + 1, dftlen))
    return int(math.floor((0.5 * fs - 0.5 * f0_min) / f0_min)) - 1


def f0_track(f0, f0_min, f0_max, fs, shift, dftlen, wavlen=None):
    """The host step of the analysis: f0 [T] in Hz, one value per frame at shift * i, values <= 0 unvoiced ->
    float32 [T']: unvoiced stretches interpolated linearly between their voiced neighbours (the end values held), clipped to
    [f0_min, f0_max] (a float32 never rounds out of the interval).  With `wavlen` the frames whose centre rnd(shift i fs) lies beyond
    wavlen are cropped and a printed line says so.  ValueError: analysis_check, an empty or non-finite track, no voiced frame."""
    analysis_check(dftlen, fs, shift, f0_min, f0_max)
    f0 = np.asarray(f0, dtype=np.float64)
    if f0.ndim != 1 or f0.size < 1 or not np.isfinite(f0).all():
        raise ValueError('ops.f0_track: f0 has to be [T] finite Hz values, T >= 1')
    voiced = f0 > 0
    if not voiced.any():
        raise ValueError('ops.f0_track: no voiced frame')
    idx = np.arange(f0.size)
    track = np.clip(np.interp(idx, idx[voiced], f0[voiced]), float(f0_min), float(f0_max))
    out = track.astype(np.float32)
    low, high = out.astype(np.float64) < float(f0_min), out.astype(np.float64) > float(f0_max)
    out[low] = np.nextafter(out[low], np.float32(np.inf))
    out[high] = np.nextafter(out[high], np.float32(-np.inf))
    if wavlen is not None:
        keep = sum(1 for i in range(out.size) if _rnd(i * float(shift) * float(fs)) <= int(wavlen))
        if keep < out.size:
            print('    f0_track: {} of {} frames lie beyond the {} samples of the waveform and are cropped'.format(
                out.size - keep, out.size, int(wavlen)))
            out = out[:keep]
    return out


def _compress_table(device, nb, fs, dftlen):
    fw, fwbytes = _fwbnd_table(device, nb, fs, bark_alpha(fs), dftlen)
    return _device_table('fwbnd_compress', device, (nb, float(fs), dftlen), torch.float64, (nb,),
                         args=(ptr(fw), fwbytes, nb, int(dftlen)))


def fwbnd_compress_check(nb, fs, dftlen):
    """ValueError for a band axis the compression cannot invert: with W[k,b] the weight with which fwbnd2spec reads band b at bin
    k fs / dftlen, every band needs sum_k W[k,b] >= 1 (nb is too large for dftlen otherwise).  Host arithmetic, no device."""
    if not 0.0 < float(fs) < 1e9:
        raise ValueError('fs={} has to be positive'.format(fs))
    spectrum_check(dftlen, bark_alpha(fs), 1.4)
    if int(nb) != nb or not 2 <= nb <= SPECTRUM_MAX_NB:
        raise ValueError('nb={} outside [2, {}]'.format(nb, SPECTRUM_MAX_NB))
    key = (int(nb), float(fs), int(dftlen))
    if key not in _band_weight_sums:
        K = dftlen // 2 + 1
        melmax = 1127.0 * math.log(1.0 + 0.5 * float(fs) / 700.0)
        fb = 700.0 * (np.exp(np.arange(nb) * melmax / ((nb - 1) * 1127.0)) - 1.0)
        f = np.arange(K) * float(fs) / dftlen
        b = np.clip(np.searchsorted(fb, f, side='right') - 1, 0, nb - 2)
        fr = np.clip((f - fb[b]) / (fb[b + 1] - fb[b]), 0.0, 1.0)
        _band_weight_sums[key] = float((np.bincount(b, 1.0 - fr, nb) + np.bincount(b + 1, fr, nb)).min())
    if _band_weight_sums[key] < 1.0:
        raise ValueError('nb={} bands are too many for dftlen={} at fs={}: a band weighs {:.3f} bins, below 1'.format(
            nb, dftlen, fs, _band_weight_sums[key]))


def frame_harmonics(wav, f0, shift, fs, dftlen, hcap, log=False):
    """wav [N] and f0 [T] (fp32 device; Hz, as ops.f0_track returns them, frame i at shift * i) -> (SPEC [T, dftlen/2+1], the
    harmonic amplitude envelope, `log`: its logarithm; u [T, hcap, 2], the unit phasors of the phase distortion between neighbouring
    harmonics), one workgroup per frame (csrc/analysis.hip).  hcap: what ops.analysis_check returns for the
    f0_min of the track; a frame below that f0_min, or whose window does not fit dftlen, is left unwritten."""
    pulse_check(dftlen, fs)
    if not 0.0 < float(shift) < 1e3:
        raise ValueError('shift={} has to be positive'.format(shift))
    if not torch.is_tensor(wav) or wav.dim() != 1 or wav.numel() >= 1 << 40:
        raise ValueError('ops.frame_harmonics: wav is not [N]')
    if not torch.is_tensor(f0) or f0.dim() != 1 or f0.numel() >= 1 << 31:
        raise ValueError('ops.frame_harmonics: f0 is not [T]')
    if int(hcap) != hcap or not 1 <= hcap <= dftlen:
        raise ValueError('ops.frame_harmonics: hcap={} outside [1, {}]'.format(hcap, dftlen))
    _no_backward('frame_harmonics', wav, f0)
    f32c(wav, 'frame_harmonics.wav'); f32c(f0, 'frame_harmonics.f0')
    T, K = f0.numel(), dftlen // 2 + 1
    spec = torch.empty((T, K), dtype=torch.float32, device=f0.device)
    u = torch.empty((T, int(hcap), 2), dtype=torch.float32, device=f0.device)
    if T == 0:
        return spec, u
    call('ptts_frame_harmonics', ptr(wav) if wav.numel() else None, wav.numel(), ptr(f0), ptr(spec), ptr(u), T, int(hcap), float(shift),
         float(fs), int(dftlen), int(bool(log)), stream(), tag=(T, dftlen, int(hcap)))
    return spec, u


def phase_coherence(u, f0, shift, fs, dftlen, nb):
    """u [T, hcap, 2] from ops.frame_harmonics and f0 [T] (fp32 device) -> (R [T, hcap], the length of the mean phasor over the
    frames within max(2, rnd(1 / (f0 shift))) of each frame, 1 behind a frame's harmonics; NM [T, nb], the hat-weighted share of
    noisy bins (R < ANALYSIS_NOISY_BELOW) per band of the fwbnd2spec axis) (csrc/analysis.hip)."""
    pulse_check(dftlen, fs)
    if not 0.0 < float(shift) < 1e3:
        raise ValueError('shift={} has to be positive'.format(shift))
    if not torch.is_tensor(u) or u.dim() != 3 or u.shape[2] != 2 or not 1 <= u.shape[1] <= dftlen:
        raise ValueError('ops.phase_coherence: u is not [T, hcap, 2]')
    T, hcap = u.shape[0], u.shape[1]
    if not torch.is_tensor(f0) or tuple(f0.shape) != (T,):
        raise ValueError('ops.phase_coherence: f0 is not [{}]'.format(T))
    fwbnd_compress_check(nb, fs, dftlen)
    _no_backward('phase_coherence', u, f0)
    f32c(u, 'phase_coherence.u'); f32c(f0, 'phase_coherence.f0')
    R = torch.empty((T, hcap), dtype=torch.float32, device=u.device)
    nm = torch.empty((T, int(nb)), dtype=torch.float32, device=u.device)
    if T == 0:
        return R, nm
    fw, fwbytes = _fwbnd_table(u.device, int(nb), fs, bark_alpha(fs), dftlen)
    ct, ctbytes = _compress_table(u.device, int(nb), fs, dftlen)
    call('ptts_phase_coherence', ptr(u), ptr(f0), ptr(R), ptr(nm), T, hcap, int(nb), float(shift), float(fs), int(dftlen), ptr(fw),
         fwbytes, ptr(ct), ctbytes, stream(), tag=(T, hcap, int(nb)))
    return R, nm


def fwbnd_compress(x, fs, nb, mode='lsq', log=False):
    """x [T,K] or [B,T,K] fp32 device, K = dftlen/2 + 1 bins -> [.., nb] on the band axis of fwbnd2spec (csrc/analysis.hip).
    mode 'mean': the hat-weighted mean of x in each band.  mode 'lsq': the band values whose fwbnd2spec(log=True) is closest in least
    squares to ln|x| (`log`: to x, which is a logarithm already); fwbnd_compress(fwbnd2spec(y)) = y up to rounding."""
    if mode not in _COMPRESS_MODES:
        raise ValueError("ops.fwbnd_compress: mode is 'mean' or 'lsq', got {!r}".format(mode))
    if not torch.is_tensor(x) or x.dim() not in (2, 3) or x.shape[-1] < 5:
        raise ValueError('ops.fwbnd_compress: expected a [T,K] or [B,T,K] tensor')
    dftlen = 2 * (x.shape[-1] - 1)
    fwbnd_compress_check(nb, fs, dftlen)
    x, T, K = _spectrum_rows(x, 'fwbnd_compress', 5, SPECTRUM_MAX_DFTLEN // 2 + 1, 'K')
    out = torch.empty(tuple(x.shape[:-1]) + (int(nb),), dtype=torch.float32, device=x.device)
    if T == 0:
        return out
    fw, fwbytes = _fwbnd_table(x.device, int(nb), fs, bark_alpha(fs), dftlen)
    ct, ctbytes = _compress_table(x.device, int(nb), fs, dftlen)
    call('ptts_fwbnd_compress', ptr(x), ptr(out), T, int(nb), dftlen, _COMPRESS_MODES[mode], int(bool(log)), ptr(fw), fwbytes, ptr(ct),
         ctbytes, stream(), tag=(T, int(nb), dftlen))
    return out


# ----------------------------------------------------------------------------------------------
# waveform analysis for the WORLD parameters (the step behind vocoders.py:234-284, which calls pyworld; the definition is the
# build's own): csrc/worldanalysis.hip
# ----------------------------------------------------------------------------------------------
def world_analysis_check(dftlen, fs, shift, f0_min, f0_max):
    """ValueError for parameters the WORLD analysis kernels do not take: analysis_check's rules (dftlen / fs
    as pulse_check, a positive shift, 0 < f0_min <= f0_max <= fs/6, the window at f0_min, 2 int(1.5 fs / f0_min) + 1 samples, within
    dftlen) and the same window rule at WORLD_UNVOICED_RATE, the rate of an unvoiced frame, which has to lie below fs/2.  Touches
    no device."""
    analysis_check(dftlen, fs, shift, f0_min, f0_max)
    fs = float(fs)
    if not WORLD_UNVOICED_RATE < 0.5 * fs:
        raise ValueError('fs={}: the rate of an unvoiced frame, {} Hz, has to lie below fs/2'.format(fs, WORLD_UNVOICED_RATE))
    if 2 * int(1.5 * fs / WORLD_UNVOICED_RATE) + 1 > dftlen:
        raise ValueError('the window at the unvoiced rate {} Hz ({} samples) does not fit dftlen={}'.format(
            WORLD_UNVOICED_RATE, 2 * int(1.5 * fs / WORLD_UNVOICED_RATE) + 1, dftlen))


def _world_frames(fn, wav, shift, fs, dftlen, **rows):
    """The checks the two WORLD analysis ops share: wav [N] and the rows [T] (fp32 device, no backward) -> T."""
    pulse_check(dftlen, fs)
    if not 0.0 < float(shift) < 1e3:
        raise ValueError('shift={} has to be positive'.format(shift))
    if not torch.is_tensor(wav) or wav.dim() != 1 or wav.numel() >= 1 << 40:
        raise ValueError('ops.{}: wav is not [N]'.format(fn))
    T = None
    for name, t in rows.items():
        if not torch.is_tensor(t) or t.dim() != 1 or t.numel() >= 1 << 31 or (T is not None and t.numel() != T):
            raise ValueError('ops.{}: {} is not [{}]'.format(fn, name, 'T' if T is None else T))
        T = t.numel()
    _no_backward(fn, wav, *rows.values())
    f32c(wav, '{}.wav'.format(fn))
    for name, t in rows.items():
        f32c(t, '{}.{}'.format(fn, name))
    return T


def world_envelope(wav, rate, shift, fs, dftlen, log=False):
    """wav [N] and rate [T] (fp32 device; Hz: f0 in a voiced frame, WORLD_UNVOICED_RATE in an unvoiced one, frame i at shift * i)
    -> SPEC [T, dftlen/2+1], the amplitude envelope that world_synthesis reads (`log`: its logarithm), one workgroup per frame
    (csrc/worldanalysis.hip, DESIGN.md section 3, after CheapTrick): the power spectrum under a unit-energy Hann window of
    2 int(1.5 fs / rate) + 1 samples, mirrored below the rate, smoothed over 2/3 of the rate, scaled by fs / rate, and liftered so
    that the smoothing is undone at the harmonics.  A frame whose window does not fit dftlen is left unwritten."""
    T = _world_frames('world_envelope', wav, shift, fs, dftlen, rate=rate)
    spec = torch.empty((T, dftlen // 2 + 1), dtype=torch.float32, device=rate.device)
    if T == 0:
        return spec
    call('ptts_world_envelope', ptr(wav) if wav.numel() else None, wav.numel(), ptr(rate), ptr(spec), T, float(shift), float(fs),
         int(dftlen), int(bool(log)), stream(), tag=(T, dftlen))
    return spec


def world_aperiodicity(wav, f0, voiced, shift, fs, dftlen, nb):
    """wav [N], f0 [T] in Hz and voiced [T] (fp32 device; voiced >= 0.5 where the frame is voiced, a bool tensor is converted) ->
    the band aperiodicities [T, nb] in dB within [-60, 0], on the band axis of fwbnd2spec, one workgroup per frame
    (csrc/worldanalysis.hip): the energy of the difference of two windows one period apart over their mean
    energy, per band, from the bins at and above f0.  The row of an unvoiced frame is 0 dB.  The build's own estimator in the place
    of D4C."""
    if torch.is_tensor(voiced) and voiced.dtype == torch.bool:
        voiced = voiced.to(torch.float32)
    T = _world_frames('world_aperiodicity', wav, shift, fs, dftlen, f0=f0, voiced=voiced)
    fwbnd_compress_check(nb, fs, dftlen)
    aper = torch.empty((T, int(nb)), dtype=torch.float32, device=f0.device)
    if T == 0:
        return aper
    fw, fwbytes = _fwbnd_table(f0.device, int(nb), fs, bark_alpha(fs), dftlen)
    call('ptts_world_aperiodicity', ptr(wav) if wav.numel() else None, wav.numel(), ptr(f0), ptr(voiced), ptr(aper), T, int(nb),
         float(shift), float(fs), int(dftlen), ptr(fw), fwbytes, stream(), tag=(T, dftlen, int(nb)))
    return aper


# ----------------------------------------------------------------------------------------------
# F0 estimation (the pitch tracker the reference runs in front of run.py:146-153 features_extraction): csrc/f0.hip
# ----------------------------------------------------------------------------------------------
F0_MIN_NCAND, F0_MAX_NCAND = 2, 16
F0_MAX_FRAMES = 32768               # frames of one ptts_f0_viterbi launch (its back-pointers live in LDS); half of it above 8 slots
F0_CONSTANTS = {'voicing_threshold': 0.45, 'silence_threshold': 0.03, 'octave_cost': 0.01, 'octave_jump_cost': 0.35,
                'voiced_unvoiced_cost': 0.14}
_f0_window_tables = {}      # (fs, f0_min) -> rw on the host


def f0_check(dftlen, fs, shift, f0_min, f0_max):
    """ValueError for parameters the F0 kernels do not take: analysis_check, and the window at f0_min,
    W = 2 int(1.5 fs / f0_min) + 1 samples, with its longest lag lmax = floor(fs / f0_min) has to fit: W + lmax + 1 <= dftlen.
    Returns (hw, lmin, lmax) = (int(1.5 fs / f0_min), ceil(fs / f0_max), floor(fs / f0_min)).  Touches no device."""
    analysis_check(dftlen, fs, shift, f0_min, f0_max)
    fs, f0_min, f0_max = float(fs), float(f0_min), float(f0_max)
    hw, lmin, lmax = int(1.5 * fs / f0_min), int(math.ceil(fs / f0_max)), int(math.floor(fs / f0_min))
    if 2 * hw + 1 + lmax + 1 > dftlen:
        raise ValueError('the window at f0_min={} ({} samples) and its longest lag ({}) do not fit dftlen={}'.format(
            f0_min, 2 * hw + 1, lmax, dftlen))
    return hw, lmin, lmax


def f0_frame_count(wavlen, shift, fs):
    """The number of frames i >= 0 whose centre rnd(i shift fs) is at most wavlen: the cropping rule of f0_track."""
    wavlen, step = int(wavlen), float(shift) * float(fs)
    if wavlen < 0 or not 0.0 < float(shift) < 1e3 or not 0.0 < float(fs) < 1e9:
        raise ValueError('ops.f0_frame_count: wavlen={} shift={} fs={}'.format(wavlen, shift, fs))
    T = int(wavlen / step) + 2
    while T > 0 and _rnd((T - 1) * float(shift) * float(fs)) > wavlen:
        T -= 1
    while _rnd(T * float(shift) * float(fs)) <= wavlen:
        T += 1
    return T


def f0_window_table(fs, f0_min, f0_max, device=None):
    """rw [lmax + 2] fp64, the normalised autocorrelation sum_j w[j] w[j+k] / sum_j w[j]^2 of the F0 window
    w[j] = 0.5 - 0.5 cos(2 pi (j + 1) / (W + 1)), built on the host once per (fs, f0_min) and kept: a numpy array, or with `device`
    the device tensor ptts_f0_candidates reads."""
    fs, f0_min, f0_max = float(fs), float(f0_min), float(f0_max)
    if not (0.0 < fs < 1e9 and 0.0 < f0_min <= f0_max <= fs / 2.0) or 1.5 * fs / f0_min > SPECTRUM_MAX_DFTLEN:
        raise ValueError('ops.f0_window_table: fs={} f0_min={} f0_max={}'.format(fs, f0_min, f0_max))
    key = (fs, f0_min)
    if key not in _f0_window_tables:
        W, lmax = 2 * int(1.5 * fs / f0_min) + 1, int(math.floor(fs / f0_min))
        w = 0.5 - 0.5 * np.cos(2.0 * np.pi * (np.arange(W) + 1.0) / (W + 1.0))
        rw = np.array([np.dot(w[:W - k], w[k:]) for k in range(lmax + 2)]) / np.dot(w, w)
        rw.setflags(write=False)
        _f0_window_tables[key] = rw
    if device is None:
        return _f0_window_tables[key]
    dkey = ('f0window', device, fs, f0_min)
    if dkey not in _spectrum_tables:
        _spectrum_tables[dkey] = torch.from_numpy(_f0_window_tables[key].copy()).to(device)
    return _spectrum_tables[dkey]


def _f0_number(fn, name, value, lo, hi, open_lo=True):
    v = float(value)
    if not ((lo < v if open_lo else lo <= v) and v < hi):
        raise ValueError('ops.{}: {}={} outside {}{}, {})'.format(fn, name, value, '(' if open_lo else '[', lo, hi))
    return v


def _f0_ncand(fn, ncand):
    if int(ncand) != ncand or not F0_MIN_NCAND <= ncand <= F0_MAX_NCAND:
        raise ValueError('ops.{}: ncand={} outside [{}, {}]'.format(fn, ncand, F0_MIN_NCAND, F0_MAX_NCAND))
    return int(ncand)


def f0_candidates(wav, T, shift, fs, dftlen, f0_min, f0_max, gpeak, ncand=8, voicing_threshold=F0_CONSTANTS['voicing_threshold'],
                  silence_threshold=F0_CONSTANTS['silence_threshold'], octave_cost=F0_CONSTANTS['octave_cost'], want_r=False):
    """wav [N] (fp32 device) -> the pitch candidates of T frames, frame i centred at rnd(i shift fs), one workgroup per frame
    (csrc/f0.hip): (freq [T, ncand] Hz, strength [T, ncand], n [T] int32, lag [T, ncand] int32), with `want_r`
    also r [T, lmax + 2], the frame's normalised autocorrelation.  Slot 0 is the unvoiced candidate, slots 1 .. n_i the strongest
    peaks of r within [f0_min, f0_max], strongest first; gpeak: max |wav - mean(wav)| of the whole waveform, measured by the caller
    in fp64."""
    _, _, lmax = f0_check(dftlen, fs, shift, f0_min, f0_max)
    ncand = _f0_ncand('f0_candidates', ncand)
    if not torch.is_tensor(wav) or wav.dim() != 1 or wav.numel() >= 1 << 40:
        raise ValueError('ops.f0_candidates: wav is not [N]')
    if int(T) != T or not 0 <= T < 1 << 31 or T * (lmax + 2) >= 1 << 40:
        raise ValueError('ops.f0_candidates: T={} frames'.format(T))
    gpeak = _f0_number('f0_candidates', 'gpeak', gpeak, 0.0, float('inf'), open_lo=False)
    vt = _f0_number('f0_candidates', 'voicing_threshold', voicing_threshold, 0.0, 1e3)
    st = _f0_number('f0_candidates', 'silence_threshold', silence_threshold, 0.0, 1e3)
    oc = _f0_number('f0_candidates', 'octave_cost', octave_cost, 0.0, 1e3, open_lo=False)
    _no_backward('f0_candidates', wav)
    f32c(wav, 'f0_candidates.wav')
    T, dev = int(T), wav.device
    freq = torch.empty((T, ncand), dtype=torch.float32, device=dev)
    strength = torch.empty((T, ncand), dtype=torch.float32, device=dev)
    n = torch.empty(T, dtype=torch.int32, device=dev)
    lag = torch.empty((T, ncand), dtype=torch.int32, device=dev)
    r = torch.empty((T, lmax + 2), dtype=torch.float32, device=dev) if want_r else None
    if T > 0:
        rw = f0_window_table(fs, f0_min, f0_max, device=dev)
        call('ptts_f0_candidates', ptr(wav) if wav.numel() else None, wav.numel(), ptr(rw), rw.numel() * 8, ptr(freq), ptr(strength),
             ptr(n), ptr(lag), ptr(r), T, ncand, float(shift), float(fs), int(dftlen), float(f0_min), float(f0_max), gpeak, vt, st, oc,
             stream(), tag=(T, int(dftlen), ncand))
    return (freq, strength, n, lag, r) if want_r else (freq, strength, n, lag)


def f0_viterbi(freq, strength, n, shift, octave_jump_cost=F0_CONSTANTS['octave_jump_cost'],
               voiced_unvoiced_cost=F0_CONSTANTS['voiced_unvoiced_cost'], want_path=False):
    """The candidate tables of ops.f0_candidates (freq, strength [T, ncand] fp32, n [T] int32, device) -> f0 [T] fp32 device, the
    frequencies along the cheapest path through the slots, 0 where it takes the unvoiced slot 0 (csrc/f0.hip, DESIGN.md section 3;
    one wave for the utterance); with `want_path` also the slots [T] int32.  T is at most F0_MAX_FRAMES (half of it above 8 slots):
    the back-pointers live in LDS."""
    if not torch.is_tensor(freq) or freq.dim() != 2:
        raise ValueError('ops.f0_viterbi: freq is not [T, ncand]')
    T, ncand = freq.shape[0], _f0_ncand('f0_viterbi', freq.shape[1])
    if not torch.is_tensor(strength) or tuple(strength.shape) != (T, ncand):
        raise ValueError('ops.f0_viterbi: strength is not [{},{}]'.format(T, ncand))
    if not torch.is_tensor(n) or tuple(n.shape) != (T,):
        raise ValueError('ops.f0_viterbi: n is not [{}]'.format(T))
    cap = F0_MAX_FRAMES if ncand <= 8 else F0_MAX_FRAMES // 2
    if T > cap:
        raise ValueError('ops.f0_viterbi: {} frames, one launch takes at most {} with ncand={}'.format(T, cap, ncand))
    if not 0.0 < float(shift) < 1e3:
        raise ValueError('shift={} has to be positive'.format(shift))
    ojc = _f0_number('f0_viterbi', 'octave_jump_cost', octave_jump_cost, 0.0, 1e3, open_lo=False)
    vuc = _f0_number('f0_viterbi', 'voiced_unvoiced_cost', voiced_unvoiced_cost, 0.0, 1e3, open_lo=False)
    _no_backward('f0_viterbi', freq, strength)
    f32c(freq, 'f0_viterbi.freq'); f32c(strength, 'f0_viterbi.strength')
    _dev_tensor(n, torch.int32, 'f0_viterbi.n')
    f0 = torch.empty(T, dtype=torch.float32, device=freq.device)
    path = torch.empty(T, dtype=torch.int32, device=freq.device) if want_path else None
    if T > 0:
        call('ptts_f0_viterbi', ptr(freq), ptr(strength), ptr(n), ptr(f0), ptr(path), T, ncand, float(shift), ojc, vuc, stream(),
             tag=(T, ncand))
    return (f0, path) if want_path else f0


def f0_estimate(wav, shift, fs, dftlen, f0_min, f0_max, ncand=8, **constants):
    """A mono waveform at fs (any float array, or an fp32 device tensor) -> f0 [T] in Hz, numpy float32, one value per frame at
    shift * i, 0 where unvoiced: what ops.f0_track and the .f0 files mean.  T = f0_frame_count(len(wav), shift, fs).  The build's
    own estimator (after Boersma 1993): ops.f0_candidates, then ops.f0_viterbi; `constants`: any of
    F0_CONSTANTS."""
    if set(constants) - set(F0_CONSTANTS):
        raise ValueError('ops.f0_estimate: unknown arguments {}'.format(sorted(set(constants) - set(F0_CONSTANTS))))
    f0_check(dftlen, fs, shift, f0_min, f0_max)
    ncand = _f0_ncand('f0_estimate', ncand)
    if torch.is_tensor(wav):
        if wav.dim() != 1:
            raise ValueError('ops.f0_estimate: wav is not [N]')
        _no_backward('f0_estimate', wav)
        N = wav.numel()
    else:
        wav = np.asarray(wav, dtype=np.float64)
        if wav.ndim != 1 or not np.isfinite(wav).all():
            raise ValueError('ops.f0_estimate: wav is not a finite [N] waveform')
        N = wav.size
    T = f0_frame_count(N, shift, fs)
    cap = F0_MAX_FRAMES if ncand <= 8 else F0_MAX_FRAMES // 2
    if T > cap:
        raise ValueError('ops.f0_estimate: {} frames, one utterance takes at most {} with ncand={}'.format(T, cap, ncand))
    if not torch.is_tensor(wav):
        from . import backend_hip
        wav = torch.from_numpy(wav.astype(np.float32)).to(backend_hip.device())
    f32c(wav, 'f0_estimate.wav')
    x = wav.to(torch.float64)                                   # gpeak in fp64 from the fp32 samples the kernel reads
    gpeak = float((x - x.mean()).abs().max().item()) if N else 0.0
    if not math.isfinite(gpeak):
        raise ValueError('ops.f0_estimate: wav is not finite')
    cand = {k: constants[k] for k in ('voicing_threshold', 'silence_threshold', 'octave_cost') if k in constants}
    path = {k: constants[k] for k in ('octave_jump_cost', 'voiced_unvoiced_cost') if k in constants}
    freq, strength, n, _ = f0_candidates(wav, T, shift, fs, dftlen, f0_min, f0_max, gpeak, ncand=ncand, **cand)
    return f0_viterbi(freq, strength, n, shift, **path).cpu().numpy()


F0_REFINE_MAX_WINDOW = 16384        # samples of the refinement's window at f0_min, 2 rnd(1.5 fs / f0_min) + 1


def f0_refine_check(fs, shift, f0_min, f0_max):
    """ValueError for parameters ptts_f0_refine does not take: a positive shift and fs,
    0 < f0_min <= f0_max <= fs/2 and a window at f0_min, 2 rnd(1.5 fs / f0_min) + 1 samples, of at most F0_REFINE_MAX_WINDOW.
    Returns that window length.  Touches no device."""
    fs, shift, f0_min, f0_max = float(fs), float(shift), float(f0_min), float(f0_max)
    if not 0.0 < shift < 1e3:
        raise ValueError('shift={} has to be positive'.format(shift))
    if not 0.0 < fs < 1e9:
        raise ValueError('fs={} has to be positive'.format(fs))
    if not 0.0 < f0_min <= f0_max <= 0.5 * fs:
        raise ValueError('f0_min={} and f0_max={} have to be positive, ordered and at most fs/2 = {}'.format(f0_min, f0_max, 0.5 * fs))
    W = 2.0 * math.floor(1.5 * fs / f0_min + 0.5) + 1.0
    if W > F0_REFINE_MAX_WINDOW:
        raise ValueError('the window at f0_min={} ({:.0f} samples) is longer than {}'.format(f0_min, W, F0_REFINE_MAX_WINDOW))
    return int(W)


def f0_refine(wav, f0, shift, fs, f0_min, f0_max, want_status=False):
    """A mono waveform at fs (any float array, or an fp32 device tensor) and an F0 track f0 [T] in Hz (an array or a tensor; frame i
    at shift * i, <= 0 or NaN: unvoiced) -> the track refined by the instantaneous frequency of its harmonics, numpy float32 [T]
    (ptts_f0_refine, csrc/f0.hip; after the published StoneMask, one workgroup per frame); with `want_status`
    also status [T] int32: 0 unvoiced (the value is 0), 1 refined, 2 left as it was (outside [f0_min, f0_max], or the window of
    2 rnd(1.5 fs / f0_i) + 1 samples leaves the waveform), 3 left as it was (no energy at the harmonics, or a result more than 20 %
    away or outside [f0_min, f0_max]).  The voicing pattern does not change."""
    f0_refine_check(fs, shift, f0_min, f0_max)
    if torch.is_tensor(wav):
        if wav.dim() != 1 or wav.numel() >= 1 << 40:
            raise ValueError('ops.f0_refine: wav is not [N]')
        _no_backward('f0_refine', wav)
    else:
        wav = np.asarray(wav, dtype=np.float64)
        if wav.ndim != 1 or not np.isfinite(wav).all():
            raise ValueError('ops.f0_refine: wav is not a finite [N] waveform')
    if torch.is_tensor(f0):
        _no_backward('f0_refine', f0)
        if f0.dim() != 1 or not (f0.is_floating_point() or f0.numel() == 0):
            raise ValueError('ops.f0_refine: f0 is not [T] Hz values')
    else:
        f0 = np.array(f0, dtype=np.float32)                     # a copy: the caller's array may be read-only
        if f0.ndim != 1:
            raise ValueError('ops.f0_refine: f0 is not [T] Hz values')
        f0 = torch.from_numpy(f0)
    T = f0.numel()
    if T >= 1 << 31:
        raise ValueError('ops.f0_refine: T={} frames'.format(T))
    if not torch.is_tensor(wav):
        from . import backend_hip
        wav = torch.from_numpy(wav.astype(np.float32)).to(backend_hip.device())
    f32c(wav, 'f0_refine.wav')
    f0 = f0.to(device=wav.device, dtype=torch.float32).contiguous()
    out = torch.empty(T, dtype=torch.float32, device=wav.device)
    status = torch.empty(T, dtype=torch.int32, device=wav.device) if want_status else None
    if T > 0:
        call('ptts_f0_refine', ptr(wav) if wav.numel() else None, wav.numel(), ptr(f0), ptr(out), ptr(status), T, float(shift),
             float(fs), float(f0_min), float(f0_max), stream(), tag=(T,))
    return (out.cpu().numpy(), status.cpu().numpy()) if want_status else out.cpu().numpy()


# ----------------------------------------------------------------------------------------------
# waveform analysis over a batch of utterances: csrc/analysisbatch.hip and the *_batch kernels of csrc/f0.hip, csrc/analysis.hip,
# csrc/worldanalysis.hip.  Device tensors in, device tensors out: nothing here reads a device value back unless it says so.
# ----------------------------------------------------------------------------------------------
ANALYSIS_MAX_UTTS = 65535           # utterances of one launch
# (status bit of include/percival_hip.h, what the ValueError says: the wording of the single-utterance path for the same condition)
_ANALYSIS_STATUS = tuple((_hip._define('PTTS_ANALYSIS_' + name), text) for name, text in (
    ('BAD_WAV', 'wav is not a finite [N] waveform'),
    ('BAD_F0', 'ops.f0_track: f0 has to be [T] finite Hz values, T >= 1'),
    ('NO_VOICED', 'ops.f0_track: no voiced frame')))


class PackedOffsets(object):
    """The layout of a packed batch along one axis: lengths (a list of ints), off (numpy int64 [B+1]), total, and dev, the offsets as
    an int64 device tensor (what the *_batch kernels read).  Made by ops.packed_offsets; every batched op takes one wherever it
    takes a list of lengths, so that a chain of ops uploads the offsets once."""

    def __init__(self, lengths, device):
        self.lengths = lengths
        self.off = np.concatenate([[0], np.cumsum(lengths, dtype=np.int64)]).astype(np.int64)
        self.total = int(self.off[-1])
        self.dev = torch.from_numpy(self.off).to(device)

    def __len__(self):
        return len(self.lengths)


def packed_offsets(lengths, device, fn='packed_offsets', what='lengths'):
    """A list of non-negative lengths (or a PackedOffsets, returned as it is) -> the PackedOffsets on `device`."""
    if isinstance(lengths, PackedOffsets):
        return lengths
    try:
        lengths = [int(n) for n in lengths]
    except (TypeError, ValueError):
        raise ValueError('ops.{}: {} has to be the utterances\' lengths'.format(fn, what))
    if not 1 <= len(lengths) <= ANALYSIS_MAX_UTTS or min(lengths) < 0:
        raise ValueError('ops.{}: {} has to hold 1 to {} lengths of at least 0'.format(fn, what, ANALYSIS_MAX_UTTS))
    if sum(lengths) >= 1 << 40:
        raise ValueError('ops.{}: {} sum to {}'.format(fn, what, sum(lengths)))
    return PackedOffsets(lengths, device)


def analysis_status(fn, info):
    """The one read-back of a batched analysis: info [B] int32 device, the PTTS_ANALYSIS_* bits of every utterance -> ValueError
    naming the first utterance that has one set."""
    info = info.cpu().numpy()
    for b in range(info.size):
        for bit, text in _ANALYSIS_STATUS:
            if info[b] & bit:
                raise ValueError('{}: utterance {}: {}'.format(fn, b, text))


def _batch_layout(fn, wav, wav_lengths, frame_lengths, **rows):
    """The checks the batched frame ops share: wav [sum N] or None, and the per-frame rows [sum T, ..] (fp32 device unless said
    otherwise, no backward) -> (wav layout or None, frame layout)."""
    first = next(t for t in list(rows.values()) + [wav] if t is not None)
    if not torch.is_tensor(first):
        raise ValueError('ops.{}: expected device tensors'.format(fn))
    fo = packed_offsets(frame_lengths, first.device, fn, 'frame_lengths')
    if fo.total >= 1 << 31:
        raise ValueError('ops.{}: {} frames'.format(fn, fo.total))
    wo = None
    if wav is not None:
        wo = packed_offsets(wav_lengths, first.device, fn, 'wav_lengths')
        if len(wo) != len(fo):
            raise ValueError('ops.{}: {} waveforms and {} frame counts'.format(fn, len(wo), len(fo)))
        if not torch.is_tensor(wav) or tuple(wav.shape) != (wo.total,):
            raise ValueError('ops.{}: wav is not [sum(wav_lengths)={}]'.format(fn, wo.total))
        f32c(wav, '{}.wav'.format(fn))
        _no_backward(fn, wav)
    for name, t in rows.items():
        if t is None:
            continue
        if not torch.is_tensor(t) or t.dim() < 1 or t.shape[0] != fo.total:
            raise ValueError('ops.{}: {} is not [sum(frame_lengths)={}, ..]'.format(fn, name, fo.total))
        _no_backward(fn, t)
    return wo, fo


def _wav_args(wav, wo):
    return ptr(wav) if wo.total else None, ptr(wo.dev), wo.total


def _info(info, B, device, fn):
    if info is None:
        return torch.zeros(B, dtype=torch.int32, device=device), True
    _dev_tensor(info, torch.int32, '{}.info'.format(fn), (B,))
    return info, False


def wave_peak(wav, wav_lengths, info=None):
    """wav [sum N] fp32 device, the utterances one after the other -> gpeak [B] fp64 device, max |x - mean(x)| of every utterance
    in fp64, what ops.f0_estimate measures for ptts_f0_candidates (csrc/analysisbatch.hip; one workgroup per utterance, a
    fixed-order sum: the same input gives the same bytes; 0 for an utterance without samples).  A sample that is not finite sets
    PTTS_ANALYSIS_BAD_WAV in `info` [B] int32 (zeroed by the caller, read by ops.analysis_status); without `info` the op reads the
    status back itself and raises the ValueError."""
    fn = 'wave_peak'
    if not torch.is_tensor(wav):
        raise ValueError('ops.{}: wav is not a packed device tensor'.format(fn))
    wo = packed_offsets(wav_lengths, wav.device, fn, 'wav_lengths')
    if tuple(wav.shape) != (wo.total,):
        raise ValueError('ops.{}: wav is not [sum(wav_lengths)={}]'.format(fn, wo.total))
    f32c(wav, fn + '.wav')
    _no_backward(fn, wav)
    B = len(wo)
    info, own = _info(info, B, wav.device, fn)
    gpeak = torch.empty(B, dtype=torch.float64, device=wav.device)
    call('ptts_wave_peak', *_wav_args(wav, wo), B, ptr(gpeak), ptr(info), stream(), tag=(B, wo.total))
    if own:
        analysis_status('ops.' + fn, info)
    return gpeak


def f0_track_lengths(fn, frame_lengths, wav_lengths, shift, fs):
    """T'_b = min(T_b, f0_frame_count(N_b, shift, fs)), f0_track's cropping rule, with its printed line per cropped utterance."""
    out = []
    for T, N in zip(frame_lengths, wav_lengths):
        keep = min(T, f0_frame_count(N, shift, fs))
        if keep < T:
            print('    f0_track: {} of {} frames lie beyond the {} samples of the waveform and are cropped'.format(T - keep, T, N))
        out.append(keep)
    return out


def f0_track_device(f0, frame_lengths, wav_lengths, f0_min, f0_max, fs, shift, dftlen, info=None):
    """ops.f0_track for every utterance of a batch, on the device (ptts_f0_track, csrc/analysisbatch.hip; one workgroup per
    utterance): f0 [sum T] fp32 or fp64 device in Hz (<= 0 unvoiced), the utterances one after the other, frame_lengths their T_b,
    wav_lengths their waveforms' N_b (lists, or PackedOffsets) -> (track [sum T'] fp32 device, bit for bit ops.f0_track(f0_b, ...,
    wavlen=N_b) of every utterance; vuv [sum T'] fp32, 1 where f0 > 0; the PackedOffsets of T'_b = min(T_b, f0_frame_count(N_b))).
    A cropped utterance prints f0_track's line.  What ops.f0_track refuses per utterance (no voiced frame, a value that is not
    finite) is a PTTS_ANALYSIS_* bit in `info` [B] int32, as in ops.wave_peak; such an utterance's rows are not written."""
    fn = 'f0_track_device'
    analysis_check(dftlen, fs, shift, f0_min, f0_max)
    _, fo = _batch_layout(fn, None, None, frame_lengths, f0=f0)
    if not (f0.is_cuda and f0.dtype in (torch.float32, torch.float64) and f0.is_contiguous() and f0.dim() == 1):
        raise _hip.HipLibraryError('{}.f0: expected a contiguous [sum T] float32 or float64 device tensor'.format(fn))
    wav_lengths = wav_lengths.lengths if isinstance(wav_lengths, PackedOffsets) else [int(n) for n in wav_lengths]
    if len(wav_lengths) != len(fo) or min(fo.lengths) < 1:
        raise ValueError('ops.{}: {} waveforms for {} tracks of at least one frame'.format(fn, len(wav_lengths), len(fo)))
    oo = packed_offsets(f0_track_lengths(fn, fo.lengths, wav_lengths, shift, fs), f0.device, fn)
    B = len(fo)
    info, own = _info(info, B, f0.device, fn)
    track = torch.zeros(oo.total, dtype=torch.float32, device=f0.device)         # zeros: the frame kernels skip a refused utterance's rows
    vuv = torch.zeros(oo.total, dtype=torch.float32, device=f0.device)
    call('ptts_f0_track', ptr(f0), int(f0.dtype == torch.float64), ptr(fo.dev), fo.total, ptr(oo.dev), oo.total, B,
         ptr(track) if oo.total else None, ptr(vuv) if oo.total else None, ptr(info), float(f0_min), float(f0_max), stream(),
         tag=(B, fo.total))
    if own:
        analysis_status('ops.' + fn, info)
    return track, vuv, oo


def f0_candidates_batch(wav, wav_lengths, frame_lengths, shift, fs, dftlen, f0_min, f0_max, gpeak, ncand=8,
                        voicing_threshold=F0_CONSTANTS['voicing_threshold'], silence_threshold=F0_CONSTANTS['silence_threshold'],
                        octave_cost=F0_CONSTANTS['octave_cost'], want_r=False):
    """ops.f0_candidates of a batch in one launch: wav [sum N] fp32 device, frame_lengths the T_b, gpeak [B] fp64 device (ops.wave_peak)
    -> (freq, strength [sum T, ncand], n [sum T], lag [sum T, ncand]) (and r [sum T, lmax + 2]), utterance b's rows bit for bit
    ops.f0_candidates(wav_b, T_b, ..., gpeak=gpeak[b])."""
    fn = 'f0_candidates_batch'
    _, _, lmax = f0_check(dftlen, fs, shift, f0_min, f0_max)
    ncand = _f0_ncand(fn, ncand)
    wo, fo = _batch_layout(fn, wav, wav_lengths, frame_lengths)
    vt = _f0_number(fn, 'voicing_threshold', voicing_threshold, 0.0, 1e3)
    st = _f0_number(fn, 'silence_threshold', silence_threshold, 0.0, 1e3)
    oc = _f0_number(fn, 'octave_cost', octave_cost, 0.0, 1e3, open_lo=False)
    _dev_tensor(gpeak, torch.float64, fn + '.gpeak', (len(wo),))
    T, dev = fo.total, wav.device
    freq = torch.empty((T, ncand), dtype=torch.float32, device=dev)
    strength = torch.empty((T, ncand), dtype=torch.float32, device=dev)
    n = torch.empty(T, dtype=torch.int32, device=dev)
    lag = torch.empty((T, ncand), dtype=torch.int32, device=dev)
    r = torch.empty((T, lmax + 2), dtype=torch.float32, device=dev) if want_r else None
    if T > 0:
        rw = f0_window_table(fs, f0_min, f0_max, device=dev)
        call('ptts_f0_candidates_batch', *_wav_args(wav, wo), ptr(fo.dev), len(fo), T, ptr(rw), rw.numel() * 8, ptr(freq), ptr(strength),
             ptr(n), ptr(lag), ptr(r), ncand, float(shift), float(fs), int(dftlen), float(f0_min), float(f0_max), ptr(gpeak), vt, st, oc,
             stream(), tag=(len(fo), T, int(dftlen), ncand))
    return (freq, strength, n, lag, r) if want_r else (freq, strength, n, lag)


def f0_viterbi_batch(freq, strength, n, frame_lengths, shift, octave_jump_cost=F0_CONSTANTS['octave_jump_cost'],
                     voiced_unvoiced_cost=F0_CONSTANTS['voiced_unvoiced_cost'], want_path=False):
    """ops.f0_viterbi of a batch in one launch, one wave per utterance: the packed tables of ops.f0_candidates_batch -> f0 [sum T]
    fp32 device (with `want_path` also the slots), utterance b's values bit for bit ops.f0_viterbi of its rows.  The frame cap
    F0_MAX_FRAMES (half of it above 8 slots) holds for each utterance, not for the batch."""
    fn = 'f0_viterbi_batch'
    if not torch.is_tensor(freq) or freq.dim() != 2:
        raise ValueError('ops.{}: freq is not [sum T, ncand]'.format(fn))
    ncand = _f0_ncand(fn, freq.shape[1])
    _, fo = _batch_layout(fn, None, None, frame_lengths, freq=freq, strength=strength, n=n)
    T = fo.total
    if tuple(strength.shape) != (T, ncand) or tuple(n.shape) != (T,):
        raise ValueError('ops.{}: strength is not [{},{}] or n is not [{}]'.format(fn, T, ncand, T))
    cap = F0_MAX_FRAMES if ncand <= 8 else F0_MAX_FRAMES // 2
    if max(fo.lengths) > cap:
        raise ValueError('ops.{}: {} frames, one utterance takes at most {} with ncand={}'.format(fn, max(fo.lengths), cap, ncand))
    if not 0.0 < float(shift) < 1e3:
        raise ValueError('shift={} has to be positive'.format(shift))
    ojc = _f0_number(fn, 'octave_jump_cost', octave_jump_cost, 0.0, 1e3, open_lo=False)
    vuc = _f0_number(fn, 'voiced_unvoiced_cost', voiced_unvoiced_cost, 0.0, 1e3, open_lo=False)
    f32c(freq, fn + '.freq'); f32c(strength, fn + '.strength')
    _dev_tensor(n, torch.int32, fn + '.n')
    f0 = torch.empty(T, dtype=torch.float32, device=freq.device)
    path = torch.empty(T, dtype=torch.int32, device=freq.device) if want_path else None
    if T > 0:
        call('ptts_f0_viterbi_batch', ptr(freq), ptr(strength), ptr(n), ptr(f0), ptr(path), ptr(fo.dev), len(fo), T, max(fo.lengths), ncand,
             float(shift), ojc, vuc, stream(), tag=(len(fo), T, ncand))
    return (f0, path) if want_path else f0


def f0_estimate_batch(wav, wav_lengths, shift, fs, dftlen, f0_min, f0_max, ncand=8, info=None, want_gpeak=False, **constants):
    """ops.f0_estimate of a batch without a read-back: wav [sum N] fp32 device -> (f0 [sum T] fp32 device, 0 where unvoiced, the
    PackedOffsets of T_b = f0_frame_count(N_b, shift, fs)) (with `want_gpeak` also gpeak [B] fp64 device): ops.wave_peak,
    ops.f0_candidates_batch, ops.f0_viterbi_batch, one launch each.  Utterance b's track is bit for bit ops.f0_candidates(wav_b,
    T_b, ..., gpeak=gpeak[b]) followed by ops.f0_viterbi; gpeak[b] and the torch value of ops.f0_estimate may differ in the last
    bit.  `info` as in ops.wave_peak."""
    fn = 'f0_estimate_batch'
    if set(constants) - set(F0_CONSTANTS):
        raise ValueError('ops.{}: unknown arguments {}'.format(fn, sorted(set(constants) - set(F0_CONSTANTS))))
    f0_check(dftlen, fs, shift, f0_min, f0_max)
    ncand = _f0_ncand(fn, ncand)
    if not torch.is_tensor(wav):
        raise ValueError('ops.{}: wav is not a packed device tensor'.format(fn))
    wo = packed_offsets(wav_lengths, wav.device, fn, 'wav_lengths')
    lengths = [f0_frame_count(N, shift, fs) for N in wo.lengths]
    cap = F0_MAX_FRAMES if ncand <= 8 else F0_MAX_FRAMES // 2
    if max(lengths) > cap:
        raise ValueError('ops.{}: {} frames, one utterance takes at most {} with ncand={}'.format(fn, max(lengths), cap, ncand))
    fo = packed_offsets(lengths, wav.device, fn)
    info, own = _info(info, len(wo), wav.device, fn)
    gpeak = wave_peak(wav, wo, info=info)
    cand = {k: constants[k] for k in ('voicing_threshold', 'silence_threshold', 'octave_cost') if k in constants}
    path = {k: constants[k] for k in ('octave_jump_cost', 'voiced_unvoiced_cost') if k in constants}
    freq, strength, n, _ = f0_candidates_batch(wav, wo, fo, shift, fs, dftlen, f0_min, f0_max, gpeak, ncand=ncand, **cand)
    f0 = f0_viterbi_batch(freq, strength, n, fo, shift, **path)
    if own:
        analysis_status('ops.' + fn, info)
    return (f0, fo, gpeak) if want_gpeak else (f0, fo)


def f0_refine_batch(wav, wav_lengths, f0, frame_lengths, shift, fs, f0_min, f0_max, want_status=False):
    """ops.f0_refine of a batch in one launch: wav [sum N] and f0 [sum T] fp32 device -> the refined track [sum T] fp32 device (with
    `want_status` also status [sum T] int32), utterance b's values bit for bit ops.f0_refine(wav_b, f0_b, ...)."""
    fn = 'f0_refine_batch'
    f0_refine_check(fs, shift, f0_min, f0_max)
    wo, fo = _batch_layout(fn, wav, wav_lengths, frame_lengths, f0=f0)
    if f0.dim() != 1:
        raise ValueError('ops.{}: f0 is not [sum T]'.format(fn))
    f32c(f0, fn + '.f0')
    T = fo.total
    out = torch.empty(T, dtype=torch.float32, device=wav.device)
    status = torch.empty(T, dtype=torch.int32, device=wav.device) if want_status else None
    if T > 0:
        call('ptts_f0_refine_batch', *_wav_args(wav, wo), ptr(fo.dev), len(fo), T, ptr(f0), ptr(out), ptr(status), float(shift), float(fs),
             float(f0_min), float(f0_max), stream(), tag=(len(fo), T))
    return (out, status) if want_status else out


def frame_harmonics_batch(wav, wav_lengths, f0, frame_lengths, shift, fs, dftlen, hcap, log=False):
    """ops.frame_harmonics of a batch in one launch: wav [sum N], f0 [sum T] fp32 device -> (SPEC [sum T, dftlen/2+1], u [sum T, hcap,
    2]), utterance b's rows bit for bit ops.frame_harmonics(wav_b, f0_b, ...)."""
    fn = 'frame_harmonics_batch'
    pulse_check(dftlen, fs)
    if not 0.0 < float(shift) < 1e3:
        raise ValueError('shift={} has to be positive'.format(shift))
    if int(hcap) != hcap or not 1 <= hcap <= dftlen:
        raise ValueError('ops.{}: hcap={} outside [1, {}]'.format(fn, hcap, dftlen))
    wo, fo = _batch_layout(fn, wav, wav_lengths, frame_lengths, f0=f0)
    if f0.dim() != 1:
        raise ValueError('ops.{}: f0 is not [sum T]'.format(fn))
    f32c(f0, fn + '.f0')
    T, K = fo.total, dftlen // 2 + 1
    spec = torch.empty((T, K), dtype=torch.float32, device=f0.device)
    u = torch.empty((T, int(hcap), 2), dtype=torch.float32, device=f0.device)
    if T > 0:
        call('ptts_frame_harmonics_batch', *_wav_args(wav, wo), ptr(fo.dev), len(fo), T, ptr(f0), ptr(spec), ptr(u), int(hcap),
             float(shift), float(fs), int(dftlen), int(bool(log)), stream(), tag=(len(fo), T, dftlen, int(hcap)))
    return spec, u


def phase_coherence_batch(u, f0, frame_lengths, shift, fs, dftlen, nb):
    """ops.phase_coherence of a batch in one launch: u [sum T, hcap, 2] and f0 [sum T] fp32 device -> (R [sum T, hcap], NM [sum T,
    nb]), utterance b's rows bit for bit ops.phase_coherence(u_b, f0_b, ...): a frame's neighbourhood ends where its utterance
    ends."""
    fn = 'phase_coherence_batch'
    pulse_check(dftlen, fs)
    if not 0.0 < float(shift) < 1e3:
        raise ValueError('shift={} has to be positive'.format(shift))
    if not torch.is_tensor(u) or u.dim() != 3 or u.shape[2] != 2 or not 1 <= u.shape[1] <= dftlen:
        raise ValueError('ops.{}: u is not [sum T, hcap, 2]'.format(fn))
    _, fo = _batch_layout(fn, None, None, frame_lengths, u=u, f0=f0)
    T, hcap = fo.total, u.shape[1]
    if f0.dim() != 1:
        raise ValueError('ops.{}: f0 is not [{}]'.format(fn, T))
    fwbnd_compress_check(nb, fs, dftlen)
    f32c(u, fn + '.u'); f32c(f0, fn + '.f0')
    R = torch.empty((T, hcap), dtype=torch.float32, device=u.device)
    nm = torch.empty((T, int(nb)), dtype=torch.float32, device=u.device)
    if T > 0:
        fw, fwbytes = _fwbnd_table(u.device, int(nb), fs, bark_alpha(fs), dftlen)
        ct, ctbytes = _compress_table(u.device, int(nb), fs, dftlen)
        call('ptts_phase_coherence_batch', ptr(u), ptr(f0), ptr(R), ptr(nm), ptr(fo.dev), len(fo), T, hcap, int(nb), float(shift),
             float(fs), int(dftlen), ptr(fw), fwbytes, ptr(ct), ctbytes, stream(), tag=(len(fo), T, hcap, int(nb)))
    return R, nm


def _world_frames_batch(fn, wav, wav_lengths, frame_lengths, shift, fs, dftlen, **rows):
    pulse_check(dftlen, fs)
    if not 0.0 < float(shift) < 1e3:
        raise ValueError('shift={} has to be positive'.format(shift))
    wo, fo = _batch_layout(fn, wav, wav_lengths, frame_lengths, **rows)
    for name, t in rows.items():
        if t.dim() != 1:
            raise ValueError('ops.{}: {} is not [sum T]'.format(fn, name))
        f32c(t, '{}.{}'.format(fn, name))
    return wo, fo


def world_envelope_batch(wav, wav_lengths, rate, frame_lengths, shift, fs, dftlen, log=False):
    """ops.world_envelope of a batch in one launch: wav [sum N], rate [sum T] fp32 device -> SPEC [sum T, dftlen/2+1], utterance b's
    rows bit for bit ops.world_envelope(wav_b, rate_b, ...)."""
    fn = 'world_envelope_batch'
    wo, fo = _world_frames_batch(fn, wav, wav_lengths, frame_lengths, shift, fs, dftlen, rate=rate)
    T = fo.total
    spec = torch.empty((T, dftlen // 2 + 1), dtype=torch.float32, device=rate.device)
    if T > 0:
        call('ptts_world_envelope_batch', *_wav_args(wav, wo), ptr(fo.dev), len(fo), T, ptr(rate), ptr(spec), float(shift), float(fs),
             int(dftlen), int(bool(log)), stream(), tag=(len(fo), T, dftlen))
    return spec


def world_aperiodicity_batch(wav, wav_lengths, f0, voiced, frame_lengths, shift, fs, dftlen, nb):
    """ops.world_aperiodicity of a batch in one launch: wav [sum N], f0 and voiced [sum T] fp32 device (a bool `voiced` is
    converted) -> the band aperiodicities [sum T, nb] in dB, utterance b's rows bit for bit ops.world_aperiodicity(wav_b, ...)."""
    fn = 'world_aperiodicity_batch'
    if torch.is_tensor(voiced) and voiced.dtype == torch.bool:
        voiced = voiced.to(torch.float32)
    wo, fo = _world_frames_batch(fn, wav, wav_lengths, frame_lengths, shift, fs, dftlen, f0=f0, voiced=voiced)
    fwbnd_compress_check(nb, fs, dftlen)
    T = fo.total
    aper = torch.empty((T, int(nb)), dtype=torch.float32, device=f0.device)
    if T > 0:
        fw, fwbytes = _fwbnd_table(f0.device, int(nb), fs, bark_alpha(fs), dftlen)
        call('ptts_world_aperiodicity_batch', *_wav_args(wav, wo), ptr(fo.dev), len(fo), T, ptr(f0), ptr(voiced), ptr(aper), int(nb),
             float(shift), float(fs), int(dftlen), ptr(fw), fwbytes, stream(), tag=(len(fo), T, dftlen, int(nb)))
    return aper


# ----------------------------------------------------------------------------------------------
# DTW alignment of utterance pairs of unequal length (the build's own): csrc/dtw.hip
# ----------------------------------------------------------------------------------------------
DTW_WORKSPACE_CAP = 1 << 30         # bytes of workspace one ptts_dtw_align_batch call may use; a larger batch is split along B
_DTW_STATUS = tuple((_hip._define('PTTS_DTW_' + name), text) for name, text in (
    ('EMPTY', 'a side has no frames'),
    ('TOO_LONG', 'a side is longer than ptts_dtw_max_frames()'),
    ('NOT_FINITE', 'a local cost is not finite (a NaN or Inf in the alignment columns)'),
    ('BAD_OFFSETS', 'the offsets do not lie inside the tensors')))
_DTW_PHASE_ALL = _hip._define('PTTS_DTW_PHASE_ALL')


def dtw_max_frames():
    """The longest side of one pair (ptts_dtw_max_frames; a host call, no device)."""
    return int(_hip.lib().ptts_dtw_max_frames())


def dtw_status(fn, info):
    """The one read-back of a DTW alignment: info [B] int32 device, the PTTS_DTW_* bits of every pair -> ValueError naming the first
    pair that has one set (ops.analysis_status for this family)."""
    info = info.cpu().numpy()
    for b in range(info.size):
        for bit, text in _DTW_STATUS:
            if info[b] & bit:
                raise ValueError('{}: utterance {}: {}'.format(fn, b, text))


def dtw_check(D, gen_lengths, ref_lengths, cols=None, scale=1.0):
    """The argument rules of ops.dtw_align, raisable without a device: D columns per row, the pairs' lengths (lists of ints),
    cols = (c0, c1) with 0 <= c0 < c1 <= D (None: all columns), a finite scale, no side longer than ptts_dtw_max_frames()
    -> (c0, c1, scale, the pairs' cell counts Tg Tr, the pairs' path slots max(Tg + Tr - 1, 0))."""
    if int(D) != D or D < 1:
        raise ValueError('ops.dtw_align: D={!r} columns'.format(D))
    c0, c1 = (0, D) if cols is None else cols
    if int(c0) != c0 or int(c1) != c1 or not 0 <= c0 < c1 <= D:
        raise ValueError('ops.dtw_align: cols={!r} is not a range 0 <= c0 < c1 <= D={}'.format(cols, D))
    scale = float(scale)
    if not math.isfinite(scale):
        raise ValueError('ops.dtw_align: scale={!r} is not finite'.format(scale))
    try:
        gl, rl = [int(n) for n in gen_lengths], [int(n) for n in ref_lengths]
    except (TypeError, ValueError):
        raise ValueError('ops.dtw_align: gen_lengths and ref_lengths have to be the utterances\' lengths')
    if len(gl) != len(rl) or not 1 <= len(gl) <= ANALYSIS_MAX_UTTS:
        raise ValueError('ops.dtw_align: {} generated and {} reference lengths (1 to {} pairs)'.format(len(gl), len(rl), ANALYSIS_MAX_UTTS))
    if min(gl + rl) < 0:
        raise ValueError('ops.dtw_align: a negative length')
    cap = dtw_max_frames()
    if max(gl + rl) > cap:
        raise ValueError('ops.dtw_align: a side of {} frames; at most {} (ptts_dtw_max_frames)'.format(max(gl + rl), cap))
    return int(c0), int(c1), scale, [g * r for g, r in zip(gl, rl)], [max(g + r - 1, 0) for g, r in zip(gl, rl)]


class DtwAlignment(object):
    """What ops.dtw_align returns.  gi, ri: device int32 [path_offsets.total], pair b's path in its first lengths[b] slots from
    path_offsets.off[b] (the slots behind them hold -1); path_offsets: the PackedOffsets of the slots, Tg + Tr - 1 per pair;
    lengths: device int32 [B], the path lengths L; cost: device fp64 [B], A(Tg-1, Tr-1); info: device int32 [B], the PTTS_DTW_*
    bits (0 for an aligned pair; a flagged one has L = 0).  host(): the paths as a list of (gi, ri) numpy arrays."""

    def __init__(self, gi, ri, path_offsets, lengths, cost, info):
        self.gi, self.ri, self.path_offsets, self.lengths, self.cost, self.info = gi, ri, path_offsets, lengths, cost, info

    def host(self):
        """[(gi_b, ri_b) numpy int32] for every pair, with one download."""
        n, B = self.path_offsets.total, len(self.path_offsets)
        flat = torch.cat([self.gi, self.ri, self.lengths]).cpu().numpy()
        gi, ri, L, off = flat[:n], flat[n:2 * n], flat[2 * n:2 * n + B], self.path_offsets.off
        return [(gi[off[b]:off[b] + L[b]].copy(), ri[off[b]:off[b] + L[b]].copy()) for b in range(B)]


def dtw_align(gen, ref, gen_lengths, ref_lengths, cols=None, scale=1.0, info=None, phases=None):
    """Dynamic time warping of B utterance pairs on the device (ptts_dtw_align_batch, csrc/dtw.hip; the definition with its tie
    rule: DESIGN.md section 3): gen [sum Tg, D] and ref [sum Tr, D] fp32 device, the utterances one after the other, gen_lengths
    and ref_lengths their frame counts (lists, or PackedOffsets), the local cost scale * ||gen[i, c0:c1] - ref[j, c0:c1]|| in fp64
    -> a DtwAlignment.  A pair's result depends on nothing but that pair, and the same input gives the same bytes.  What cannot be
    aligned (an empty side, a local cost that is not finite) is a PTTS_DTW_* bit in `info` [B] int32, which the op writes; without
    `info` the op reads the status back itself and raises the ValueError.  phases (tools/dtw_probe.py): a subset of the launches,
    on what the last call with the same arguments left in the workspace."""
    fn = 'dtw_align'
    if not (torch.is_tensor(gen) and torch.is_tensor(ref)) or gen.dim() != 2 or ref.dim() != 2 or gen.shape[1] != ref.shape[1]:
        raise ValueError('ops.{}: gen and ref have to be packed [rows, D] device tensors of one width'.format(fn))
    D = gen.shape[1]
    go = packed_offsets(gen_lengths, gen.device, fn, 'gen_lengths')
    ro = packed_offsets(ref_lengths, gen.device, fn, 'ref_lengths')
    c0, c1, scale, cells, slots = dtw_check(D, go.lengths, ro.lengths, cols, scale)
    if gen.shape[0] != go.total or ref.shape[0] != ro.total:
        raise ValueError('ops.{}: gen {} and ref {} are not [sum(lengths)={} and {}, D]'.format(fn, tuple(gen.shape), tuple(ref.shape),
                                                                                               go.total, ro.total))
    _no_backward(fn, gen, ref)
    f32c(gen, fn + '.gen'); f32c(ref, fn + '.ref')
    B, dev = len(go), gen.device
    po = packed_offsets(slots, dev, fn, 'path slots')
    info, own = _info(info, B, dev, fn)
    gi = torch.full((po.total,), -1, dtype=torch.int32, device=dev)
    ri = torch.full((po.total,), -1, dtype=torch.int32, device=dev)
    L = torch.empty(B, dtype=torch.int32, device=dev)
    cost = torch.empty(B, dtype=torch.float64, device=dev)
    l = _hip.lib()
    b0 = 0
    while b0 < B:                                           # as many pairs per call as DTW_WORKSPACE_CAP holds, at least one
        n, ncells, nslots = 0, 0, 0
        while b0 + n < B and (n == 0 or l.ptts_dtw_workspace_bytes(ncells + cells[b0 + n], n + 1, po.total) <= DTW_WORKSPACE_CAP):
            ncells += cells[b0 + n]
            n += 1
        nws = l.ptts_dtw_workspace_bytes(ncells, n, po.total)
        ws = _workspace(nws, dev)
        call('ptts_dtw_align_batch', ptr(gen) if go.total else None, ptr(go.dev[b0:]), go.total, ptr(ref) if ro.total else None,
             ptr(ro.dev[b0:]), ro.total, n, D, c0, c1, scale, max(go.lengths[b0:b0 + n]), max(ro.lengths[b0:b0 + n]), ncells,
             ptr(po.dev[b0:]), po.total, ptr(gi) if po.total else None, ptr(ri) if po.total else None, ptr(L[b0:]), ptr(cost[b0:]),
             ptr(info[b0:]), _DTW_PHASE_ALL if phases is None else int(phases), ptr(ws), nws, stream(), tag=(n, ncells, D))
        b0 += n
    if own:
        dtw_status('ops.' + fn, info)
    return DtwAlignment(gi, ri, po, L, cost, info)


# ----------------------------------------------------------------------------------------------
# forced alignment by flat-start Viterbi training (the build's own): csrc/align.hip
# ----------------------------------------------------------------------------------------------
ALIGN_WORKSPACE_CAP = 1 << 30       # bytes of workspace one ptts_align_viterbi_batch call may use; a larger batch is split along B
ALIGN_FLAGS = tuple((name, _hip._define('PTTS_ALIGN_' + name), text) for name, text in (
    ('EMPTY', 'no frames or no states'),
    ('TOO_LONG', 'more states than ptts_align_max_states()'),
    ('TOO_SHORT', 'fewer frames than states'),
    ('NOT_FINITE', 'an emission or the score is not finite (a NaN or Inf in the alignment columns or the model)'),
    ('BAD_OFFSETS', 'the offsets do not lie inside the tensors'),
    ('BAD_GAUSS', 'a Gaussian index outside [0, Q)')))
_ALIGN_PHASE_ALL = _hip._define('PTTS_ALIGN_PHASE_ALL')


def align_max_states():
    """The longest chain of one utterance (ptts_align_max_states; a host call, no device)."""
    return int(_hip.lib().ptts_align_max_states())


def align_status(fn, info, names=None):
    """The one read-back of an alignment: info [B] int32 (device or numpy), the PTTS_ALIGN_* bits of every utterance -> ValueError
    naming the first utterance that has one set (names[b] if given, else its index) and the flag."""
    info = info.cpu().numpy() if torch.is_tensor(info) else np.asarray(info)
    for b in range(info.size):
        for flag, bit, text in ALIGN_FLAGS:
            if info[b] & bit:
                raise ValueError('{}: utterance {}: PTTS_ALIGN_{}: {}'.format(fn, b if names is None else names[b], flag, text))


def align_check(Dx, frame_lengths, state_lengths, Q, cols=None):
    """The argument rules of ops.align_viterbi, raisable without a device: Dx columns per row, the utterances' frame and state
    counts (lists of ints), Q Gaussians, cols = (c0, c1) with 0 <= c0 < c1 <= Dx (None: all columns)
    -> (c0, c1, the utterances' cell counts T N; 0 for one the kernels will flag)."""
    if int(Dx) != Dx or Dx < 1:
        raise ValueError('ops.align_viterbi: Dx={!r} columns'.format(Dx))
    c0, c1 = (0, Dx) if cols is None else cols
    if int(c0) != c0 or int(c1) != c1 or not 0 <= c0 < c1 <= Dx:
        raise ValueError('ops.align_viterbi: cols={!r} is not a range 0 <= c0 < c1 <= Dx={}'.format(cols, Dx))
    if int(Q) != Q or Q < 1:
        raise ValueError('ops.align_viterbi: Q={!r} Gaussians'.format(Q))
    try:
        fl, sl = [int(n) for n in frame_lengths], [int(n) for n in state_lengths]
    except (TypeError, ValueError):
        raise ValueError('ops.align_viterbi: frame_lengths and state_lengths have to be the utterances\' lengths')
    if len(fl) != len(sl) or not 1 <= len(fl) <= ANALYSIS_MAX_UTTS:
        raise ValueError('ops.align_viterbi: {} frame and {} state counts (1 to {} utterances)'.format(len(fl), len(sl), ANALYSIS_MAX_UTTS))
    if min(fl + sl) < 0:
        raise ValueError('ops.align_viterbi: a negative length')
    if sum(fl) >= 1 << 31 or sum(sl) >= 1 << 31:
        raise ValueError('ops.align_viterbi: {} frames and {} states; fewer than 2^31 each'.format(sum(fl), sum(sl)))
    cap = align_max_states()
    return int(c0), int(c1), [t * n if 1 <= n <= min(t, cap) else 0 for t, n in zip(fl, sl)]


class AlignResult(object):
    """What ops.align_viterbi returns, all on the device.  dur: int32 [sum N], the frames in every chain state; state: int32 [sum T],
    the chain state of every frame (None unless asked for); score: fp64 [B], V(T-1, N-1); info: int32 [B], the PTTS_ALIGN_* bits
    (0 for an aligned utterance; a flagged one has dur 0, state -1 and score NaN); frame_offsets, state_offsets: the PackedOffsets."""

    def __init__(self, dur, state, score, info, frame_offsets, state_offsets):
        self.dur, self.state, self.score, self.info = dur, state, score, info
        self.frame_offsets, self.state_offsets = frame_offsets, state_offsets


def _align_model_check(fn, mu, w, g):
    for name, t in (('mu', mu), ('w', w), ('g', g)):
        _dev_tensor(t, torch.float64, '{}.{}'.format(fn, name))
    if mu.dim() != 2 or min(mu.shape) < 1 or tuple(w.shape) != tuple(mu.shape) or tuple(g.shape) != (mu.shape[0],):
        raise ValueError('ops.{}: mu {}, w {} and g {} are not [Q,D], [Q,D] and [Q]'.format(fn, tuple(mu.shape), tuple(w.shape), tuple(g.shape)))
    return mu.shape


def _align_inputs(fn, X, frame_lengths, gauss, state_lengths):
    if not torch.is_tensor(X) or X.dim() != 2 or X.shape[1] < 1:
        raise ValueError('ops.{}: X has to be a packed [rows, Dx] device tensor'.format(fn))
    fo = packed_offsets(frame_lengths, X.device, fn, 'frame_lengths')
    so = packed_offsets(state_lengths, X.device, fn, 'state_lengths')
    if X.shape[0] != fo.total:
        raise ValueError('ops.{}: X {} is not [sum(frame_lengths)={}, Dx]'.format(fn, tuple(X.shape), fo.total))
    _no_backward(fn, X)
    f32c(X, fn + '.X')
    _dev_tensor(gauss, torch.int32, fn + '.gauss', (so.total,))
    return fo, so


def _align_chunks(cells, fo, so, cap):
    """[(first utterance, count, cells)]: as many utterances per call as `cap` bytes of workspace hold, at least one."""
    l, B, b0, out = _hip.lib(), len(fo), 0, []
    while b0 < B:
        n, ncells = 0, 0
        while b0 + n < B and (n == 0 or l.ptts_align_workspace_bytes(ncells + cells[b0 + n], n + 1, int(fo.off[b0 + n + 1] - fo.off[b0])) <= cap):
            ncells += cells[b0 + n]
            n += 1
        out.append((b0, n, ncells))
        b0 += n
    return out


def align_viterbi(X, frame_lengths, gauss, state_lengths, mu, w, g, cols=None, want_state=True, info=None, phases=None,
                  workspace_bytes=None):
    """Viterbi alignment of B utterances to their chains on the device (ptts_align_viterbi_batch, csrc/align.hip; the definition
    with its tie rule -- staying wins -- is in DESIGN.md section 3): X [sum T, Dx] fp32 device, the utterances one after the other,
    frame_lengths their frame counts; gauss [sum N] int32 device, the Gaussian of every chain state, state_lengths the chains'
    lengths (lists, or PackedOffsets); mu, w [Q, D] and g [Q] fp64 device with D = c1 - c0 the width of cols (None: all columns of
    X) -> an AlignResult.  An utterance's result depends on nothing but that utterance, and the same input gives the same bytes.
    What cannot be aligned is a PTTS_ALIGN_* bit in `info` [B] int32, which the op writes; without `info` the op reads the status
    back itself and raises the ValueError.  workspace_bytes (default ALIGN_WORKSPACE_CAP): the batch goes through in chunks of
    utterances whose workspace stays below it.  phases (tools/align_probe.py): a subset of the launches, on what the last call with
    the same arguments left in the workspace."""
    fn = 'align_viterbi'
    fo, so = _align_inputs(fn, X, frame_lengths, gauss, state_lengths)
    Q, D = _align_model_check(fn, mu, w, g)
    c0, c1, cells = align_check(X.shape[1], fo.lengths, so.lengths, Q, cols)
    if c1 - c0 != D:
        raise ValueError('ops.{}: the model has {} columns, cols={} selects {}'.format(fn, D, (c0, c1), c1 - c0))
    B, dev = len(fo), X.device
    info, own = _info(info, B, dev, fn)
    dur = torch.zeros(so.total, dtype=torch.int32, device=dev)
    state = torch.full((fo.total,), -1, dtype=torch.int32, device=dev) if want_state else None
    score = torch.full((B,), float('nan'), dtype=torch.float64, device=dev)
    l = _hip.lib()
    for b0, n, ncells in _align_chunks(cells, fo, so, ALIGN_WORKSPACE_CAP if workspace_bytes is None else int(workspace_bytes)):
        f0, f1, s0, s1 = (int(v) for v in (fo.off[b0], fo.off[b0 + n], so.off[b0], so.off[b0 + n]))
        whole = n == B
        foff = fo.dev if whole else fo.dev[b0:b0 + n + 1] - f0
        soff = so.dev if whole else so.dev[b0:b0 + n + 1] - s0
        nws = l.ptts_align_workspace_bytes(ncells, n, f1 - f0)
        ws = _workspace(nws, dev)
        call('ptts_align_viterbi_batch', ptr(X[f0:]) if f1 > f0 else None, ptr(foff), f1 - f0, X.shape[1], c0, c1,
             ptr(gauss[s0:]) if s1 > s0 else None, ptr(soff), s1 - s0, ptr(mu), ptr(w), ptr(g), Q, n, ncells,
             ptr(dur[s0:]) if s1 > s0 else None, ptr(state[f0:]) if want_state and f1 > f0 else None, ptr(score[b0:]), ptr(info[b0:]),
             _ALIGN_PHASE_ALL if phases is None else int(phases), ptr(ws), nws, stream(), tag=(n, ncells, D))
    if own:
        align_status('ops.' + fn, info)
    return AlignResult(dur, state, score, info, fo, so)


def align_occurrences(gauss, Q):
    """The occurrence table of ptts_align_accumulate from the host's copy of gauss [sum N]: (occ int32 [sum N], the indices of the
    chain states sorted by Gaussian, equal ones in index order; occ_off int64 [Q+1], Gaussian q's run of occ), numpy arrays.  An
    index outside [0, Q) is a ValueError."""
    gauss = np.asarray(gauss)
    if gauss.ndim != 1 or gauss.dtype.kind not in 'iu' or (gauss.size and (gauss.min() < 0 or gauss.max() >= Q)):
        raise ValueError('ops.align_occurrences: gauss has to be a vector of integers in [0, {})'.format(Q))
    occ = np.argsort(gauss, kind='stable').astype(np.int32)
    occ_off = np.concatenate([[0], np.cumsum(np.bincount(gauss, minlength=Q))]).astype(np.int64)
    return occ, occ_off


def align_accumulate(X, frame_lengths, gauss, state_lengths, dur, occ, occ_off, Q, cols=None, sums=None):
    """The sufficient statistics of the Gaussians under a segmentation (ptts_align_accumulate): dur [sum N] int32 device, the
    frames of every chain state (ops.align_viterbi's, or ops.align_uniform's); occ, occ_off: the table of ops.align_occurrences on
    the device -> (count [Q] int64, s1 [Q,D], s2 [Q,D] fp64).  With sums = (count, s1, s2) the call ADDS to them (a corpus in
    several calls); a Gaussian without frames is left untouched.  No floating-point atomics: the same call writes the same bytes."""
    fn = 'align_accumulate'
    fo, so = _align_inputs(fn, X, frame_lengths, gauss, state_lengths)
    if len(fo) != len(so):
        raise ValueError('ops.{}: {} frame and {} state counts'.format(fn, len(fo), len(so)))
    if int(Q) != Q or Q < 1:
        raise ValueError('ops.{}: Q={!r} Gaussians'.format(fn, Q))
    Dx = X.shape[1]
    c0, c1 = (0, Dx) if cols is None else cols
    if int(c0) != c0 or int(c1) != c1 or not 0 <= c0 < c1 <= Dx:
        raise ValueError('ops.{}: cols={!r} is not a range 0 <= c0 < c1 <= Dx={}'.format(fn, cols, Dx))
    if fo.total >= 1 << 31 or so.total >= 1 << 31:
        raise ValueError('ops.{}: {} frames and {} states; fewer than 2^31 each'.format(fn, fo.total, so.total))
    D, dev = int(c1) - int(c0), X.device
    _dev_tensor(dur, torch.int32, fn + '.dur', (so.total,))
    _dev_tensor(occ, torch.int32, fn + '.occ', (so.total,))
    _dev_tensor(occ_off, torch.int64, fn + '.occ_off', (Q + 1,))
    if sums is None:
        sums = (torch.zeros(Q, dtype=torch.int64, device=dev), torch.zeros((Q, D), dtype=torch.float64, device=dev),
                torch.zeros((Q, D), dtype=torch.float64, device=dev))
    count, s1, s2 = sums
    _dev_tensor(count, torch.int64, fn + '.count', (Q,))
    _dev_tensor(s1, torch.float64, fn + '.s1', (Q, D))
    _dev_tensor(s2, torch.float64, fn + '.s2', (Q, D))
    nws = _hip.lib().ptts_align_accumulate_workspace_bytes(so.total)
    ws = _workspace(nws, dev)
    call('ptts_align_accumulate', ptr(X) if fo.total else None, ptr(fo.dev), fo.total, Dx, int(c0), int(c1), ptr(gauss) if so.total else None,
         ptr(so.dev), so.total, ptr(dur) if so.total else None, ptr(occ) if so.total else None, ptr(occ_off), int(Q), len(fo), ptr(count),
         ptr(s1), ptr(s2), ptr(ws), nws, stream(), tag=(len(fo), fo.total, int(Q), D))
    return count, s1, s2


def align_update(count, s1, s2, floor, mu, w, g, min_count=2):
    """The Gaussians from their statistics, in place (ptts_align_update): for count[q] >= min_count mu = s1 / count,
    var = max(s2 / count - mu mu, floor[d]), w = 1 / var, g = sum_d log var; a Gaussian below min_count keeps its mu, w, g.
    floor [D] fp64 device.  Returns (kept [Q] int32: 1 for a Gaussian that was kept, floored [Q] int32: its variances that took
    the floor), on the device."""
    fn = 'align_update'
    Q, D = _align_model_check(fn, mu, w, g)
    if isinstance(min_count, bool) or int(min_count) != min_count or min_count < 1:
        raise ValueError('ops.{}: min_count={!r} is not an integer >= 1'.format(fn, min_count))
    _dev_tensor(count, torch.int64, fn + '.count', (Q,))
    _dev_tensor(s1, torch.float64, fn + '.s1', (Q, D))
    _dev_tensor(s2, torch.float64, fn + '.s2', (Q, D))
    _dev_tensor(floor, torch.float64, fn + '.floor', (D,))
    kept = torch.empty(Q, dtype=torch.int32, device=mu.device)
    floored = torch.empty(Q, dtype=torch.int32, device=mu.device)
    call('ptts_align_update', ptr(count), ptr(s1), ptr(s2), ptr(floor), Q, D, int(min_count), ptr(mu), ptr(w), ptr(g), ptr(kept),
         ptr(floored), stream(), tag=(Q, D))
    return kept, floored


def align_uniform(fo, so):
    """The flat start: dur[n] = floor((n+1) T / N) - floor(n T / N) for every chain state, and the chain state of every frame, in
    integer arithmetic on the device -> (dur int32 [sum N], state int32 [sum T]).  Every utterance needs T >= N >= 1."""
    dev = fo.dev.device
    N = torch.from_numpy(np.asarray(so.lengths, dtype=np.int64)).to(dev)
    T = torch.from_numpy(np.asarray(fo.lengths, dtype=np.int64)).to(dev)
    n = torch.arange(so.total, dtype=torch.int64, device=dev) - torch.repeat_interleave(so.dev[:-1], N, output_size=so.total)
    Ts, Ns = (torch.repeat_interleave(v, N, output_size=so.total) for v in (T, N))
    dur = torch.div((n + 1) * Ts, Ns, rounding_mode='floor') - torch.div(n * Ts, Ns, rounding_mode='floor')
    state = torch.repeat_interleave(n, dur, output_size=fo.total)
    return dur.to(torch.int32), state.to(torch.int32)


class AlignModel(object):
    """Q diagonal Gaussians on the device as the kernels read them: mu [Q,D], w = 1 / var [Q,D], g = sum_d log var [Q], fp64."""

    def __init__(self, mu, w, g):
        self.mu, self.w, self.g = mu, w, g

    @classmethod
    def from_host(cls, mu, var, device):
        """mu, var [Q,D] numpy -> the model on `device` (w and g in fp64 on the host: 1 / var, the logs added in index order)."""
        mu, var = np.ascontiguousarray(mu, dtype=np.float64), np.ascontiguousarray(var, dtype=np.float64)
        if mu.ndim != 2 or mu.shape != var.shape or min(mu.shape) < 1 or not (var > 0).all() or not np.isfinite(mu).all():
            raise ValueError('AlignModel.from_host: mu and var have to be [Q,D], var positive')
        g = np.zeros(mu.shape[0])
        for d in range(mu.shape[1]):
            g = g + np.log(var[:, d])
        return cls(*(torch.from_numpy(a).to(device) for a in (mu, 1.0 / var, g)))

    def host(self):
        """(mu, var) [Q,D] numpy fp64."""
        return self.mu.cpu().numpy(), 1.0 / self.w.cpu().numpy()


def forced_align_train(X, frame_lengths, chains, Q, c0=0, c1=None, n_iter=20, var_floor=0.01, min_count=2, model=None,
                       workspace_bytes=ALIGN_WORKSPACE_CAP, names=None, trace=None):
    """Flat-start Viterbi training (segmental k-means) of Q diagonal Gaussians on a corpus, and its alignment.
    X [sum T, Dx] fp32 device: the corpus packed row-wise once; frame_lengths: the utterances' frame counts; chains: per utterance
    the Gaussian index of every chain state (a list of integer vectors); the alignment columns are X[:, c0:c1].
    Iteration 0 is the uniform segmentation (ops.align_uniform), accumulate, update; every later one aligns every utterance
    (in chunks of utterances whose workspace stays below workspace_bytes), accumulates from zeroed sums and updates.  It stops when
    no frame of the corpus changed its chain state, or after n_iter alignments.  floor[d] = var_floor x the variance of column d over
    all frames (two passes in fp64, torch on the device); a Gaussian with fewer than min_count frames keeps its values (mean 0,
    variance 1 from the flat start).  With `model` (an AlignModel) the flat start is skipped, and with n_iter = 0 besides the call
    only aligns: how new utterances are aligned with stored models.
    -> (AlignModel, dur int32 [sum N] device: the last alignment, history): history holds per iteration
    (total score: the utterances' scores added in index order, NaN for the flat start; frames that changed their chain state;
    Gaussians kept; variances floored).  Everything but the history stays on the device.  An utterance that cannot be aligned is a
    ValueError naming it (names[b], else its index) and its PTTS_ALIGN_* flag.  trace: a list that receives, per iteration, numpy
    copies of (dur, the utterances' scores, and mu, w, g as the alignment of that iteration read them; None for the flat start)."""
    fn = 'forced_align_train'
    if not torch.is_tensor(X) or X.dim() != 2:
        raise ValueError('ops.{}: X has to be a packed [rows, Dx] device tensor'.format(fn))
    Dx = X.shape[1]
    c1 = Dx if c1 is None else c1
    if isinstance(n_iter, bool) or int(n_iter) != n_iter or n_iter < 0:
        raise ValueError('ops.{}: n_iter={!r} is not an integer >= 0'.format(fn, n_iter))
    if not (math.isfinite(float(var_floor)) and var_floor > 0):
        raise ValueError('ops.{}: var_floor={!r} is not positive'.format(fn, var_floor))
    try:
        chains = [np.asarray(c).astype(np.int64).reshape(-1) for c in chains]
    except (TypeError, ValueError):
        raise ValueError('ops.{}: chains has to hold one vector of Gaussian indices per utterance'.format(fn))
    fl = list(frame_lengths.lengths) if isinstance(frame_lengths, PackedOffsets) else [int(n) for n in frame_lengths]
    if len(chains) != len(fl):
        raise ValueError('ops.{}: {} chains for {} utterances'.format(fn, len(chains), len(fl)))
    sl = [c.size for c in chains]
    c0, c1, cells = align_check(Dx, fl, sl, Q, (c0, c1))
    D, dev = c1 - c0, X.device
    gauss_host = np.concatenate(chains) if chains else np.zeros(0, np.int64)
    occ, occ_off = align_occurrences(gauss_host, Q)
    cap = align_max_states()
    for b, (t, n) in enumerate(zip(fl, sl)):                # what the kernels would flag, before the device is touched
        if not 1 <= n <= min(t, cap):
            flag = 'EMPTY' if n == 0 or t == 0 else 'TOO_LONG' if n > cap else 'TOO_SHORT'
            raise ValueError('ops.{}: utterance {}: PTTS_ALIGN_{}: {} frames for {} states (1 <= states <= frames, at most {} states)'.format(
                fn, b if names is None else names[b], flag, t, n, cap))
    fo, so = packed_offsets(fl, dev, fn, 'frame_lengths'), packed_offsets(sl, dev, fn, 'chains')
    gauss = torch.from_numpy(gauss_host.astype(np.int32)).to(dev)
    _align_inputs(fn, X, fo, gauss, so)
    occ, occ_off = torch.from_numpy(occ).to(dev), torch.from_numpy(occ_off).to(dev)
    history, prev, dur = [], None, None
    kept = floored = 0

    def reestimate(dur):
        sums = align_accumulate(X, fo, gauss, so, dur, occ, occ_off, Q, (c0, c1))
        k, f = align_update(*sums, floor, model.mu, model.w, model.g, min_count)
        return int(k.sum().item()), int(f.sum().item())

    if model is None:
        Xc = X[:, c0:c1].to(torch.float64)
        floor = (float(var_floor) * ((Xc - Xc.mean(dim=0)) ** 2).mean(dim=0)).contiguous()
        del Xc
        model = AlignModel(torch.zeros((Q, D), dtype=torch.float64, device=dev), torch.ones((Q, D), dtype=torch.float64, device=dev),
                           torch.zeros(Q, dtype=torch.float64, device=dev))
        dur, prev = align_uniform(fo, so)
        kept, floored = reestimate(dur)
        history.append((float('nan'), fo.total, kept, floored))
        if trace is not None:
            trace.append((dur.cpu().numpy(), None, None, None, None))
    else:
        if tuple(_align_model_check(fn, model.mu, model.w, model.g)) != (Q, D):
            raise ValueError('ops.{}: the model is not {} Gaussians of {} columns'.format(fn, Q, D))
        if n_iter > 0:
            Xc = X[:, c0:c1].to(torch.float64)
            floor = (float(var_floor) * ((Xc - Xc.mean(dim=0)) ** 2).mean(dim=0)).contiguous()
            del Xc
    done = 0
    while done < n_iter or (n_iter == 0 and done == 0 and dur is None):
        used = None if trace is None else tuple(t.cpu().numpy() for t in (model.mu, model.w, model.g))
        res = align_viterbi(X, fo, gauss, so, model.mu, model.w, model.g, (c0, c1), want_state=True,
                            info=torch.zeros(len(fo), dtype=torch.int32, device=dev), workspace_bytes=workspace_bytes)
        done += 1
        align_status('ops.' + fn, res.info, names)
        total = 0.0
        for v in res.score.cpu().numpy().tolist():
            total = total + v
        changed = fo.total if prev is None else int((res.state != prev).sum().item())
        dur, prev = res.dur, res.state
        if changed and n_iter > 0:
            kept, floored = reestimate(dur)
        history.append((total, changed, kept, floored))
        if trace is not None:
            trace.append((dur.cpu().numpy(), res.score.cpu().numpy()) + used)
        if changed == 0:
            break
    return model, dur, history


# ----------------------------------------------------------------------------------------------
# waveform pre-processing (vocoders.py:45-63 preprocwav): csrc/preproc.hip
# ----------------------------------------------------------------------------------------------
RESAMPLE_MAX_UP = 1024                      # rows of the resampler's table
RESAMPLE_MAX_TABLE_BYTES = 4 << 20
RESAMPLE_ZEROS, RESAMPLE_CUTOFF, RESAMPLE_BETA = 16, 0.95, 9.0
HIGHPASS_PADLEN = 15                        # the default odd extension, samples at each end
HIGHPASS_MAX_PADLEN = 1 << 20
HIGHPASS_MIN_FC_RATIO = 1.0 / 4000.0        # fc >= fs / 4000: where the blocked recurrence was checked against the sequential one
PREPROC_MAX_UTTS = 65535                    # utterances of one launch
_resample_tables = {}       # (up, down) -> h [up, 2 hw] on the host


def _rate(fn, name, value):
    if isinstance(value, bool) or not isinstance(value, (int, float, np.integer, np.floating)) or value != int(value) or not 0 < value < 1 << 30:
        raise ValueError('ops.{}: {}={!r} is not a positive integer rate'.format(fn, name, value))
    return int(value)


def preproc_check(fs_in, fs_out, fc=None, padlen=HIGHPASS_PADLEN):
    """ValueError for parameters the pre-processing kernels do not take: the rates positive integers with
    up = fs_out / gcd at most RESAMPLE_MAX_UP and a table of at most RESAMPLE_MAX_TABLE_BYTES; with `fc`, the high-pass cut-off in Hz,
    fs_out / 4000 <= fc < fs_out / 2 and padlen an integer in [0, HIGHPASS_MAX_PADLEN].  Returns (up, down, hw), hw = the half width
    of the resampler's window in input samples.  Touches no device."""
    fs_in, fs_out = _rate('preproc_check', 'fs_in', fs_in), _rate('preproc_check', 'fs_out', fs_out)
    g = math.gcd(fs_in, fs_out)
    up, down = fs_out // g, fs_in // g
    hw = int(math.ceil(RESAMPLE_ZEROS / (RESAMPLE_CUTOFF * min(1.0, up / float(down)))))
    if up > RESAMPLE_MAX_UP or up * 2 * hw * 8 > RESAMPLE_MAX_TABLE_BYTES:
        raise ValueError('resampling {} -> {} Hz needs a table of {} x {} taps: at most {} rows and {} bytes'.format(
            fs_in, fs_out, up, 2 * hw, RESAMPLE_MAX_UP, RESAMPLE_MAX_TABLE_BYTES))
    if fc is not None:
        if isinstance(fc, (str, bool)) or not fs_out * HIGHPASS_MIN_FC_RATIO <= float(fc) < fs_out / 2.0:
            raise ValueError('the high-pass cut-off {!r} Hz is outside [fs / 4000, fs / 2) at fs={}'.format(fc, fs_out))
        if isinstance(padlen, bool) or int(padlen) != padlen or not 0 <= padlen <= HIGHPASS_MAX_PADLEN:
            raise ValueError('padlen={!r} is not an integer in [0, {}]'.format(padlen, HIGHPASS_MAX_PADLEN))
    return up, down, hw


def resample_length(N, up, down):
    """Samples that N input samples give: ceil(N up / down)."""
    return (int(N) * up + down - 1) // down


def resample_table(fs_in, fs_out, device=None):
    """h [up, 2 hw] fp64, the Kaiser-windowed sinc of ptts_resample: row p, column j + hw - 1 holds
    c sinc(c tau) I0(beta sqrt(1 - (tau / R)^2)) / I0(beta) at tau = p / up - j (0 from |tau| = R on), c = 0.95 min(1, up / down),
    R = 16 / c, beta = 9.  Built on the host once per (up, down) and kept: a numpy array, or with `device` the device tensor."""
    up, down, hw = preproc_check(fs_in, fs_out)
    key = (up, down)
    if key not in _resample_tables:
        c = RESAMPLE_CUTOFF * min(1.0, up / float(down))
        R = RESAMPLE_ZEROS / c
        tau = np.arange(up, dtype=np.float64)[:, None] / up - np.arange(-hw + 1, hw + 1, dtype=np.float64)[None, :]
        inside = np.abs(tau) < R
        win = np.i0(RESAMPLE_BETA * np.sqrt(np.where(inside, 1.0 - (tau / R) ** 2, 0.0))) / np.i0(RESAMPLE_BETA)
        h = np.ascontiguousarray(np.where(inside, c * np.sinc(c * tau) * win, 0.0))
        h.setflags(write=False)
        _resample_tables[key] = h
    if device is None:
        return _resample_tables[key]
    dkey = ('resample', device, up, down)
    if dkey not in _spectrum_tables:
        _spectrum_tables[dkey] = torch.from_numpy(_resample_tables[key].copy()).to(device)
    return _spectrum_tables[dkey]


def _waveforms(fn, wav):
    """One [N] tensor or a list of them -> (list, was a list); ValueError for anything else, before the device is looked at."""
    single = torch.is_tensor(wav)
    wavs = [wav] if single else list(wav) if isinstance(wav, (list, tuple)) else None
    if wavs is None or not all(torch.is_tensor(w) and w.dim() == 1 for w in wavs):
        raise ValueError('ops.{}: wav is not an [N] tensor or a list of them'.format(fn))
    if len(wavs) > PREPROC_MAX_UTTS or sum(w.numel() for w in wavs) >= 1 << 40:
        raise ValueError('ops.{}: {} utterances, one launch takes at most {}'.format(fn, len(wavs), PREPROC_MAX_UTTS))
    _no_backward(fn, *wavs)
    return wavs, not single


def _packed(fn, wavs):
    """fp32 device waveforms -> (one packed array, its 64-bit offsets on the device)."""
    for w in wavs:
        f32c(w, '{}.wav'.format(fn))
    x = wavs[0] if len(wavs) == 1 else torch.cat(wavs)
    off = np.concatenate([[0], np.cumsum([w.numel() for w in wavs])]).astype(np.int64)
    return x, torch.from_numpy(off).to(x.device)


def resample(wav, fs_in, fs_out):
    """wav [N] at fs_in (fp32 device), or a list of them -> the same at fs_out, ceil(N up / down) samples each, by the rational-ratio
    Kaiser-windowed sinc of csrc/preproc.hip, all utterances in one launch, one thread per output sample.
    fs_in == fs_out returns its input and launches nothing."""
    up, down, hw = preproc_check(fs_in, fs_out)
    wavs, as_list = _waveforms('resample', wav)
    if up == down:
        return wav
    lens = [resample_length(w.numel(), up, down) for w in wavs]
    if not wavs:
        return []
    x, x_off = _packed('resample', wavs)
    y_off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    y = torch.empty(int(y_off[-1]), dtype=torch.float32, device=x.device)
    if y.numel():
        h = resample_table(fs_in, fs_out, device=x.device)
        y_off_dev = torch.from_numpy(y_off).to(x.device)
        call('ptts_resample', ptr(x), ptr(x_off), x.numel(), ptr(y), ptr(y_off_dev), y.numel(), max(lens), len(wavs), ptr(h),
             h.numel() * 8, up, down, hw, stream(), tag=(len(wavs), y.numel(), up, down))
    out = [y[int(a):int(b)] for a, b in zip(y_off[:-1], y_off[1:])]
    return out if as_list else out[0]


def highpass_tile():
    """(chunk, tile) of ptts_highpass_zerophase: the samples a lane owns and the samples a workgroup holds at a time."""
    chunk, tile = ctypes.c_int(0), ctypes.c_int(0)
    call('ptts_highpass_tile', ctypes.byref(chunk), ctypes.byref(tile))
    return chunk.value, tile.value


def highpass_zerophase(wav, fs, fc, padlen=HIGHPASS_PADLEN):
    """wav [N] at fs (fp32 device), or a list of them -> the same, high-passed at `fc` Hz by the order-4 Butterworth filter run forward
    and backward over the odd extension by `padlen` samples (csrc/preproc.hip): mathematically
    scipy.signal.sosfiltfilt(butter(4, fc / (fs / 2), 'high', output='sos'), wav, padtype='odd', padlen=padlen).  All utterances in one
    launch, one workgroup each; every one has to be longer than padlen."""
    preproc_check(fs, fs, fc, padlen)
    wavs, as_list = _waveforms('highpass_zerophase', wav)
    for w in wavs:
        if w.numel() <= padlen:
            raise ValueError('ops.highpass_zerophase: a waveform of {} samples is not longer than padlen={}'.format(w.numel(), padlen))
    if not wavs:
        return []
    x, off = _packed('highpass_zerophase', wavs)
    y = torch.empty_like(x)
    nws = _hip.lib().ptts_highpass_workspace_bytes(x.numel(), len(wavs), int(padlen))
    ws = _workspace(nws, x.device)
    call('ptts_highpass_zerophase', ptr(x), ptr(y), ptr(off), x.numel(), len(wavs), float(fs), float(fc), int(padlen), ptr(ws), nws,
         stream(), tag=(len(wavs), x.numel()))
    lens = [w.numel() for w in wavs]
    out = list(torch.split(y, lens))
    return out if as_list else out[0]


# ----------------------------------------------------------------------------------------------
# label front end (external/merlin/label_normalisation.py): csrc/labels.hip
# ----------------------------------------------------------------------------------------------
LABELS_MAX_LABEL = 1024                     # PTTS_LABELS_MAX_LABEL: bytes of a label the match kernel stages
LABELS_CC_POINTS = 600
LABELS_ANCHOR_START, LABELS_ANCHOR_END, LABELS_WILD = 0x10000, 0x20000, 0x40000
LABELS_CAPTURE_DIGITS, LABELS_CAPTURE_DECIMAL = 0, 1
LABELS_ERR_DIGITS, LABELS_ERR_FORMAT = 1, 2
LABELS_MODES = {'full': 0, 'minimal_frame': 1, 'state_only': 2, 'none': 3, 'minimal_phoneme': 4, 'coarse_coding': 5}
LABELS_FEATURES = {'full': 9, 'minimal_frame': 2, 'state_only': 1, 'none': 0, 'minimal_phoneme': 3, 'coarse_coding': 4}


def labels_match(labels, label_off, max_label_len, table):
    """labels: packed uint8 bytes of P labels, label_off [P+1] int32 (both device), max_label_len: the longest of them as the host
    measured it; table: dict of device tensors pat_bytes (uint8), pat_off, pat_meta [NP], qs_first [nQS+1], cqs [nCQS,3] (int32;
    None for an absent kind) as label_normalisation.QuestionSet.device_table builds it.  Returns V [P, nQS+nCQS] fp32 and
    status [P] int32 (0, or the failed capture: see include/percival_hip.h)."""
    if max_label_len > LABELS_MAX_LABEL:
        raise ValueError('a label of {} bytes exceeds the {} the match kernel stages'.format(max_label_len, LABELS_MAX_LABEL))
    _dev_tensor(labels, torch.uint8, 'labels_match.labels')
    P = _offsets(label_off, 'labels_match', 'label_off', 'P')
    NP = table['pat_off'].numel()
    _dev_tensor(table['pat_bytes'], torch.uint8, 'labels_match.pat_bytes')
    _dev_tensor(table['pat_off'], torch.int32, 'labels_match.pat_off', (NP,))
    _dev_tensor(table['pat_meta'], torch.int32, 'labels_match.pat_meta', (NP,))
    nQS = nCQS = 0
    if table.get('qs_first') is not None:
        nQS = _dev_tensor(table['qs_first'], torch.int32, 'labels_match.qs_first').numel() - 1
    if table.get('cqs') is not None:
        nCQS = _dev_tensor(table['cqs'], torch.int32, 'labels_match.cqs').shape[0]
    if nQS + nCQS < 1:
        raise ValueError('ops.labels_match: the question table has no question')
    V = torch.empty((P, nQS + nCQS), dtype=torch.float32, device=labels.device)
    status = torch.empty(P, dtype=torch.int32, device=labels.device)
    call('ptts_labels_match', ptr(labels), ptr(label_off), P, labels.numel(), int(max_label_len), ptr(table['pat_bytes']),
         table['pat_bytes'].numel(), ptr(table['pat_off']), ptr(table['pat_meta']), NP, ptr(table.get('qs_first')), nQS,
         ptr(table.get('cqs')), nCQS, ptr(V), ptr(status), stream(), tag=(P, nQS, nCQS))
    return V, status


def labels_expand(V, seg, T, subphone_feats, cc_table=None):
    """V [P,Q] fp32, seg [S,8] int32 (phone row, first output row, frame_number, state_index, state_index_backward,
    phone_duration, state_duration_base, 0; first rows ascending, T the end of the last) -> X [T, Q+F] fp32, F frame features of
    `subphone_feats` (LABELS_MODES); cc_table [3,600] fp32 for 'coarse_coding'."""
    if subphone_feats not in LABELS_MODES:
        raise ValueError('ops.labels_expand: unknown subphone_feats {!r}'.format(subphone_feats))
    P, Q = _rows2d(V, 'labels_expand', 'V', 'P,Q')
    _dev_tensor(seg, torch.int32, 'labels_expand.seg')
    if seg.dim() != 2 or seg.shape[1] != 8 or seg.shape[0] < 1:
        raise ValueError('ops.labels_expand: seg {} is not [S,8]'.format(tuple(seg.shape)))
    if subphone_feats == 'coarse_coding':
        _dev_tensor(cc_table, torch.float32, 'labels_expand.cc_table', (3, LABELS_CC_POINTS))
    else:
        cc_table = None
    T = int(T)
    if not 0 < T < 1 << 31:
        raise ValueError('ops.labels_expand: T={} rows'.format(T))
    X = torch.empty((T, Q + LABELS_FEATURES[subphone_feats]), dtype=torch.float32, device=V.device)
    call('ptts_labels_expand', ptr(V), ptr(seg), ptr(cc_table), ptr(X), P, Q, seg.shape[0], T, LABELS_MODES[subphone_feats], stream(),
         tag=(P, Q, seg.shape[0], T))
    return X


LABELS_SEG_STATES = 5                       # PTTS_LABELS_SEG_STATES
LABELS_SEG_CLAMPED = 1
LABELS_SEG_MAX_FRAMES = 1 << 24


def labels_segments(dur, unit_off, min_frames, max_frames):
    """dur [P,D] fp32 durations in frames (D = 5 states or 1 phone), unit_off [U+1] int32 utterance offsets over the P phones (both
    device) -> (seg [P*D,8] int32 as labels_expand reads it, rows [U+1] int32: every utterance's first output row and, last, the
    total T, status [U] int32: LABELS_SEG_CLAMPED where a duration was above max_frames), all on the device.  A duration is
    rounded to the nearest integer, ties to even; NaN and anything below min_frames count min_frames.  P = 0 is allowed."""
    f32c(dur, 'labels_segments.dur')
    if dur.dim() != 2 or dur.shape[1] not in (LABELS_SEG_STATES, 1):
        raise ValueError('ops.labels_segments: dur {} is not [P,{}] or [P,1]'.format(tuple(dur.shape), LABELS_SEG_STATES))
    _no_backward('labels_segments', dur)
    P, D = dur.shape
    U = _offsets(unit_off, 'labels_segments', 'unit_off', 'U')
    min_frames, max_frames = int(min_frames), int(max_frames)
    if not 0 <= min_frames <= max_frames <= LABELS_SEG_MAX_FRAMES:
        raise ValueError('ops.labels_segments: min_frames={} max_frames={} are not 0 <= min <= max <= {}'.format(
            min_frames, max_frames, LABELS_SEG_MAX_FRAMES))
    if P * D * max_frames >= 1 << 31:
        raise ValueError('ops.labels_segments: P={} D={} max_frames={} allow 2^31 rows or more'.format(P, D, max_frames))
    seg = torch.zeros((P * D, 8), dtype=torch.int32, device=dur.device)      # zeros: phones outside every utterance own no row
    rows = torch.empty(U + 1, dtype=torch.int32, device=dur.device)
    status = torch.empty(U, dtype=torch.int32, device=dur.device)
    call('ptts_labels_segments', ptr(dur), ptr(unit_off), P, D, U, min_frames, max_frames, ptr(seg), ptr(rows), ptr(status), stream(),
         tag=(P, D, U))
    return seg, rows, status
