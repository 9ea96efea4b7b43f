"""Timing of the label front end (csrc/labels.hip, external/merlin/label_normalisation.py) on the fixtures of tests/golden/labels:
host wall time and HIP-event time of the two launches at a corpus-sized batch, and files per second end to end.

    python tools/labels_probe.py [--copies 70] [--files 100] [--reps 5] [--utts 64] [--ab-reps 15]

Prints one JSON line.  `match`: the fixtures' 144 phone labels replicated `copies` times (10 080 phones at 70, about 40 000 at 280) against the
shipped question set; `expand`: their segment tables replicated the same way, GB/s against the T x 425 floats it has to write;
`end_to_end`: `files` label files (the five fixtures, cycled) through perform_normalisation into a temporary directory, with the
share of the wall time spent parsing text, on the device path (upload, two launches, download) and writing files;
`from_durations`: a batch of `utts` utterances (the five fixtures, cycled) from durations -- labels without times and a device tensor of
the aligned files' own state durations through normalise_with_durations (ptts_labels_segments + _match + _expand, the rows left on the
device; a second figure adds their download) -- beside perform_normalisation on the aligned files of the same durations (text with
times in, float32 files out), the two alternating in one process `ab_reps` times: median and p10-p90 of the wall time, and the
HIP-event time of the three launches of ptts_labels_segments alone.
"""
from __future__ import print_function

import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
G = os.path.join(ROOT, 'tests', 'golden', 'labels')
FIDS = ['arctic_a0002', 'arctic_a0004', 'arctic_a0005', 'arctic_a0006', 'arctic_a0008']


def timed(fn, reps):
    """(best wall ms including the stream synchronisation, best HIP-event ms of the launch) over `reps` calls after one warm-up."""
    import torch
    from percivaltts_amd import _hip
    fn()
    torch.cuda.synchronize()
    wall, dev = [], []
    for _ in range(reps):
        with _hip.KernelTimer() as kt:
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            wall.append(1e3 * (time.perf_counter() - t0))
        dev.append(sum(ms for _, _, ms in kt.durations_ms()))
    return min(wall), min(dev)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--copies', type=int, default=70)
    ap.add_argument('--files', type=int, default=100)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--utts', type=int, default=64)
    ap.add_argument('--ab-reps', type=int, default=15)
    args = ap.parse_args()
    import torch
    from percivaltts_amd import compose, ops
    from percivaltts_amd.external.merlin import label_normalisation as ln
    dev = compose._device()
    norm = ln.HTSLabelNormalisation(os.path.join(G, 'questions-radio_dnn_416.hed'))
    parsed = [norm._parse(os.path.join(G, 'label_state_align', fid + '.lab'), 'state_align') for fid in FIDS] * args.copies

    phones, segs, p0, row = [], [], 0, 0
    for ph, sg in parsed:
        sg = np.concatenate([sg, np.zeros((len(sg), 1), np.int32)], axis=1)
        sg[:, 0] += p0; sg[:, 1] += row
        segs.append(sg); phones.extend(ph)
        p0 += len(ph); row += int(sg[:, 2].sum())
    off = np.zeros(len(phones) + 1, dtype=np.int32)
    off[1:] = np.cumsum([len(p) for p in phones])
    to = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    labels_d, off_d, seg_d = to(np.frombuffer(b''.join(phones), dtype=np.uint8).copy()), to(off), to(np.concatenate(segs))
    table = norm.questions.device_table(dev)
    maxlen = max(len(p) for p in phones)
    V, _ = ops.labels_match(labels_d, off_d, maxlen, table)
    mw, md = timed(lambda: ops.labels_match(labels_d, off_d, maxlen, table), args.reps)
    ew, ed = timed(lambda: ops.labels_expand(V, seg_d, row, 'full'), args.reps)
    out_bytes = row * norm.dimension * 4
    result = dict(device=torch.cuda.get_device_name(dev),
                  match=dict(phones=len(phones), questions=norm.dict_size, patterns=len(norm.questions.patterns), label_bytes=int(off[-1]),
                             wall_ms=round(mw, 3), event_ms=round(md, 3), us_per_phone=round(1e3 * md / len(phones), 4)),
                  expand=dict(rows=row, width=norm.dimension, segments=int(seg_d.shape[0]), bytes_written=out_bytes, wall_ms=round(ew, 3),
                              event_ms=round(ed, 3), write_GBps=round(out_bytes / (ed * 1e-3) / 1e9, 1)))

    with tempfile.TemporaryDirectory() as d:
        ins = [os.path.join(G, 'label_state_align', FIDS[i % len(FIDS)] + '.lab') for i in range(args.files)]
        outs = [os.path.join(d, '{:05d}.lab'.format(i)) for i in range(args.files)]
        norm.perform_normalisation(ins[:5], outs[:5])
        t0 = time.perf_counter()
        norm.perform_normalisation(ins, outs)
        total = time.perf_counter() - t0
        t0 = time.perf_counter()
        chunk = [norm._parse(f, 'state_align') for f in ins]
        t_parse = time.perf_counter() - t0
        t0 = time.perf_counter()
        X, offs = norm._run_chunk(chunk, dev)
        t_device = time.perf_counter() - t0
        t0 = time.perf_counter()
        for i, o in enumerate(outs): X[offs[i]:offs[i + 1]].tofile(o)
        t_write = time.perf_counter() - t0
    result['end_to_end'] = dict(files=args.files, frames=int(offs[-1]), seconds=round(total, 4), files_per_s=round(args.files / total, 1),
                                parse_s=round(t_parse, 4), device_path_s=round(t_device, 4), write_s=round(t_write, 4))
    result['from_durations'] = from_durations(norm, dev, args.utts, args.ab_reps)
    print(json.dumps(result))


def from_durations(norm, dev, utts, reps):
    import torch
    from percivaltts_amd import _hip, ops
    pct = lambda v: dict(median_ms=round(float(np.median(v)), 3), p10_ms=round(float(np.percentile(v, 10)), 3),
                         p90_ms=round(float(np.percentile(v, 90)), 3))
    with tempfile.TemporaryDirectory() as d:
        aligned = [os.path.join(G, 'label_state_align', FIDS[i % len(FIDS)] + '.lab') for i in range(utts)]
        bare, durs = [], []
        for fid in FIDS:                                        # labels without times, one per phone
            path = os.path.join(d, fid + '.lab')
            with open(os.path.join(G, 'label_phone_align', fid + '.lab')) as f, open(path, 'w') as g:
                g.writelines(line.split()[-1] + '\n' for line in f if line.strip())
            bare.append(path)
            durs.append(norm.extract_dur_features(os.path.join(G, 'label_state_align', fid + '.lab')))
        labels = [bare[i % len(FIDS)] for i in range(utts)]
        dur_d = torch.from_numpy(np.concatenate([durs[i % len(FIDS)] for i in range(utts)])).to(dev)
        outs = [os.path.join(d, '{:05d}.bin'.format(i)) for i in range(utts)]

        def device_rows():
            X, offs = norm.normalise_with_durations(labels, dur_d, 'state_align', min_frames=0)
            torch.cuda.synchronize()
            return X, offs

        X, offs = device_rows()
        norm.perform_normalisation(aligned, outs)
        same = all(np.fromfile(outs[i], dtype=np.float32).tobytes() == X[offs[i]:offs[i + 1]].cpu().numpy().tobytes() for i in range(min(utts, 5)))
        t_dev, t_host, t_files = [], [], []
        for _ in range(reps):                                   # alternating, one process
            t0 = time.perf_counter(); X, offs = device_rows(); t_dev.append(1e3 * (time.perf_counter() - t0))
            t0 = time.perf_counter(); X, offs = device_rows(); X.cpu(); t_host.append(1e3 * (time.perf_counter() - t0))
            t0 = time.perf_counter(); norm.perform_normalisation(aligned, outs); t_files.append(1e3 * (time.perf_counter() - t0))
        uoff = np.zeros(utts + 1, dtype=np.int32)
        uoff[1:] = np.cumsum([len(durs[i % len(FIDS)]) for i in range(utts)])
        uoff_d = torch.from_numpy(uoff).to(dev)
        _, seg_ms = timed(lambda: ops.labels_segments(dur_d, uoff_d, 0, 10000), reps)
    return dict(utterances=utts, phones=int(dur_d.shape[0]), rows=int(offs[-1]), same_bytes_as_aligned=bool(same),
                from_durations_rows_on_device=pct(t_dev), from_durations_rows_downloaded=pct(t_host),
                perform_normalisation_aligned_files=pct(t_files), segments_event_ms=round(seg_ms, 4))


if __name__ == '__main__':
    main()
