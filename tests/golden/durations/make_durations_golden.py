"""Regenerates the fixtures of tests/test_durations.py from a checkout of the reference project (percivaltts), which is NOT part
of this repository:

    python tests/golden/durations/make_durations_golden.py /path/to/percivaltts

Inputs: the label files and question sets already committed under tests/golden/labels/ (make_labels_golden.py put them there).
Two utterances, both question sets.

Expected outputs, all from the reference's own external/merlin/label_normalisation.py (imported from the checkout, with `xrange`
aliased to `range`), cast to float32 as its array_to_binary_file writes them:
  dur_features.npz            HTSLabelNormalisation.extract_dur_features for the six (feature_type, unit_size, feat_size) it computes
                              soundly, keys '<fid>/<label_type>/<feature_type>_<unit_size>_<feat_size>';
  <set>_duration_inputs.npz   HTSDurationLabelNormalisation.extract_linguistic_features on the state-aligned file, the phone-aligned
                              file, and a timing-less file with one bare label per line (written to a temporary directory from the
                              phone-aligned one), keys '<fid>/state_align', '<fid>/phone_align', '<fid>/bare'.
"""
import builtins
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
LABELS = os.path.join(os.path.dirname(HERE), 'labels')
FIDS = ['arctic_a0005', 'arctic_a0008']
QUESTION_SETS = {'radio416': 'questions-radio_dnn_416.hed', 'handwritten': 'questions-handwritten.hed'}
COMBINATIONS = {'state_align': [('numerical', 'state', 'phoneme'), ('numerical', 'phoneme', 'phoneme'), ('binary', 'state', 'frame'),
                                ('binary', 'phoneme', 'frame')],
                'phone_align': [('numerical', 'phoneme', 'phoneme'), ('binary', 'phoneme', 'frame')]}


def lab(fid, align):
    return os.path.join(LABELS, 'label_' + align, fid + '.lab')


def main(reference):
    builtins.xrange = range
    sys.path.insert(0, os.path.join(reference, 'percivaltts', 'external', 'merlin'))
    import label_normalisation as ref                   # the reference's module, from the checkout

    norm = ref.HTSLabelNormalisation(os.path.join(LABELS, QUESTION_SETS['handwritten']))
    out = {}
    for fid in FIDS:
        for align, combos in COMBINATIONS.items():
            for combo in combos:
                A = norm.extract_dur_features(lab(fid, align), None, align, *combo)
                out['{}/{}/{}'.format(fid, align, '_'.join(combo))] = np.array(A, 'float32')
    path = os.path.join(HERE, 'dur_features.npz')
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), {k: v.shape for k, v in out.items()})

    with tempfile.TemporaryDirectory() as tmp:
        for fid in FIDS:
            with open(lab(fid, 'phone_align')) as f, open(os.path.join(tmp, fid + '.lab'), 'w') as g:
                g.writelines(line.split()[-1] + '\n' for line in f if line.strip())
        for qname, qfile in QUESTION_SETS.items():
            dnorm = ref.HTSDurationLabelNormalisation(os.path.join(LABELS, qfile))
            out = {}
            for fid in FIDS:
                for key, fname in (('state_align', lab(fid, 'state_align')), ('phone_align', lab(fid, 'phone_align')),
                                   ('bare', os.path.join(tmp, fid + '.lab'))):
                    out['{}/{}'.format(fid, key)] = np.array(dnorm.extract_linguistic_features(fname, None), 'float32')
            path = os.path.join(HERE, '{}_duration_inputs.npz'.format(qname))
            np.savez_compressed(path, **out)
            print(path, os.path.getsize(path), {k: v.shape for k, v in out.items()})


if __name__ == '__main__':
    main(sys.argv[1])
