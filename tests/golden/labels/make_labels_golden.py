"""Regenerates the fixtures of tests/test_labels.py from a checkout of the reference project (percivaltts), which is NOT part of
this repository:

    python tests/golden/labels/make_labels_golden.py /path/to/percivaltts

Inputs copied from the reference's data: its question set external/merlin/questions-radio_dnn_416.hed and five of the ten
state-aligned label files of tests/slt_arctic_merlin_test.tar.gz; the phone-aligned versions are derived here by merging the five
state lines of every phone.  questions-handwritten.hed is written by hand and committed beside this script.

Expected outputs: the reference's own HTSLabelNormalisation (external/merlin/label_normalisation.py, imported from the checkout,
with `xrange` aliased to `range`, its only Python 2 construct on this path) run on those inputs, one .npz per (question set,
subphone_feats, alignment) it can run -- every supported combination but 'coarse_coding', whose table needs mlab.normpdf, which
matplotlib no longer has.  Each .npz maps a file id to its float32 [T, dimension] matrix.
"""
import builtins
import io
import os
import shutil
import sys
import tarfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
FIDS = ['arctic_a0002', 'arctic_a0004', 'arctic_a0005', 'arctic_a0006', 'arctic_a0008']
QUESTION_SETS = {'radio416': 'questions-radio_dnn_416.hed', 'handwritten': 'questions-handwritten.hed'}
COMBINATIONS = [('full', 'state_align'), ('minimal_frame', 'state_align'), ('state_only', 'state_align'), ('none', 'state_align'),
                ('minimal_phoneme', 'phone_align'), ('none', 'phone_align')]


def phone_aligned(state_lines):
    """Five state lines "start end label[k]" per phone -> one line "start end label"."""
    rows = [ln.split() for ln in state_lines if ln.strip()]
    assert len(rows) % 5 == 0
    out = []
    for i in range(0, len(rows), 5):
        assert [r[2][-3:] for r in rows[i:i + 5]] == ['[2]', '[3]', '[4]', '[5]', '[6]']
        out.append('{} {} {}\n'.format(rows[i][0], rows[i + 4][1], rows[i][2][:-3]))
    return out


def main(reference):
    shutil.copyfile(os.path.join(reference, 'percivaltts', 'external', 'merlin', QUESTION_SETS['radio416']),
                    os.path.join(HERE, QUESTION_SETS['radio416']))
    for d in ('label_state_align', 'label_phone_align'):
        os.makedirs(os.path.join(HERE, d), exist_ok=True)
    with tarfile.open(os.path.join(reference, 'tests', 'slt_arctic_merlin_test.tar.gz')) as tar:
        for fid in FIDS:
            text = tar.extractfile('slt_arctic_merlin_test/label_state_align/{}.lab'.format(fid)).read().decode('ascii')
            with open(os.path.join(HERE, 'label_state_align', fid + '.lab'), 'w') as f:
                f.write(text)
            with open(os.path.join(HERE, 'label_phone_align', fid + '.lab'), 'w') as f:
                f.writelines(phone_aligned(io.StringIO(text).readlines()))

    builtins.xrange = range
    sys.path.insert(0, os.path.join(reference, 'percivaltts', 'external', 'merlin'))
    import label_normalisation as ref                   # the reference's module, from the checkout
    for qname, qfile in QUESTION_SETS.items():
        for feats, align in COMBINATIONS:
            norm = ref.HTSLabelNormalisation(os.path.join(HERE, qfile), add_frame_features=True, subphone_feats=feats)
            out = {}
            for fid in FIDS:
                A = norm.extract_linguistic_features(os.path.join(HERE, 'label_' + align, fid + '.lab'), None, label_type=align)
                out[fid] = np.array(A, 'float32')        # what its array_to_binary_file writes
            path = os.path.join(HERE, '{}_{}_{}.npz'.format(qname, feats, align))
            np.savez_compressed(path, **out)
            print(path, os.path.getsize(path), {k: v.shape for k, v in out.items()})


if __name__ == '__main__':
    main(sys.argv[1])
