"""Time ptts_mlpg alone (HIP events, warm, median of N launches) against the host loop of the fp64 restatement
(tests/test_mlpg.py: one scipy.linalg.solveh_banded per feature) on the same inputs.  Prints one JSON line per shape."""
from __future__ import print_function

import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from percivaltts_amd import _hip, ops              # noqa: E402
from tests import test_mlpg as R                    # noqa: E402

SHAPES = [(1, 1000, 163), (10, 1000, 163), (64, 400, 163)]
LAUNCHES = 30


def main():
    for B, T, D in SHAPES:
        y, mean, std = R.make_inputs(0, B, T, D, R.REF_WINS)
        var = std * std
        dy, dm, ds, dv = (torch.from_numpy(a).cuda() for a in (y, mean, std, var))
        for _ in range(3):
            out = ops.mlpg(dy, R.REF_WINS, dv, mean=dm, std=ds)
        torch.cuda.synchronize()
        ms = []
        for _ in range(LAUNCHES):
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            out = ops.mlpg(dy, R.REF_WINS, dv, mean=dm, std=ds)
            e.record()
            torch.cuda.synchronize()
            ms.append(s.elapsed_time(e))
        t0 = time.perf_counter()
        want = R.want_for(y, mean, std, var, R.REF_WINS)
        host_ms = (time.perf_counter() - t0) * 1e3
        R.check_tol(out.cpu().numpy(), want, str((B, T, D)))
        print(json.dumps({'shape': [B, T, D], 'device_ms_median': float(np.median(ms)), 'device_ms_min': float(np.min(ms)),
                          'device_ms_max': float(np.max(ms)), 'host_loop_ms': host_ms,
                          'workspace_bytes': int(_hip.lib().ptts_mlpg_workspace_bytes(B, T, D))}))
        sys.stdout.flush()


if __name__ == '__main__':
    main()
