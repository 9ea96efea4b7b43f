"""bench.py's own contract: the options, a plain run's result line (headline loop only) and --dump-outputs."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STEPS = 11          # the last timed step (batch id 10) trains the generator as well


def test_bench_options(monkeypatch):
    import bench
    monkeypatch.setattr(sys, 'argv', ['bench.py', '--gpus', '1', '--steps', '7', '--warmup', '2', '--dump-outputs', 'out'])
    a = bench.parse()
    assert a.steps == 7 and a.warmup == 2 and a.dump_outputs == 'out' and not a.full
    monkeypatch.setattr(sys, 'argv', ['bench.py', '--full'])
    a = bench.parse()
    assert a.full and a.dump_outputs is None


def _plain_run(outdir, env=None):
    cmd = [sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', '1', '--steps', str(STEPS), '--warmup', '1',
           '--batch', '4', '--frames', '40', '--dump-outputs', str(outdir)]
    out = subprocess.run(cmd, cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    assert out.returncode == 0, out.stderr.decode()[-2000:]
    lines = [l for l in out.stdout.decode().splitlines() if l.startswith('{')]
    assert len(lines) == 1, lines
    return json.loads(lines[0])


@pytest.mark.gpu
def test_bench_plain_run_and_dumped_outputs(tmp_path):
    """A plain run prints the headline figures only; --dump-outputs writes the last timed step's losses and state.  Two runs with
    the same arguments compute that step from the same inputs (seeded batches, the seeded training state, the device's random stream):
    by default their outputs agree to the rounding of the fp32 atomics' summation order, in deterministic mode (no fp32 atomics,
    DESIGN.md) bit for bit."""
    res = _plain_run(tmp_path / 'a')
    for k in ('metric', 'value', 'unit', 'higher_is_better', 'dtype', 'ms_per_step'):
        assert k in res, k
    assert res['steps'] == STEPS and res['warmup'] == 1 and res['value'] > 0 and res['ms_per_step'] > 0
    assert res['unit'] == 'frames/s' and res['higher_is_better'] is True and res['dtype'] == 'f32'
    for k in ('roofline', 'cpu_baseline', 'critic_step_ms', 'generator_step_ms', 'variant_fp32_mfma_gemms', 'pcie_inclusive',
              'reference_shape', 'config2_bf16', 'config4_gated_dilated_causal_T2000', 'all_exact_work_reductions_off'):
        assert k not in res, k
    names = sorted(f[:-4] for f in os.listdir(tmp_path / 'a'))
    # a generator loss exactly when the last step trains the generator ((steps - 1) % 5 == 0 in the steady-state schedule)
    must = {'critic_loss', 'critic_weights', 'generator_weights'}
    if (STEPS - 1) % 5 == 0:
        must.add('generator_loss')
    assert must <= set(names) <= must | {'critic_moving_averages', 'generator_moving_averages'}, names
    a = {n: np.load(tmp_path / 'a' / (n + '.npy')) for n in names}
    assert sum(v.nbytes for v in a.values()) <= 64 << 20
    for n, v in a.items():
        assert v.dtype == np.float32 and v.size > 0 and np.isfinite(v).all(), n
    assert a['critic_loss'].shape == (1,) and a['generator_loss'].shape == (1,)
    _plain_run(tmp_path / 'b')
    for n in names:
        b = np.load(tmp_path / 'b' / (n + '.npy'))
        assert b.shape == a[n].shape, n
        # the losses and moving averages to rounding (the state of the last timed step as it was before: 2-8 % apart); the weights
        # only bit for bit below: at this batch of 4 the atomics' rounding flips the sign of a few gradients, and Adam's first step
        # moves those weights by lr the other way
        if 'weights' not in n:
            np.testing.assert_allclose(b, a[n], rtol=1e-4, atol=1e-5, err_msg=n)
    det = dict(os.environ, PTTS_DETERMINISTIC='1')
    _plain_run(tmp_path / 'c', det)
    _plain_run(tmp_path / 'd', det)
    for n in names:
        c, d = np.load(tmp_path / 'c' / (n + '.npy')), np.load(tmp_path / 'd' / (n + '.npy'))
        assert c.shape == d.shape == a[n].shape, n
        assert np.array_equal(c, d), n
