"""GRU / Bidirectional GRU (networktts.py:101-114: kl.GRU(reset_after=False), recurrent_activation left at TF 1.x's
'hard_sigmoid') on the HIP step kernels of csrc/gru.hip, against a float64 restatement of the Keras formulas.

    xp = x.W + b ;  z, r = hs(xp_z + h U_z), hs(xp_r + h U_r) ;  hh = tanh(xp_h + (r h) U_h) ;  h' = z h + (1 - z) hh
    hs(a) = clip(0.2 a + 0.5, 0, 1) ; direction 1 of a Bidirectional walks time backwards, outputs stay at their time index.

The restatement lives here (not in oracle/); its gradients come from autograd and are checked against finite differences on
the CPU."""
import math
import os

import numpy as np
import pytest
import torch

from oracle import percival_oracle as O


def hs(a):
    return torch.clamp(0.2 * a + 0.5, 0.0, 1.0)


def gru_ref(x, W, U, b, pre=None):
    """float64 torch: x [B,T,In], W [nd,In,3H], U [nd,H,3H], b [nd,3H] -> h [B,T,nd*H].  `pre` (a list) collects the z|r
    pre-activations."""
    nd, H = U.shape[0], U.shape[1]
    B, T = x.shape[0], x.shape[1]
    outs = []
    for d in range(nd):
        xp = x @ W[d] + b[d]
        h = x.new_zeros(B, H)
        seq = [None] * T
        for t in (range(T - 1, -1, -1) if d == 1 else range(T)):
            a_zr = xp[:, t, :2 * H] + h @ U[d][:, :2 * H]
            if pre is not None:
                pre.append(a_zr.detach())
            z, r = hs(a_zr[:, :H]), hs(a_zr[:, H:])
            hh = torch.tanh(xp[:, t, 2 * H:] + (r * h) @ U[d][:, 2 * H:])
            h = z * h + (1 - z) * hh
            seq[t] = h
        outs.append(torch.stack(seq, dim=1))
    return torch.cat(outs, dim=-1)


def np_gru(x, W, U, b):
    """A plain numpy loop over samples, steps and units."""
    nd, H = U.shape[0], U.shape[1]
    B, T = x.shape[0], x.shape[1]
    out = np.zeros((B, T, nd * H))
    for d in range(nd):
        for bi in range(B):
            h = np.zeros(H)
            for t in (range(T - 1, -1, -1) if d == 1 else range(T)):
                xp = x[bi, t] @ W[d] + b[d]
                z = np.array([min(max(0.2 * (xp[j] + h @ U[d][:, j]) + 0.5, 0.0), 1.0) for j in range(H)])
                r = np.array([min(max(0.2 * (xp[H + j] + h @ U[d][:, H + j]) + 0.5, 0.0), 1.0) for j in range(H)])
                hh = np.array([math.tanh(xp[2 * H + j] + (r * h) @ U[d][:, 2 * H + j]) for j in range(H)])
                h = z * h + (1 - z) * hh
                out[bi, t, d * H:(d + 1) * H] = h
    return out


def rand_gru(B, T, In, H, nd, seed, wscale=1.0):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, T, In, generator=g, dtype=torch.float64)
    W = torch.randn(nd, In, 3 * H, generator=g, dtype=torch.float64) / math.sqrt(In) * wscale
    U = torch.randn(nd, H, 3 * H, generator=g, dtype=torch.float64) / math.sqrt(H) * wscale
    b = torch.randn(nd, 3 * H, generator=g, dtype=torch.float64) * 0.2 * wscale
    return x, W, U, b


# ---------------------------------------------------------------------------------------------------------------------------
# CPU: the restatement itself
# ---------------------------------------------------------------------------------------------------------------------------
def test_hard_sigmoid_is_the_keras_clip():
    a = torch.linspace(-4.0, 4.0, 801, dtype=torch.float64)
    np.testing.assert_array_equal(hs(a).numpy(), np.clip(0.2 * a.numpy() + 0.5, 0.0, 1.0))
    assert float(hs(torch.tensor(-2.5, dtype=torch.float64))) == 0.0 and float(hs(torch.tensor(2.5, dtype=torch.float64))) == 1.0


@pytest.mark.parametrize('case', [(2, 5, 3, 4, 1), (3, 4, 6, 5, 2)])
def test_restatement_matches_a_numpy_loop(case):
    B, T, In, H, nd = case
    x, W, U, b = rand_gru(B, T, In, H, nd, seed=1)
    got = gru_ref(x, W, U, b).numpy()
    want = np_gru(x.numpy(), W.numpy(), U.numpy(), b.numpy())
    np.testing.assert_allclose(got, want, rtol=1e-12, atol=1e-12)


def test_restatement_gradients_match_central_differences():
    """Small weights keep every gate pre-activation well inside (-2.5, 2.5), where hs is smooth."""
    x, W, U, b = rand_gru(2, 4, 3, 3, 2, seed=2, wscale=0.5)
    pre = []
    with torch.no_grad():
        gru_ref(x, W, U, b, pre=pre)
    assert max(float(p.abs().max()) for p in pre) < 2.3
    args = tuple(t.clone().requires_grad_(True) for t in (x, W, U, b))
    assert torch.autograd.gradcheck(lambda *a: gru_ref(*a), args, eps=1e-6, atol=1e-7, rtol=1e-6)


def test_gru_entry_points_reject_bad_arguments():
    """PTTS_EINVAL for B, T, H < 1 or ndir not in {1, 2} and PTTS_EWORKSPACE for a short workspace: both are returned before
    any launch (the tensor pointers are never dereferenced on the host), so no GPU is needed."""
    import ctypes
    from percivaltts_amd import _hip
    if not os.path.exists(_hip.LIB_PATH):
        pytest.skip('libpercival_hip.so not built (run __graft_entry__.build())')
    lib = _hip.lib()
    p = ctypes.c_void_p(256)           # non-null, never read
    EINVAL, EWORKSPACE = -1, -3
    for B, T, H, nd in ((0, 5, 4, 1), (2, 0, 4, 1), (2, 5, 0, 2), (2, 5, 4, 0), (2, 5, 4, 3)):
        assert lib.ptts_gru_fwd(p, p, p, p, p, p, 1 << 30, B, T, H, nd, None) == EINVAL
        assert lib.ptts_gru_bwd(p, p, p, p, p, p, 1 << 30, B, T, H, nd, None) == EINVAL
    assert lib.ptts_gru_fwd(None, p, p, p, p, p, 1 << 30, 2, 5, 4, 2, None) == EINVAL
    assert lib.ptts_gru_bwd(p, p, p, p, None, p, 1 << 30, 2, 5, 4, 2, None) == EINVAL
    for nd in (1, 2):
        nf, nb = lib.ptts_gru_fwd_workspace_bytes(3, 7, 70, nd), lib.ptts_gru_bwd_workspace_bytes(3, 7, 70, nd)
        assert lib.ptts_gru_fwd(p, p, p, p, p, p, nf - 1, 3, 7, 70, nd, None) == EWORKSPACE
        assert lib.ptts_gru_fwd(p, p, p, p, p, None, nf, 3, 7, 70, nd, None) == EWORKSPACE
        assert lib.ptts_gru_bwd(p, p, p, p, p, p, nb - 1, 3, 7, 70, nd, None) == EWORKSPACE
        assert 'workspace' in _hip.last_error()


# ---------------------------------------------------------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------------------------------------------------------
def _dev(t, grad=False):
    d = t.to(torch.float32).cuda().contiguous()
    return d.requires_grad_(True) if grad else d


def close(got, want, rtol, atol, what, kink_entries=0):
    """Elementwise bound; with kink_entries > 0 (fp64 gate pre-activations within 1e-5 of +-2.5, where fp32 may land on the
    other side of the clip and the hard-sigmoid derivative jumps by 0.2) a relative L2 bound of 2e-2 instead."""
    got = got.detach().cpu().to(torch.float64)
    want = want.detach().cpu().to(torch.float64)
    assert got.shape == want.shape, what
    err = (got - want).abs()
    bad = err > atol + rtol * want.abs()
    if not bad.any():
        return
    rel = float(err.norm()) / max(float(want.norm()), 1e-300)
    if kink_entries > 0:
        print('{}: {} pre-activations within 1e-5 of +-2.5: relative L2 {:.3e}'.format(what, kink_entries, rel))
        assert rel <= 2e-2, '{}: relative L2 {:.3e}'.format(what, rel)
        return
    i = int(torch.argmax(err))
    raise AssertionError('{}: {}/{} off, worst err {:.3e} (got {:.6e} want {:.6e}), rel L2 {:.3e}'.format(
        what, int(bad.sum()), err.numel(), float(err.flatten()[i]), float(got.flatten()[i]), float(want.flatten()[i]), rel))


@pytest.mark.gpu
@pytest.mark.parametrize('case', [(3, 7, 5, 4, 1), (2, 1, 3, 5, 2), (16, 20, 24, 64, 2), (5, 33, 10, 70, 2), (1, 57, 425, 4, 2),
                                  (64, 6, 40, 256, 2)])
def test_gru_op_matches_fp64(case):
    from percivaltts_amd import ops
    B, T, In, H, nd = case
    x, W, U, b = rand_gru(B, T, In, H, nd, seed=10)
    dh = torch.randn(B, T, nd * H, generator=torch.Generator().manual_seed(11), dtype=torch.float64)
    pre = []
    rs = [t.clone().requires_grad_(True) for t in (x, W, U, b)]
    hr = gru_ref(*rs, pre=pre)
    hr.backward(dh)
    kinks = int(sum(int(((p.abs() - 2.5).abs() < 1e-5).sum()) for p in pre))
    ds = [_dev(t, True) for t in (x, W, U, b)]
    hd = ops.gru(*ds)
    close(hd, hr, 2e-4, 2e-5, 'h')
    hd.backward(_dev(dh))
    for name, d, r in zip(('dx', 'dW', 'dU', 'db'), ds, rs):
        close(d.grad, r.grad, 3e-4, 2e-4, name, kinks)


def _generic(H=4, B=2):
    import percivaltts_amd
    from percivaltts_amd import vocoders, modeltts_common
    cfg = percivaltts_amd.configuration()
    cfg.arch_hiddenwidth = H
    cfg.train_batch_size = B
    voc = vocoders.VocoderPML(16000, 0.005, 65, 17)
    return cfg, modeltts_common.Generic(425, voc, layertypes=['GRU', 'BGRU'], cfgarch=cfg)


def _inject(model, seed):
    """Random weights of the model's shapes (float64), set into the model; order: GRU (kernel, recurrent, bias), BGRU (same),
    lo_f0spec (kernel, bias), lo_nm (kernel, bias)."""
    g = torch.Generator().manual_seed(seed)
    ws = []
    for i, w in enumerate(model.kerasmodel.get_weights()):
        scale = 0.2 if i in (2, 5, 7, 9) else 1.0 / math.sqrt(w.shape[-2])
        ws.append(torch.randn(w.shape, generator=g, dtype=torch.float64) * scale)
    model.kerasmodel.set_weights([w.to(torch.float32).numpy() for w in ws])
    return [w.to(torch.float32).to(torch.float64) for w in ws]        # what the model holds


def generic_ref(ws, X):
    k1, u1, b1, k2, u2, b2, wf, bf, wn, bn = ws
    h = gru_ref(gru_ref(X, k1, u1, b1), k2, u2, b2)
    return torch.cat([O.dense(h, wf, bf), torch.sigmoid(O.dense(h, wn, bn))], dim=-1)


@pytest.mark.gpu
def test_generic_gru_bgru_predict_matches_fp64_and_runs_on_hip():
    """The parent's torch loop used sigmoid gates: this fails there."""
    from percivaltts_amd import _hip, optimizertts
    cfg, model = _generic()
    ws = _inject(model, seed=3)
    assert [tuple(w.shape) for w in ws[:6]] == [(1, 425, 12), (1, 4, 12), (1, 12), (2, 4, 12), (2, 4, 12), (2, 12)]
    rng = np.random.RandomState(0)
    X = (rng.rand(2, 30, 425) * 2 - 1).astype(np.float32)
    out = model.predict(X)
    want = generic_ref(ws, torch.as_tensor(X, dtype=torch.float64))
    close(torch.as_tensor(out), want, 2e-4, 2e-5, 'predict')

    # one training step: the recurrence runs on ptts_gru_fwd / ptts_gru_bwd and nothing issues a stock matrix product
    opt = optimizertts.OptimizerTTS(cfg, model)
    opt.prepare()
    Y = rng.randn(2, 30, 83).astype(np.float32)
    with _hip.KernelTimer() as kt:
        opt.train_on_batch(0, X, Y)
    names = [r[0] for r in kt.records]
    assert 'ptts_gru_fwd' in names and 'ptts_gru_bwd' in names
    with torch.profiler.profile(activities=[torch.profiler.ProfilerActivity.CPU]) as prof:
        opt.train_on_batch(1, X, Y)
        torch.cuda.synchronize()
    ops_seen = {e.name for e in prof.events()}
    assert not ({'aten::mm', 'aten::addmm', 'aten::bmm', 'aten::matmul'} & ops_seen), sorted(ops_seen)


@pytest.mark.gpu
def test_generic_gru_bgru_lse_step_matches_fp64_adam():
    from percivaltts_amd import optimizertts
    cfg, model = _generic()
    ws = _inject(model, seed=4)
    opt = optimizertts.OptimizerTTS(cfg, model)
    opt.prepare()
    rng = np.random.RandomState(1)
    X = (rng.rand(2, 30, 425) * 2 - 1).astype(np.float32)
    Y = rng.randn(2, 30, 83).astype(np.float32)
    opt.train_on_batch(0, X, Y)
    got = model.kerasmodel.get_weights()

    ps = [w.clone().requires_grad_(True) for w in ws]
    pred = generic_ref(ps, torch.as_tensor(X, dtype=torch.float64))
    loss = O.specweighted_lse_loss(torch.as_tensor(Y, dtype=torch.float64), pred, 1.0)
    grads = torch.autograd.grad(loss, ps)
    ps = [p.detach().clone() for p in ps]
    c = opt.cfg                        # (the optimiser's configuration carries the LSE defaults)
    O.adam_keras(ps, grads, [torch.zeros_like(p) for p in ps], [torch.zeros_like(p) for p in ps], 1,
                 10 ** c.train_lse_learningrate_log10, c.train_lse_adam_beta1, c.train_lse_adam_beta2,
                 eps=10 ** c.train_lse_adam_epsilon_log10)
    for i, (g_, w) in enumerate(zip(got, ps)):
        np.testing.assert_allclose(g_, w.numpy(), rtol=1e-3, atol=1e-6, err_msg='weight {}'.format(i))


@pytest.mark.gpu
def test_generic_gru_bgru_training_driver(tmp_path, monkeypatch):
    """The reference's smoke line Generic(lab_size, vocoder, layertypes=['GRU', 'BGRU']) with OptimizerTTS
    (tests/test_smoke_tensorflowkeras.py:171-173) through the epoch loop on a synthetic corpus."""
    monkeypatch.setenv('PERCIVAL_CORPUS', str(tmp_path / 'corpus'))
    monkeypatch.chdir(tmp_path)
    import importlib
    import percivaltts_amd.run as run
    from percivaltts_amd import modeltts_common, optimizertts
    run = importlib.reload(run)
    cfg = run.cfg
    cfg.id_valid_start = 8
    cfg.id_valid_nb = 1
    cfg.id_test_nb = 1
    cfg.train_min_nbepochs = 1
    cfg.train_max_nbepochs = 2
    cfg.train_cancel_nodecepochs = 3
    cfg.train_nbepochs_scalewdata = False
    cfg.train_batch_size = 2
    cfg.arch_hiddenwidth = 4
    cfg.train_batch_lengthmax = 60
    run.synthesize_corpus(nfiles=10, minlen=90, maxlen=140)
    fids = run.readids(cfg.fileids)
    model = modeltts_common.Generic(run.ctxsize, run.vocoder, layertypes=['GRU', 'BGRU'], cfgarch=cfg)
    opt = optimizertts.OptimizerTTS(cfg, model)
    seen = []
    inner = opt.update_validation_cost
    opt.update_validation_cost = lambda *a: seen.append(inner(*a)) or seen[-1]
    opt.train(cfg.inpath, cfg.outpath, cfg.wpath, fids[:cfg.id_train_nb()],
              fids[cfg.id_valid_start:cfg.id_valid_start + cfg.id_valid_nb], 'model.h5')
    assert os.path.exists('model.h5.weights.npz')
    assert seen and all(np.isfinite(c) for c in seen)


@pytest.mark.gpu
def test_gru_deterministic_mode_is_bit_identical():
    """At (64,400,256,256,2) the weight gradients are products over K = B*T = 25 600: outside deterministic mode these take the
    split bf16x6 weight-gradient kernel or ptts_gemm's stream-K form, both of which combine partial sums with atomics.  The
    KernelTimer records show that in deterministic mode dW, dU_zr and dU_h went through ptts_gemm and the split kernel was
    not used."""
    from percivaltts_amd import _hip, ops
    x, W, U, b = rand_gru(64, 400, 256, 256, 2, seed=20)
    dh = _dev(torch.randn(64, 400, 512, generator=torch.Generator().manual_seed(21), dtype=torch.float64))
    was = ops.deterministic()
    ops.deterministic(True)
    try:
        runs = []
        for _ in range(2):
            ds = [_dev(t, True) for t in (x, W, U, b)]
            with _hip.KernelTimer() as kt:
                h = ops.gru(*ds)
                h.backward(dh)
            runs.append([h.detach()] + [d.grad for d in ds])
            calls = {(n, tag) for n, tag, _, _ in kt.records}
            for N in (768, 512, 256):          # dW, dU_zr, dU_h: [256, N] over K = 25 600 rows, transA = 1
                assert ('ptts_gemm', (256, N, 25600, 1, 0, 0)) in calls, sorted(calls)
            assert not any(n == 'ptts_dense_wgrad_bf16x6' for n, _ in calls)
        torch.cuda.synchronize()
    finally:
        ops.deterministic(was)
    for a, c in zip(*runs):
        assert torch.equal(a, c)
