"""csrc/elementwise.hip -- column reductions, BatchNorm finalisers, activations, WGAN-GP pieces, losses, Adam, clip, gated product --
at every branch its launchers choose between, against float64 (torch on the CPU, oracle.percival_oracle where it has the operation).

Every output and the reduction workspace lie inside a larger buffer whose margins hold a sentinel (Guard); the workspace has exactly
ptts_colstats_workspace_bytes(rows, C) bytes.  The margins are compared after every call: a tail or cap bug is a failed assert.  Outputs
start as NaN, so an element a kernel leaves out fails the finiteness check.  Each check prints its worst error / bound ratio
(`pytest -s`, lines `ew-ratio ...`).

Path -> case that reaches it (EW = 256 lanes, VU = 4 row sweeps in flight, R = rows per sweep):

  colreduce2_vec4_kernel (C % 4 == 0, C <= 1024, 16-byte aligned operands; C4 = C/4, R = 256 / C4)
      butterfly finish (C4 a power of two <= 32)      C = 4, 8 (COL_CASES)
      serial finish, C4 divides 256                   C = 256 (C4 = 64), C = 1024 (C4 = 256, R = 1)
      serial finish, idle lanes (256 % C4 != 0)       C = 12 (C4 = 3, R = 85), C = 260 (C4 = 65, R = 3)
      rows = 1, rows = R - 1, rows = R VU k + 1       (1, C), (255, 4) (84, 12) (2, 260), (3073, 4) (681, 12) (61, 260) (9, 1024)
      one pass / two passes of <= 1024 workgroups     (262144 + 77, 4): 257 chunks of R VU rows, one pass of 257 workgroups;
                                                      (1048576 + 77, 4): 1025 chunks, two passes of 513 workgroups
      fp32 fold ending mid-count (ActBwdOp4 only;     every case of test_affine_act_backward_every_path: a lane makes 1 or 2 sweeps of VU
      the statistics add in fp64)                     rows, so the 16-row fold is never complete.  (A complete fold needs 4 sweeps per
                                                      lane: 4 passes of 1024 workgroups = 12.6 M floats at any C, three times the size
                                                      limit of this file.)
  colreduce2_kernel, rows-per-workgroup branch (C <= 256)
      C = 1, 3, 86, 255; rows = 1; the 512-workgroup cap (174080 + 5, 3); C = 8 and C = 256 through the unaligned fallback
  colreduce2_kernel, slot branch (256 < C <= 2048)    C = 257, 1028 (C % 4 == 0 but too wide for vec4), 2047, 2048
  colreduce2_wide_kernel (C > 2048)                   (3, 2049); tests/test_lstm.py has the rest
  unaligned fallback (C % 4 == 0, operand at 4 mod 16) C = 8, 256 with x (and mask_src, dy, y, dx) at element offset 1: the same
                                                      values, references and bounds as the aligned cases of the same shape
  colreduce_final_kernel / ptts_partial_rows_sum      nrows 1, 31, 32, 33, 65 x ncols 1, 7, 8, 9, 520
  bn_finalize_kernel / bn_finalize_partials_kernel (C <= 16) / _wide_kernel (C > 16)
                                                      C = 1, 15, 16, 17, 300 x nrows 1, 33; count = 1; NULL gamma / beta; update on / off;
                                                      inference mode
  bn_stats_fused_kernel (ptts_bn_batch_stats)         C = 4, 8, 16; one workgroup (rows = 1, 700); the 256 cap (rows = 256 R VU + 77);
                                                      the existing test reaches C = 4 past the cap and C = 16 / 8 with one workgroup
  bn_bwd_coefs_kernel (plain and accumulate)          C = 1, 300; gamma, dgamma, dbeta NULL in turn
  axpby_cols_kernel                                   18 NULL combinations at C = 3 and 260; the 2048 cap at n = 2097152 + 1027
  gp_interpolate / gp_scale_rows (64-workgroup cap)   TD = 70001 > 65536
  gp_penalty_kernel (four wave sums, b += 256 loop)   B = 70 (two waves), B = 300 (all four, second loop step)
  gp_sqnorm_kernel (1024 lanes, i += 1024)            TD = 1, 63, 1023, 1025, 70001
  mean_scaled (256 cap) / wlse_fwd (512 cap)          n = 1048576 + 333 / 2097152 + 333 and the D = 7, 86 neighbours
  deterministic() single-workgroup form               test_losses_deterministic_mode
  ops.wasserstein_pair                                B = 1, 5 x T = 1, 33, one output unused
  ew_blocks cap (2048 workgroups)                     adam, weight_clip, wlse_bwd, axpby_cols, affine_act at n > 2097152;
                                                      float4 kernels (affine_act4, gated_mul) at n > 4194304
  adam_keras_kernel at a large step                   device step 9999 -> t = 10000, with each optimiser's own hyper-parameters
  gated_mul tail only / tail + body / cap             n = 1, 3 / 5, 1023 / 4194304 + 1030; b = +-30, +-88, +-89, +-100
  argument refusals, workspace size                   CPU tests at the end of the CPU section

Bounds.  Column sums and affine_act backward: those of tests/test_ops_gpu.py (test_colsums_modes_wide, test_affine_act_bwd_wide).
WGAN-GP, losses, gated product, affine_act forward: that file's default, rtol 1e-4 / atol 1e-5.  Adam and clip: those of
test_adam_keras_and_clip.  Finalisers and bn_bwd_coefs do their arithmetic in fp64 and round once to fp32: rtol 2^-23 (one fp32
rounding is 2^-24; the factor 2 covers the fp64 reference's own order of operations), atol 1e-12.  axpby_cols is three fp32
terms added without contraction: 4 x 2^-24 x (|c0| + |a c1| + |x c2|) per element.
"""
import ctypes
import functools
import itertools
import math
import os
import types

import numpy as np
import pytest
import torch

from oracle import percival_oracle as O

RT, AT = 1e-4, 1e-5                    # the default of tests/test_ops_gpu.py
SUM_TOL = (1e-5, 2e-3)                 # test_colsums_modes_wide
DSUM_TOL = (2e-4, 2e-3)                # test_affine_act_bwd_wide: dscale, dshift
F64_TOL = (2.0 ** -23, 1e-12)          # fp64 arithmetic, one rounding to fp32
U32 = 2.0 ** -24
ALPHA = 0.3
EPS, MOM = 1e-3, 0.99                  # ops.BN_EPS, ops.BN_MOMENTUM
EPS32, MOM32 = float(np.float32(EPS)), float(np.float32(MOM))     # as the kernels receive them (float arguments)
EINVAL, EWORKSPACE = -1, -3
IN_NONE, IN_LRELU, IN_MASKMUL = 0, 1, 2
ACTS = {None: 0, 'lrelu': 1, 'sigmoid': 2, 'tanh': 3}


def gen(seed):
    return torch.Generator().manual_seed(seed)


def r32(t):
    """float64 values that are exactly representable in float32: what the device tensor holds."""
    return t.to(torch.float32).to(torch.float64)


def randn32(g, *shape):
    return r32(torch.randn(*shape, generator=g, dtype=torch.float64))


def rand32(g, *shape):
    return r32(torch.rand(*shape, generator=g, dtype=torch.float64))


def lrelu64(p, mask_from=None):
    return torch.where((p if mask_from is None else mask_from) > 0, p, ALPHA * p)


# ---------------------------------------------------------------------------------------------------------------------------
# hand-written float64 references (checked against autograd / the oracle by the CPU tests below)
# ---------------------------------------------------------------------------------------------------------------------------
def act_fwd_ref(x, sc, sh, act):
    p = x if sc is None else x * sc + sh
    return {None: lambda t: t, 'lrelu': lrelu64, 'sigmoid': torch.sigmoid, 'tanh': torch.tanh}[act](p)


def act_bwd_ref(dy, x, y, sc, sh, act):
    """(dx, dscale, dshift) of y = act(x sc + sh).  The LeakyReLU mask is taken at the float32 pre-activation (one rounded product,
    one rounded sum: the library is built without contraction), the point at which the kernel's function has its kink; sigmoid and
    tanh take the derivative from the y handed in."""
    if act == 'lrelu':
        p32 = x.to(torch.float32) if sc is None else x.to(torch.float32) * sc.to(torch.float32) + sh.to(torch.float32)
        d = torch.where(p32 > 0, torch.tensor(1.0, dtype=torch.float64), torch.tensor(ALPHA, dtype=torch.float64))
    elif act == 'sigmoid':
        d = y * (1 - y)
    elif act == 'tanh':
        d = 1 - y * y
    else:
        d = torch.ones_like(x)
    gd = dy * d
    dx = gd if sc is None else gd * sc
    return dx, (gd * x).sum(0), gd.sum(0)


def bn_finalize_ref(s, q, count, gamma, beta, mm, mv, training=True, update=True, unbiased=False, eps=EPS, mom=MOM):
    """(scale, shift, mean, rstd, moving_mean, moving_var) of Keras BatchNormalization from the column sums s and sums of squares q."""
    C = (s if training else mm).numel()
    g = torch.ones(C, dtype=torch.float64) if gamma is None else gamma
    b = torch.zeros(C, dtype=torch.float64) if beta is None else beta
    if training:
        mean = s / count
        var = (q / count - mean * mean).clamp(min=0.0)
        if update:
            vm = var * count / (count - 1) if (unbiased and count > 1) else var
            mm, mv = mm * mom + mean * (1 - mom), mv * mom + vm * (1 - mom)
    else:
        mean, var = mm, mv
    rstd = 1 / torch.sqrt(var + eps)
    return g * rstd, b - mean * g * rstd, mean, rstd, mm, mv


def bn_bwd_coefs_ref(dscale, dshift, mean, rstd, gamma, count):
    """BatchNorm(z) = scale z + shift with scale = gamma rstd, shift = beta - mean scale, rstd = (var + eps)^-1/2.  Given dL/dscale and
    dL/dshift: (dgamma, dbeta, c0, c2) with dL/dz += c0 + c2 z, from dmean/dz = 1/N and dvar/dz = 2 (z - mean) / N."""
    g = torch.ones_like(mean) if gamma is None else gamma
    dsc = dscale - mean * dshift                       # dL/d(scale) in total: shift holds -mean scale
    dL_dmean = -dshift * g * rstd
    dL_dvar = dsc * g * (-0.5 * rstd ** 3)
    c2 = 2 * dL_dvar / count
    return dsc * rstd, dshift.clone(), dL_dmean / count - c2 * mean, c2


def adam_ref(p, g, m, v, t, lr, b1, b2, eps):
    """One Keras-2.2 Adam step in float64, out of place: (p, m, v)."""
    lr_t = lr * math.sqrt(1.0 - b2 ** t) / (1.0 - b1 ** t)
    m = b1 * m + (1 - b1) * g
    v = b2 * v + (1 - b2) * g * g
    return p - lr_t * m / (torch.sqrt(v) + eps), m, v


def f32(x):
    return float(np.float32(x))


def optimiser_hypers():
    """(name, lr, b1, b2, eps) as optimizertts.py and optimizertts_wgan.py hand them to KerasAdam, read from their default options."""
    from percivaltts_amd import optimizertts, optimizertts_wgan
    cfg = types.SimpleNamespace()
    optimizertts.OptimizerTTS.default_options(None, cfg)
    optimizertts_wgan.OptimizerTTSWGAN.default_options(None, cfg)
    return [('lse', 10 ** cfg.train_lse_learningrate_log10, cfg.train_lse_adam_beta1, cfg.train_lse_adam_beta2, 10 ** cfg.train_lse_adam_epsilon_log10),
            ('critic', 10 ** cfg.train_wgan_critic_learningrate_log10, cfg.train_wgan_critic_adam_beta1, cfg.train_wgan_critic_adam_beta2, 1e-7),
            ('generator', 10 ** cfg.train_wgan_gen_learningrate_log10, cfg.train_wgan_gen_adam_beta1, cfg.train_wgan_gen_adam_beta2, 1e-7)]


# (rows, C, element offset of x / mask_src / dy): the sweep of the docstring
COL_CASES = [
    (1, 4, 0), (255, 4, 0), (3073, 4, 0), (262144 + 77, 4, 0), (1048576 + 77, 4, 0),
    (1, 8, 0), (37, 8, 0), (1000, 8, 0),
    (1, 12, 0), (84, 12, 0), (681, 12, 0),
    (3, 256, 0), (33, 256, 0),
    (1, 260, 0), (2, 260, 0), (61, 260, 0),
    (1, 1024, 0), (9, 1024, 0),
    (1, 1, 0), (700, 1, 0), (1, 3, 0), (174080 + 5, 3, 0), (1, 86, 0), (40, 86, 0), (1, 255, 0), (9, 255, 0),
    (1, 8, 1), (37, 8, 1), (1000, 8, 1), (3, 256, 1), (33, 256, 1),
    (1, 257, 0), (5, 257, 0), (3, 1028, 0), (2, 2047, 0), (1, 2048, 0), (5, 2048, 0),
    (3, 2049, 0),
]
GP_SHAPES = [(1, 1), (3, 63), (70, 7), (300, 5), (2, 1023), (2, 1025), (2, 70001)]
LOSS_N = [1, 255, 257, 4097, 1048576 + 333, 2097152 + 333]
WLSE_SHAPES = [(n, 1) for n in LOSS_N] + [(37, 7), (3, 86), (48, 86), (149797 + 48, 7), (299593 + 48, 7), (12193 + 4, 86), (24386 + 4, 86)]
ADAM_N = [1, 255, 10007, 2097152 + 1027]
GATED_N = [1, 3, 4, 5, 1023, 4194304 + 1030]


# ---------------------------------------------------------------------------------------------------------------------------
# CPU
# ---------------------------------------------------------------------------------------------------------------------------
def _lib():
    from percivaltts_amd import _hip
    if not os.path.exists(_hip.LIB_PATH):
        pytest.skip('libpercival_hip.so not built (run __graft_entry__.build())')
    return _hip.lib(), _hip


def test_act_bwd_reference_matches_autograd():
    g = gen(1)
    x, dy = randn32(g, 9, 5), randn32(g, 9, 5)
    sc, sh = r32(rand32(g, 5) + 0.5), randn32(g, 5)
    for act in ACTS:
        for affine in (True, False):
            xs = [t.clone().requires_grad_(True) for t in ((x, sc, sh) if affine else (x,))]
            y = act_fwd_ref(xs[0], xs[1] if affine else None, xs[2] if affine else None, act)
            y.backward(dy)
            dx, dscale, dshift = act_bwd_ref(dy, x, y.detach(), sc if affine else None, sh if affine else None, act)
            torch.testing.assert_close(dx, xs[0].grad, rtol=1e-13, atol=1e-13)
            if affine:
                torch.testing.assert_close(dscale, xs[1].grad, rtol=1e-13, atol=1e-13)
                torch.testing.assert_close(dshift, xs[2].grad, rtol=1e-13, atol=1e-13)


@pytest.mark.parametrize('with_gamma', [True, False])
def test_bn_references_match_autograd_and_the_oracle(with_gamma):
    """bn_finalize_ref against oracle.BN (values and moving statistics); bn_bwd_coefs_ref + the pass dz = dz_through + c2 z + c0
    (what ptts_axpby_cols adds) against autograd through the oracle's BatchNorm."""
    g = gen(2)
    N, C = 13, 6
    z = torch.randn(N, C, generator=g, dtype=torch.float64) * 1.5 + 0.4
    w = torch.randn(N, C, generator=g, dtype=torch.float64)
    gamma = (torch.rand(C, generator=g, dtype=torch.float64) + 0.5) if with_gamma else torch.ones(C, dtype=torch.float64)
    beta = torch.randn(C, generator=g, dtype=torch.float64)
    for unbiased in (False, True):
        mm, mv = torch.full((C,), 0.25, dtype=torch.float64), torch.full((C,), 1.5, dtype=torch.float64)
        zr, gr, br = (t.clone().requires_grad_(True) for t in (z, gamma, beta))
        bn = O.BN(gr, br, mm.clone(), mv.clone())
        y = bn(zr, True, update=True, unbiased_moving=unbiased)
        (y * w).sum().backward()
        scale, shift, mean, rstd, mm2, mv2 = bn_finalize_ref(z.sum(0), (z * z).sum(0), N, gamma if with_gamma else None, beta, mm, mv, True, True, unbiased)
        torch.testing.assert_close(scale * z + shift, y.detach(), rtol=1e-12, atol=1e-12)
        torch.testing.assert_close(mm2, bn.mm, rtol=1e-13, atol=1e-13)
        torch.testing.assert_close(mv2, bn.mv, rtol=1e-13, atol=1e-13)
        dgamma, dbeta, c0, c2 = bn_bwd_coefs_ref((w * z).sum(0), w.sum(0), mean, rstd, gamma if with_gamma else None, N)
        torch.testing.assert_close(w * scale + c2 * z + c0, zr.grad, rtol=1e-11, atol=1e-11)
        torch.testing.assert_close(dgamma, gr.grad, rtol=1e-11, atol=1e-11)
        torch.testing.assert_close(dbeta, br.grad, rtol=1e-11, atol=1e-11)
    # count = 1: the unbiased factor count / (count - 1) is not applied
    one = bn_finalize_ref(z[0], z[0] * z[0], 1, None, None, mm, mv, True, True, True)
    assert bool(torch.isfinite(torch.stack(one)).all())
    torch.testing.assert_close(one[5], mv * MOM, rtol=1e-13, atol=1e-13)


def test_adam_reference_matches_the_oracle():
    g = gen(3)
    p, gr = torch.randn(17, generator=g, dtype=torch.float64), torch.randn(17, generator=g, dtype=torch.float64)
    m, v = torch.randn(17, generator=g, dtype=torch.float64) * 0.1, torch.rand(17, generator=g, dtype=torch.float64) * 0.01
    for _, lr, b1, b2, eps in optimiser_hypers():
        for t in (1, 2, 10000):
            po, mo, vo = p.clone(), m.clone(), v.clone()
            O.adam_keras([po], [gr], [mo], [vo], t, lr, b1, b2, eps)
            pr, mr, vr = adam_ref(p, gr, m, v, t, lr, b1, b2, eps)
            for a, b in ((pr, po), (mr, mo), (vr, vo)):
                torch.testing.assert_close(a, b, rtol=1e-14, atol=1e-16)


def test_optimiser_hyper_parameters_are_read_from_the_optimisers():
    h = {name: rest for name, *rest in optimiser_hypers()}
    assert h['lse'][1:] == [0.9, 0.999, 1e-8] and abs(h['lse'][0] - 4e-4) < 1e-9
    assert h['critic'] == [1e-4, 0.5, 0.9, 1e-7] and h['generator'] == [1e-3, 0.5, 0.9, 1e-7]


def test_colstats_workspace_size():
    """At least one row of 2 C doubles for every (rows, C) of this file and never less for more rows (a caller may size one buffer
    for its largest map); 0 for C <= 0; less than one row, or a NULL workspace, is PTTS_EWORKSPACE.  (The GPU tests hand every
    reduction exactly this many bytes between two sentinel margins.)"""
    lib, _hip = _lib()
    p = ctypes.c_void_p(256)
    ladder = sorted({r + d for r, _, _ in COL_CASES for d in (-1, 0, 1) if r + d > 0} |
                    {k * 2 ** s + d for s in range(0, 23) for k in (1, 3) for d in (-1, 0, 1, 77) if k * 2 ** s + d > 0})
    for C in sorted({c for _, c, _ in COL_CASES} | {16, 64, 128, 512, 4096}):
        last = 0
        for rows in ladder:
            if rows * C > 1 << 33:
                break
            need = lib.ptts_colstats_workspace_bytes(rows, C)
            assert need >= 2 * C * 8 and need % (2 * C * 8) == 0, (rows, C, need)
            assert need >= last, 'workspace shrinks from {} to {} bytes at rows = {}, C = {}'.format(last, need, rows, C)
            last = need
    for C in (0, -4, -1):
        assert lib.ptts_colstats_workspace_bytes(100, C) == 0
    for rows, C, _ in COL_CASES:
        need = lib.ptts_colstats_workspace_bytes(rows, C)
        for ptr_ in (p, ctypes.c_void_p(260)):         # aligned (vectorised where C allows) and the fallback
            # (only sizes below one row of 2 C doubles and a NULL workspace: anything a kernel could accept would be launched)
            assert lib.ptts_colstats(ptr_, rows, C, IN_NONE, None, None, None, ALPHA, p, None, need, None) == EWORKSPACE
            assert 'workspace' in _hip.last_error()
            assert lib.ptts_colstats(ptr_, rows, C, IN_NONE, None, None, None, ALPHA, p, p, 2 * C * 8 - 1, None) == EWORKSPACE
            assert lib.ptts_affine_act_bwd(ptr_, p, p, None, None, p, p, p, 2 * C * 8 - 1, rows, C, 0, ALPHA, None) == EWORKSPACE
            assert 'workspace' in _hip.last_error()


def test_elementwise_entry_points_reject_bad_arguments():
    """PTTS_EINVAL (-1) with a message in ptts_last_error for NULL pointers, rows <= 0, scale without shift, B > 65535, lo > hi, an
    unsupported or unaligned ptts_bn_batch_stats input, unaligned gated-product operands; PTTS_EWORKSPACE (-3) for a short or NULL
    workspace.  All are returned before any launch (no pointer is dereferenced on the host), so no GPU is needed."""
    lib, _hip = _lib()
    p, u = ctypes.c_void_p(256), ctypes.c_void_p(260)
    big = 1 << 40

    def refused(rc, word, code=EINVAL):
        assert rc == code, (rc, _hip.last_error())
        assert word in _hip.last_error(), _hip.last_error()

    # ptts_colstats / ptts_affine_act_bwd
    refused(lib.ptts_colstats(None, 5, 4, 0, None, None, None, ALPHA, p, p, big, None), 'null')
    refused(lib.ptts_colstats(p, 5, 4, 0, None, None, None, ALPHA, None, p, big, None), 'null')
    for C, ptr_ in ((4, p), (4, u), (3, p), (2049, p)):
        for rows in (0, -3):
            refused(lib.ptts_colstats(ptr_, rows, C, 0, None, None, None, ALPHA, p, p, big, None), 'rows')
            refused(lib.ptts_affine_act_bwd(ptr_, p, p, None, None, p, p, p, big, rows, C, 0, ALPHA, None), 'bad args')
    for ptr_ in (p, u):
        for C in (0, -4):
            refused(lib.ptts_colstats(ptr_, 5, C, 0, None, None, None, ALPHA, p, p, big, None), 'C={}'.format(C))
    refused(lib.ptts_colstats(p, 5, 4, 1, p, None, None, ALPHA, p, p, big, None), 'together')
    refused(lib.ptts_colstats(p, 5, 4, 1, None, p, None, ALPHA, p, p, big, None), 'together')
    refused(lib.ptts_affine_act_bwd(p, p, p, p, None, p, p, p, big, 5, 4, 1, ALPHA, None), 'together')
    refused(lib.ptts_affine_act_bwd(None, p, p, None, None, p, p, p, big, 5, 4, 1, ALPHA, None), 'bad args')
    refused(lib.ptts_affine_act_bwd(p, p, None, None, None, p, p, p, big, 5, 4, 2, ALPHA, None), 'need y')
    refused(lib.ptts_affine_act_bwd(p, p, None, None, None, p, p, p, big, 5, 4, 3, ALPHA, None), 'need y')
    refused(lib.ptts_affine_act_bwd(p, p, p, None, None, p, None, p, big, 5, 4, 0, ALPHA, None), 'dsums')
    refused(lib.ptts_colstats(p, 5, 4, 0, None, None, None, ALPHA, p, None, big, None), 'workspace', EWORKSPACE)
    # ptts_affine_act / ptts_axpby_cols
    refused(lib.ptts_affine_act(None, None, None, p, 5, 4, 0, ALPHA, None), 'bad args')
    refused(lib.ptts_affine_act(p, None, None, None, 5, 4, 0, ALPHA, None), 'bad args')
    refused(lib.ptts_affine_act(p, None, None, p, 0, 4, 0, ALPHA, None), 'bad args')
    refused(lib.ptts_affine_act(p, None, None, p, 5, 0, 0, ALPHA, None), 'bad args')
    refused(lib.ptts_affine_act(p, p, None, p, 5, 4, 0, ALPHA, None), 'together')
    refused(lib.ptts_affine_act(p, None, p, p, 5, 4, 0, ALPHA, None), 'together')
    refused(lib.ptts_axpby_cols(p, None, p, None, None, None, 5, 4, None), 'bad args')
    refused(lib.ptts_axpby_cols(p, None, p, None, None, p, 0, 4, None), 'bad args')
    refused(lib.ptts_axpby_cols(p, None, p, None, None, p, 5, 0, None), 'bad args')
    # BatchNorm finalisers
    refused(lib.ptts_bn_finalize(p, 5, None, None, p, p, EPS, MOM, 1, 1, 0, 4, None, p, None, None, None), 'null output')
    refused(lib.ptts_bn_finalize(p, 5, None, None, p, p, EPS, MOM, 1, 1, 0, 0, p, p, None, None, None), 'null output')
    refused(lib.ptts_bn_finalize(None, 5, None, None, p, p, EPS, MOM, 1, 1, 0, 4, p, p, None, None, None), 'needs sums')
    refused(lib.ptts_bn_finalize(None, 5, None, None, None, p, EPS, MOM, 0, 0, 0, 4, p, p, None, None, None), 'moving')
    refused(lib.ptts_bn_finalize(p, 5, None, None, p, None, EPS, MOM, 1, 1, 0, 4, p, p, None, None, None), 'moving')
    refused(lib.ptts_bn_finalize_partials(None, 3, 5, 4, None, None, p, p, EPS, MOM, 1, 0, p, p, None, None, None), 'bad args')
    refused(lib.ptts_bn_finalize_partials(p, 0, 5, 4, None, None, p, p, EPS, MOM, 1, 0, p, p, None, None, None), 'bad args')
    refused(lib.ptts_bn_finalize_partials(p, 3, 0, 4, None, None, p, p, EPS, MOM, 1, 0, p, p, None, None, None), 'bad args')
    refused(lib.ptts_bn_finalize_partials(p, 3, 5, 0, None, None, p, p, EPS, MOM, 1, 0, p, p, None, None, None), 'C = 0')
    refused(lib.ptts_bn_finalize_partials(p, 3, 5, 4, None, None, None, p, EPS, MOM, 1, 0, p, p, None, None, None), 'moving')
    refused(lib.ptts_partial_rows_sum(None, 3, 4, p, None), 'bad args')
    refused(lib.ptts_partial_rows_sum(p, 3, 0, p, None), 'bad args')
    for C in (3, 12, 32, 0):
        assert lib.ptts_bn_batch_stats_supported(100, C) == 0
        refused(lib.ptts_bn_batch_stats(p, 100, C, None, None, p, p, EPS, MOM, 1, 0, p, p, None, None, p, big, p, None), 'unsupported')
    for C in (4, 8, 16):
        assert lib.ptts_bn_batch_stats_supported(100, C) == 1 and lib.ptts_bn_batch_stats_supported(0, C) == 0
        refused(lib.ptts_bn_batch_stats(u, 100, C, None, None, p, p, EPS, MOM, 1, 0, p, p, None, None, p, big, p, None), 'aligned')
        refused(lib.ptts_bn_batch_stats(p, 0, C, None, None, p, p, EPS, MOM, 1, 0, p, p, None, None, p, big, p, None), 'unsupported')
        refused(lib.ptts_bn_batch_stats(p, 100, C, None, None, p, p, EPS, MOM, 1, 0, p, p, None, None, p, big, None, None), 'null')
        refused(lib.ptts_bn_batch_stats(p, 100, C, None, None, None, p, EPS, MOM, 1, 0, p, p, None, None, p, big, p, None), 'moving')
        refused(lib.ptts_bn_batch_stats(p, 100, C, None, None, p, p, EPS, MOM, 1, 0, p, p, None, None, p, 2 * C * 8 - 1, p, None), 'workspace', EWORKSPACE)
        refused(lib.ptts_bn_batch_stats(p, 100, C, None, None, p, p, EPS, MOM, 1, 0, p, p, None, None, None, big, p, None), 'workspace', EWORKSPACE)
    for fn in (lib.ptts_bn_bwd_coefs, lib.ptts_bn_bwd_coefs_acc):
        for null in (0, 1, 2, 3, 9, 10):               # dscale, dshift, mean, rstd, c0, c2
            args = [p, p, p, p, None, 5, 4, None, None, p, p, None]
            args[null] = None
            refused(fn(*args), 'bad args')
        refused(fn(p, p, p, p, None, 0, 4, None, None, p, p, None), 'bad args')
        refused(fn(p, p, p, p, None, 5, 0, None, None, p, p, None), 'bad args')
    # WGAN-GP, losses
    for B in (0, 65536):
        refused(lib.ptts_gp_interpolate(p, p, p, p, B, 7, None), 'bad args')
        refused(lib.ptts_gp_scale_rows(p, p, None, p, B, 7, None), 'bad args')
    refused(lib.ptts_gp_interpolate(p, p, None, p, 2, 7, None), 'bad args')
    refused(lib.ptts_gp_interpolate(p, p, p, p, 2, 0, None), 'bad args')
    refused(lib.ptts_gp_scale_rows(p, None, None, p, 2, 7, None), 'bad args')
    refused(lib.ptts_gp_sqnorm(p, None, 2, 7, None), 'bad args')
    refused(lib.ptts_gp_sqnorm(p, p, 0, 7, None), 'bad args')
    refused(lib.ptts_gp_penalty(None, p, p, 2, None), 'bad args')
    refused(lib.ptts_gp_penalty(p, p, p, 0, None), 'bad args')
    refused(lib.ptts_mean_scaled(None, 5, 1.0, p, None), 'bad args')
    refused(lib.ptts_mean_scaled(p, 0, 1.0, p, None), 'bad args')
    refused(lib.ptts_wlse_fwd(p, None, None, p, 5, 4, None), 'bad args')
    refused(lib.ptts_wlse_fwd(p, p, None, p, 0, 4, None), 'bad args')
    refused(lib.ptts_wlse_fwd(p, p, None, p, 5, 0, None), 'bad args')
    refused(lib.ptts_wlse_bwd(p, p, None, None, None, 5, 4, None), 'bad args')
    refused(lib.ptts_wlse_bwd(p, p, None, None, p, 0, 4, None), 'bad args')
    # Adam, clip, gated product
    refused(lib.ptts_weight_clip(p, 5, 0.5, -0.5, None), 'bad args')
    refused(lib.ptts_weight_clip(None, 5, -0.5, 0.5, None), 'bad args')
    refused(lib.ptts_weight_clip(p, 0, -0.5, 0.5, None), 'bad args')
    for null in (0, 1, 2, 3, 10):
        args = [p, p, p, p, 5, 1e-3, 0.5, 0.9, 1e-7, 1.0, p, None]
        args[null] = None
        refused(lib.ptts_adam_keras_step(*args), 'bad args')
    refused(lib.ptts_adam_keras_step(p, p, p, p, 0, 1e-3, 0.5, 0.9, 1e-7, 1.0, p, None), 'bad args')
    refused(lib.ptts_gated_mul_fwd(p, p, p, 0, None), 'bad args')
    refused(lib.ptts_gated_mul_fwd(p, None, p, 5, None), 'bad args')
    refused(lib.ptts_gated_mul_bwd(p, p, p, p, None, 5, None), 'bad args')
    for k in range(3):
        refused(lib.ptts_gated_mul_fwd(*([u if i == k else p for i in range(3)] + [5, None])), 'aligned')
    for k in range(5):
        refused(lib.ptts_gated_mul_bwd(*([u if i == k else p for i in range(5)] + [5, None])), 'aligned')


# ---------------------------------------------------------------------------------------------------------------------------
# GPU helpers
# ---------------------------------------------------------------------------------------------------------------------------
PAD = 64
SENTINEL = {torch.float32: 12345.0, torch.float64: 12345.0, torch.int32: 12345, torch.uint8: 165}


class Guard(object):
    """n elements (`.t`, NaN-filled, zero for integers) at `off` elements past a 256-byte boundary, with PAD elements (uint8: 4 PAD)
    of sentinel on either side; intact() compares the margins."""
    def __init__(self, n, dtype=torch.float32, off=0, shape=None):
        pad = PAD * (4 if dtype == torch.uint8 else 1)
        self.n, self.lo, self.s = int(n), pad + off, SENTINEL[dtype]
        self.buf = torch.full((self.n + 2 * pad + off,), self.s, dtype=dtype, device='cuda')
        self.t = self.buf[self.lo:self.lo + self.n]
        self.t.fill_(float('nan') if dtype.is_floating_point else 0)
        if shape is not None:
            self.t = self.t.view(shape)
        assert self.t.data_ptr() % 16 == (off * self.buf.element_size()) % 16

    def intact(self, what):
        torch.cuda.synchronize()
        assert bool((self.buf[:self.lo] == self.s).all()), '{}: written in front of the buffer'.format(what)
        assert bool((self.buf[self.lo + self.n:] == self.s).all()), '{}: written behind the buffer'.format(what)


def intact(what, *guards):
    for k, g_ in enumerate(guards):
        g_.intact('{} (buffer {})'.format(what, k))


def dev(t, off=0):
    """A contiguous float32 device copy whose first element lies `off` elements past a 512-byte boundary."""
    if t is None:
        return None
    t = t.detach().to(torch.float32)
    flat = torch.empty(t.numel() + off, dtype=torch.float32, device='cuda')
    v = flat[off:].view(t.shape)
    v.copy_(t)
    assert v.is_contiguous() and v.data_ptr() % 16 == (4 * off) % 16
    return v


def check(got, want, tol, what, finite=True):
    """|got - want| <= bound elementwise; the bound is (rtol, atol) -> atol + rtol |want|, or a tensor.  Prints the worst error / bound
    ratio before it asserts."""
    got = got.detach().cpu().to(torch.float64).reshape(-1)
    want = want.detach().cpu().to(torch.float64).reshape(-1)
    assert got.shape == want.shape, '{}: {} values for {}'.format(what, got.numel(), want.numel())
    if finite:
        assert bool(torch.isfinite(got).all()), '{}: not finite'.format(what)
    bound = tol[1] + tol[0] * want.abs() if isinstance(tol, tuple) else tol.detach().to(torch.float64).reshape(-1)
    err = (got - want).abs()
    ratio = torch.where(err == 0, torch.zeros_like(err), err / bound.clamp(min=1e-300))
    i = int(torch.argmax(ratio))
    print('ew-ratio {} {:.4f}'.format(what, float(ratio[i])))
    assert float(ratio[i]) <= 1.0, '{}: {} / {} off, worst err {:.3e} = {:.2f} x bound at {} (got {:.9e} want {:.9e})'.format(
        what, int((ratio > 1.0).sum()), err.numel(), float(err[i]), float(ratio[i]), i, float(got[i]), float(want[i]))
    return float(ratio[i])


def _api():
    from percivaltts_amd import _hip, ops
    return ops, _hip.call, _hip.ptr, _hip.stream, _hip.lib()


def _workspace(lib, rows, C):
    return Guard(lib.ptts_colstats_workspace_bytes(rows, C), torch.uint8)


# ---------------------------------------------------------------------------------------------------------------------------
# 1. column reductions
# ---------------------------------------------------------------------------------------------------------------------------
def _col_inputs(rows, C):
    g = gen(1000 + C)
    x, m, dy = (randn32(g, rows, C) for _ in range(3))
    return x, m, dy, r32(rand32(g, C) + 0.5), r32(torch.randn(C, generator=g, dtype=torch.float64) * 0.3)


@pytest.mark.gpu
@pytest.mark.parametrize('case', COL_CASES, ids=lambda c: '{}x{}{}'.format(c[0], c[1], '+1' if c[2] else ''))
def test_colsums_every_path(case):
    """ptts_colstats in its three input modes (IN_LRELU with and without the affine) on the path the docstring names for this case;
    ops.colsums returns the same bits."""
    ops, call, P, S, lib = _api()
    rows, C, off = case
    x, m, _, sc, sh = _col_inputs(rows, C)
    xd, md, scd, shd = dev(x, off), dev(m, off), dev(sc), dev(sh)
    pre = x.to(torch.float32) * sc.to(torch.float32) + sh.to(torch.float32)            # the kernel's float32 pre-activation
    variants = [('none', IN_NONE, None, None, None, x),
                ('lrelu-affine', IN_LRELU, scd, shd, None, lrelu64(x * sc + sh, pre)),
                ('lrelu', IN_LRELU, None, None, None, lrelu64(x)),
                ('maskmul', IN_MASKMUL, None, None, md, x * torch.where(m > 0, 1.0, ALPHA))]
    for name, mode, s_, h_, m_, want in variants:
        sums, ws = Guard(2 * C, torch.float64), _workspace(lib, rows, C)
        call('ptts_colstats', P(xd), rows, C, mode, P(s_), P(h_), P(m_), ALPHA, P(sums.t), P(ws.t), ws.n, S())
        tag = 'colstats {} {}'.format(name, case)
        intact(tag, sums, ws)
        check(sums.t[:C], want.sum(0), SUM_TOL, tag + ' sum')
        check(sums.t[C:], (want * want).sum(0), SUM_TOL, tag + ' sumsq')
        kw = dict(scale=s_, shift=h_, mask_src=m_)
        assert torch.equal(ops.colsums(xd, mode=mode, alpha=ALPHA, **kw), sums.t), tag + ': ops.colsums differs'


@pytest.mark.gpu
@pytest.mark.parametrize('case', COL_CASES, ids=lambda c: '{}x{}{}'.format(c[0], c[1], '+1' if c[2] else ''))
def test_affine_act_backward_every_path(case):
    """ptts_affine_act_bwd (dx and the fp64 dscale / dshift sums in one pass) for the four activations with and without the affine,
    and the backward of ops.affine_act, on the reduction path of this case."""
    ops, call, P, S, lib = _api()
    rows, C, off = case
    x, _, dy, sc, sh = _col_inputs(rows, C)
    xd, dyd, scd, shd = dev(x, off), dev(dy, off), dev(sc), dev(sh)
    big = rows * C > 2000000                               # (the path does not depend on the activation: two of the eight variants)
    for act, code in ACTS.items():
        for affine in (True, False):
            if big and (act, affine) not in (('lrelu', True), ('tanh', False)):
                continue
            y = r32(act_fwd_ref(x, sc if affine else None, sh if affine else None, act))
            want = act_bwd_ref(dy, x, y, sc if affine else None, sh if affine else None, act)
            yd = dev(y, off)
            dx, dsums, ws = Guard(rows * C, off=off), Guard(2 * C, torch.float64), _workspace(lib, rows, C)
            call('ptts_affine_act_bwd', P(dyd), P(xd), P(yd), P(scd if affine else None), P(shd if affine else None), P(dx.t), P(dsums.t),
                 P(ws.t), ws.n, rows, C, code, ALPHA, S())
            tag = 'act_bwd {} {} {}'.format(act, 'affine' if affine else 'plain', case)
            intact(tag, dx, dsums, ws)
            check(dx.t, want[0], (RT, AT), tag + ' dx')
            check(dsums.t[:C], want[1], DSUM_TOL, tag + ' dscale')
            check(dsums.t[C:], want[2], DSUM_TOL, tag + ' dshift')
            # without dx (the reduction alone): the same sums, bit for bit
            dsums2, ws2 = Guard(2 * C, torch.float64), _workspace(lib, rows, C)
            call('ptts_affine_act_bwd', P(dyd), P(xd), P(yd), P(scd if affine else None), P(shd if affine else None), None, P(dsums2.t),
                 P(ws2.t), ws2.n, rows, C, code, ALPHA, S())
            intact(tag + ' no dx', dsums2, ws2)
            assert torch.equal(dsums2.t, dsums.t), tag + ': the sums depend on whether dx is written'
        if big and act != 'lrelu':
            continue
        # the autograd node (leaves that share the storage of the views: an unaligned x stays unaligned)
        xg, sg, hg = (t.detach().requires_grad_(True) for t in (xd, scd, shd))
        yop = ops.affine_act(xg, sg, hg, act, ALPHA)
        yop.backward(dyd)
        y = r32(yop.detach().cpu())
        want = act_bwd_ref(dy, x, y, sc, sh, act)
        check(xg.grad, want[0], (RT, AT), 'ops.affine_act {} {} dx'.format(act, case))
        check(sg.grad, want[1], DSUM_TOL, 'ops.affine_act {} {} dscale'.format(act, case))
        check(hg.grad, want[2], DSUM_TOL, 'ops.affine_act {} {} dshift'.format(act, case))


def _bn_conditioning(kind, shape):
    """Inputs (float32-exact), the fp64 statistics, and the error of the oracle's BatchNorm statistics evaluated in plain float32."""
    g = gen(31)
    C = shape[-1]
    rows = int(np.prod(shape[:-1]))
    z = torch.randn(rows, C, generator=g, dtype=torch.float64) * 2 + 0.7
    if kind == 'constant':
        z[:, 1] = 0.7
    else:
        col = torch.randn(rows, generator=g, dtype=torch.float64)
        col = (col - col.mean()) / col.std(unbiased=False)
        z[:, 1] = 0.5 * col + 5.0                        # |mean| / std = 10
    z = r32(z)
    gamma, beta = r32(rand32(g, C) + 0.5), randn32(g, C)

    def stats(x, dt):
        mean, var = x.mean(0), x.var(0, unbiased=False)
        scale = gamma.to(dt) / torch.sqrt(var + EPS)
        return scale, beta.to(dt) - mean * scale, var
    sc64, sh64, var64 = stats(z, torch.float64)
    sc32, sh32, _ = stats(z.to(torch.float32), torch.float32)
    return z.view(shape), gamma, beta, sc64, sh64, var64, float((sc32.double() - sc64).abs().max()), float((sh32.double() - sh64).abs().max())


@pytest.mark.gpu
@pytest.mark.parametrize('shape', [(2, 25, 37, 4), (1850, 86), (1850, 260)], ids=['fused-C4', 'scalar-C86', 'vec4-C260'])
@pytest.mark.parametrize('kind', ['constant', 'mean10std'])
def test_batchnorm_affine_conditioning(kind, shape):
    """ops.batchnorm_affine in training mode on a map one of whose channels is constant (0.7: var = 0, scale = gamma / sqrt(eps)) or has
    |mean| / std = 10 (mean 5, std 0.5), on its three statistics paths (ptts_bn_batch_stats; ptts_colstats scalar and vectorised +
    ptts_bn_finalize).  var = E[x^2] - mean^2 from fp64 sums.

    The bound is measured, not fixed: 4 x the largest error over the channels of the oracle's formula evaluated in plain float32
    (torch's two-pass mean / var) against float64, for scale and for shift separately -- the kernel must be no worse than naive
    float32, with room for the order of the additions.  Measured on the MI355X, 1850 rows (fp32-oracle error, x 4 = bound, kernel
    error; `ew-cond` lines of the output):
        constant   fused-C4    scale 1.636e-06  6.544e-06  2.713e-07   shift 4.429e-06  1.772e-05  6.146e-07
        constant   scalar-C86  scale 1.077e-06  4.307e-06  1.077e-06   shift 3.101e-06  1.240e-05  2.398e-07
        constant   vec4-C260   scale 1.872e-06  7.489e-06  3.508e-08   shift 3.781e-06  1.512e-05  1.123e-07
        mean10std  fused-C4    scale 7.914e-08  3.165e-07  4.007e-08   shift 8.161e-08  3.264e-07  8.161e-08
        mean10std  scalar-C86  scale 2.288e-07  9.152e-07  2.948e-08   shift 6.749e-07  2.699e-06  2.788e-07
        mean10std  vec4-C260   scale 7.381e-08  2.952e-07  7.381e-08   shift 6.210e-07  2.484e-06  3.326e-07
    Before the statistics kernels added exact squares in fp64 (they rounded x*x to float32 and, on the vectorised and one-launch
    paths, added sums and squares in float32 over up to 16 rows first) three cases missed the bound: constant fused-C4 scale 2.262e-05,
    mean10std fused-C4 scale 6.361e-07 / shift 3.419e-06, mean10std vec4-C260 scale 7.891e-07 / shift 4.147e-06.
    var >= 0 is asserted through the moving variance (it starts at 0, so it is (1 - momentum) var) and scale <= gamma / sqrt(eps);
    scale and shift are finite."""
    ops, call, P, S, lib = _api()
    z, gamma, beta, sc64, sh64, var64, e_scale, e_shift = _bn_conditioning(kind, shape)
    C = shape[-1]
    mm, mv = torch.zeros(C, device='cuda'), torch.zeros(C, device='cuda')
    gd = dev(gamma)
    _, scale, shift = ops.batchnorm_affine(dev(z), gd, dev(beta), mm, mv, True, True, False)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(scale).all()) and bool(torch.isfinite(shift).all())
    assert bool((mv >= 0).all()), 'negative variance'
    assert bool((scale.double().cpu() <= gamma / math.sqrt(EPS) * (1 + 2.0 ** -22)).all()), 'scale beyond gamma / sqrt(eps): negative variance'
    k_scale, k_shift = float((scale.double().cpu() - sc64).abs().max()), float((shift.double().cpu() - sh64).abs().max())
    print('ew-cond {} {}: scale fp32-oracle {:.3e} x4 = {:.3e} kernel {:.3e} | shift fp32-oracle {:.3e} x4 = {:.3e} kernel {:.3e}'.format(
        kind, shape, e_scale, 4 * e_scale, k_scale, e_shift, 4 * e_shift, k_shift))
    check(scale, sc64, torch.full((C,), 4 * e_scale, dtype=torch.float64), 'bn conditioning {} {} scale'.format(kind, shape))
    check(shift, sh64, torch.full((C,), 4 * e_shift, dtype=torch.float64), 'bn conditioning {} {} shift'.format(kind, shape))
    check(mv, (1 - MOM) * var64, (1e-5, 1e-8), 'bn conditioning {} {} moving variance'.format(kind, shape))


# ---------------------------------------------------------------------------------------------------------------------------
# 2. final stage and BatchNorm finalisers
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize('ncols', [1, 7, 8, 9, 520])
@pytest.mark.parametrize('nrows', [1, 31, 32, 33, 65])
def test_partial_rows_sum(nrows, ncols):
    """colreduce_final_kernel: 32 row groups (rows g, g + 32, ...), then the groups in index order.  Positive terms, so rtol 1e-15
    against an 80-bit sum is a statement about every addition.  With nrows <= 32 a group holds at most one row and the result is the
    in-order sum, bit for bit; beyond that it is the grouped sum, bit for bit (the library is built without reassociation)."""
    ops, call, P, S, lib = _api()
    part = torch.rand(nrows, ncols, generator=gen(40 + nrows), dtype=torch.float64) + 0.5
    out, pd = Guard(ncols, torch.float64), part.cuda()
    call('ptts_partial_rows_sum', P(pd), nrows, ncols, P(out.t), S())
    intact('partial_rows_sum', out)
    got = out.t.cpu()
    exact = part.numpy().astype(np.longdouble).sum(0)
    ratio = float(np.max(np.abs(got.numpy().astype(np.longdouble) - exact) / (1e-15 * np.abs(exact))))
    print('ew-ratio partial_rows_sum {}x{} {:.4f}'.format(nrows, ncols, ratio))
    assert ratio <= 1.0
    groups = torch.zeros(32, ncols, dtype=torch.float64)
    for r in range(nrows):
        groups[r % 32] += part[r]
    grouped = torch.zeros(ncols, dtype=torch.float64)
    for k in range(32):
        grouped += groups[k]
    assert torch.equal(got, grouped), 'not the grouped fixed-order sum'
    if nrows <= 32:
        inorder = torch.zeros(ncols, dtype=torch.float64)
        for r in range(nrows):
            inorder += part[r]
        assert torch.equal(got, inorder), 'not the in-order sum'


def _finalize_case(C, nrows, count_one=False):
    g = gen(50 + C)
    per = 1 if count_one else 5
    z = torch.randn(nrows * per, C, generator=g, dtype=torch.float64) * 1.5 + 0.4
    zz = z.view(nrows, per, C)
    part = torch.cat([zz.sum(1), (zz * zz).sum(1)], dim=1).contiguous()           # [nrows, 2C]
    return part, nrows * per, r32(rand32(g, C) + 0.5), randn32(g, C), rand32(g, C), r32(rand32(g, C) + 0.5)


@pytest.mark.gpu
@pytest.mark.parametrize('nrows', [1, 33])
@pytest.mark.parametrize('C', [1, 15, 16, 17, 300])
def test_bn_finalize_and_finalize_partials(C, nrows):
    """ptts_bn_finalize_partials (one workgroup for C <= 16, a workgroup per 8 channels beyond) and ptts_bn_finalize on the same sums:
    gamma / beta NULL, moving statistics updated or left alone (and then allowed to be NULL), the unbiased moving variance, count = 1
    with unbiased_moving (no division by count - 1), mean / rstd outputs NULL, inference mode."""
    ops, call, P, S, lib = _api()
    combos = [(True, True, True, False, True), (False, False, True, True, True), (True, False, False, False, True), (False, True, True, True, False),
              (True, True, False, True, False)]
    for count_one in ((False, True) if nrows == 1 else (False,)):
        part, count, gamma, beta, mm, mv = _finalize_case(C, nrows, count_one)
        sums = part.sum(0)
        partd, sumsd, gmd, btd = part.cuda(), sums.cuda(), dev(gamma), dev(beta)
        for with_g, with_b, update, unbiased, with_ms in combos:
            want = bn_finalize_ref(sums[:C], sums[C:], count, gamma if with_g else None, beta if with_b else None, mm, mv, True, update, unbiased, EPS32, MOM32)
            for entry in ('partials', 'sums'):
                outs = [Guard(C) for _ in range(4)]
                mmg, mvg = Guard(C), Guard(C)
                mmg.t.copy_(mm); mvg.t.copy_(mv)
                moving = (mmg.t, mvg.t) if (update or with_ms) else (None, None)
                mean_rstd = (outs[2].t, outs[3].t) if with_ms else (None, None)
                if entry == 'partials':
                    call('ptts_bn_finalize_partials', P(partd), nrows, count, C, P(gmd if with_g else None), P(btd if with_b else None),
                         P(moving[0]), P(moving[1]), EPS, MOM, int(update), int(unbiased), P(outs[0].t), P(outs[1].t), P(mean_rstd[0]), P(mean_rstd[1]), S())
                else:
                    call('ptts_bn_finalize', P(sumsd), count, P(gmd if with_g else None), P(btd if with_b else None),
                         P(moving[0]), P(moving[1]), EPS, MOM, 1, int(update), int(unbiased), C, P(outs[0].t), P(outs[1].t), P(mean_rstd[0]), P(mean_rstd[1]), S())
                tag = 'bn_finalize[{}] C={} nrows={} count={} g{} b{} u{} ub{} ms{}'.format(entry, C, nrows, count, *map(int, (with_g, with_b, update, unbiased, with_ms)))
                intact(tag, mmg, mvg, *outs)
                names = ('scale', 'shift', 'mean', 'rstd') if with_ms else ('scale', 'shift')
                for name, o, w in zip(names, outs, want):
                    check(o.t, w, F64_TOL, tag + ' ' + name)
                if not with_ms:
                    assert bool(torch.isnan(outs[2].t).all()) and bool(torch.isnan(outs[3].t).all()), tag + ': a NULL output was written'
                check(mmg.t, want[4], F64_TOL, tag + ' moving_mean')
                check(mvg.t, want[5], F64_TOL, tag + ' moving_var')
                if not update:
                    assert torch.equal(mmg.t.cpu(), mm.float()) and torch.equal(mvg.t.cpu(), mv.float()), tag + ': moving statistics changed'
    # inference: the affine of the moving statistics, which stay as they are; sums NULL
    part, count, gamma, beta, mm, mv = _finalize_case(C, nrows)
    gmd, btd = dev(gamma), dev(beta)
    for with_gb in (True, False):
        want = bn_finalize_ref(None, None, 1, gamma if with_gb else None, beta if with_gb else None, mm, mv, training=False, eps=EPS32, mom=MOM32)
        scale, shift, mmg, mvg = Guard(C), Guard(C), Guard(C), Guard(C)
        mmg.t.copy_(mm); mvg.t.copy_(mv)
        call('ptts_bn_finalize', None, 1, P(gmd if with_gb else None), P(btd if with_gb else None), P(mmg.t), P(mvg.t), EPS, MOM, 0, 0, 0, C,
             P(scale.t), P(shift.t), None, None, S())
        intact('bn_finalize inference', scale, shift, mmg, mvg)
        check(scale.t, want[0], F64_TOL, 'bn_finalize inference C={} scale'.format(C))
        check(shift.t, want[1], F64_TOL, 'bn_finalize inference C={} shift'.format(C))
        assert torch.equal(mmg.t.cpu(), mm.float()) and torch.equal(mvg.t.cpu(), mv.float())


def _batch_stats_rows(C):
    R = 256 // (C // 4)
    return [1, 700, 256 * R * 4 + 77]


@pytest.mark.gpu
@pytest.mark.parametrize('case', [(C, k) for C in (4, 8, 16) for k in range(3)] + [(4, 3)],
                         ids=lambda c: 'C{}-{}'.format(c[0], ('one-row', 'one-workgroup', 'cap-256', 'five-sweeps')[c[1]]))
def test_bn_batch_stats_every_path(case):
    """ptts_bn_batch_stats (bn_stats_fused_kernel) at C = 4, 8, 16 with one workgroup (rows = 1, 700), past the cap of 256 workgroups
    (rows = 256 R VU + 77: the three-launch path runs 257 there) and, at C = 4, with 1048576 + 77 rows: workgroup 0 makes five sweeps
    and the others four.

    Twice back to back on one counter: the same bits, the counter zero after each.  Against ptts_colstats + ptts_bn_finalize:
    tests/test_ops_gpu.py::test_bn_batch_stats_one_launch_equals_the_three_launch_path states agreement to fp32 rounding (rtol 2e-6 /
    atol 1e-6: 'the two reduction trees differ in the last bits of the fp64 sums') and that holds at every case here.  Where the two
    paths provably add the same numbers in the same order -- the same number of workgroups (no cap), and either 32 row groups in the
    finish (C = 4) or at most one partial row per group -- the results are equal bit for bit, and that is asserted too.  Past the cap
    the fused kernel's workgroups add other rows together than the 257 workgroups of the three-launch path, so the fp64 sums differ
    in their last bits by construction.  Against fp64 statistics: the existing test's rtol 1e-5 / atol 1e-6, also at
    rows = 1, where var must come out as exactly 0 (scale = gamma / sqrt(eps))."""
    ops, call, P, S, lib = _api()
    C, k = case
    rows = (_batch_stats_rows(C) + [1048576 + 77])[k]
    g = gen(60 + C)
    z = r32(torch.randn(rows, C, generator=g, dtype=torch.float64) * 1.7 + 0.4)
    gamma, beta = r32(rand32(g, C) + 0.5), randn32(g, C)
    zd, gd, bd = dev(z), dev(gamma), dev(beta)
    assert lib.ptts_bn_batch_stats_supported(rows, C) == 1
    cnt = Guard(1, torch.int32)
    runs = []
    for which in ('fused', 'fused', 'three'):
        outs = [Guard(C) for _ in range(6)]            # scale, shift, mean, rstd, moving_mean, moving_var
        outs[4].t.fill_(0.25); outs[5].t.fill_(1.5)
        ws = _workspace(lib, rows, C)
        o = [P(x_.t) for x_ in outs]
        if which == 'fused':
            call('ptts_bn_batch_stats', P(zd), rows, C, P(gd), P(bd), o[4], o[5], EPS, MOM, 1, 1, o[0], o[1], o[2], o[3], P(ws.t), ws.n, P(cnt.t), S())
            intact('bn_batch_stats {}'.format(case), ws, cnt, *outs)
            assert int(cnt.t.item()) == 0, 'the counter is not left at zero'
        else:
            sums = Guard(2 * C, torch.float64)
            call('ptts_colstats', P(zd), rows, C, IN_NONE, None, None, None, ALPHA, P(sums.t), P(ws.t), ws.n, S())
            call('ptts_bn_finalize', P(sums.t), rows, P(gd), P(bd), o[4], o[5], EPS, MOM, 1, 1, 1, C, o[0], o[1], o[2], o[3], S())
            intact('three launches {}'.format(case), ws, sums, *outs)
        runs.append([x_.t.clone() for x_ in outs])
    names = ('scale', 'shift', 'mean', 'rstd', 'moving_mean', 'moving_var')
    for name, a, b in zip(names, runs[0], runs[1]):
        assert torch.equal(a, b), '{}: the second call on the same counter gives other bits'.format(name)
    R = 256 // (C // 4)
    chunks = (rows + 4 * R - 1) // (4 * R)
    same_tree = chunks <= 256 and (C == 4 or chunks <= 256 // (2 * C))
    bits = all(torch.equal(a, b) for a, b in zip(runs[0], runs[2]))
    print('ew-bits bn_batch_stats {} rows={} equal to the three-launch path bit for bit: {} (same tree: {})'.format(case, rows, bits, same_tree))
    if same_tree:
        assert bits, 'the fused launch and the three-launch path add the same numbers in the same order but differ'
    for name, a, b in zip(names, runs[0], runs[2]):
        check(a, b, (2e-6, 1e-6), 'bn_batch_stats {} {} against three launches'.format(case, name))
    want = bn_finalize_ref(z.sum(0), (z * z).sum(0), rows, gamma, beta, torch.full((C,), 0.25, dtype=torch.float64),
                           torch.full((C,), 1.5, dtype=torch.float64), True, True, True, EPS32, MOM32)
    for name, a, w in zip(names, runs[0], want):
        check(a, w, (1e-5, 1e-6), 'bn_batch_stats {} {} against fp64'.format(case, name))
    # an unaligned map is refused with PTTS_EINVAL, nothing written
    from percivaltts_amd._hip import HipLibraryError
    outs = [Guard(C) for _ in range(4)]
    ws = _workspace(lib, rows, C)
    zu = dev(z[:min(rows, 64)], 1)
    with pytest.raises(HipLibraryError, match='aligned'):
        call('ptts_bn_batch_stats', P(zu), zu.shape[0], C, P(gd), P(bd), None, None, EPS, MOM, 0, 0, P(outs[0].t), P(outs[1].t), P(outs[2].t), P(outs[3].t),
             P(ws.t), ws.n, P(cnt.t), S())
    torch.cuda.synchronize()
    assert all(bool(torch.isnan(o_.t).all()) for o_ in outs) and int(cnt.t.item()) == 0


@pytest.mark.gpu
@pytest.mark.parametrize('C', [1, 300])
def test_bn_bwd_coefs_plain_and_accumulating(C):
    """ptts_bn_bwd_coefs and ptts_bn_bwd_coefs_acc against bn_bwd_coefs_ref, with gamma, dgamma and dbeta NULL in turn; the
    accumulating form adds to what the buffers hold (one more float32 rounding: 2^-24 of the sum)."""
    ops, call, P, S, lib = _api()
    g = gen(70 + C)
    dscale, dshift, mean = r32(randn32(g, C) * 3), randn32(g, C), randn32(g, C)
    rstd, gamma = r32(rand32(g, C) + 0.3), r32(rand32(g, C) + 0.5)
    old_g, old_b = randn32(g, C), randn32(g, C)
    count = 1234
    ins = [dev(t) for t in (dscale, dshift, mean, rstd)]
    gmd = dev(gamma)
    for acc in (False, True):
        for with_gamma, with_dg, with_db in ((True, True, True), (False, True, True), (True, False, True), (True, True, False), (False, False, False)):
            want = bn_bwd_coefs_ref(dscale, dshift, mean, rstd, gamma if with_gamma else None, count)
            dg, db, c0, c2 = Guard(C), Guard(C), Guard(C), Guard(C)
            dg.t.copy_(old_g); db.t.copy_(old_b)
            call('ptts_bn_bwd_coefs_acc' if acc else 'ptts_bn_bwd_coefs', *[P(t) for t in ins], P(gmd if with_gamma else None), count, C,
                 P(dg.t if with_dg else None), P(db.t if with_db else None), P(c0.t), P(c2.t), S())
            tag = 'bn_bwd_coefs{} C={} gamma{} dgamma{} dbeta{}'.format('_acc' if acc else '', C, int(with_gamma), int(with_dg), int(with_db))
            intact(tag, dg, db, c0, c2)
            check(c0.t, want[2], F64_TOL, tag + ' c0')
            check(c2.t, want[3], F64_TOL, tag + ' c2')
            wg, wb = (old_g + r32(want[0]), old_b + want[1]) if acc else (want[0], want[1])
            if with_dg:
                check(dg.t, wg, F64_TOL[1] + F64_TOL[0] * want[0].abs() + (2 * U32 * wg.abs() if acc else 0.0), tag + ' dgamma')
            else:
                assert torch.equal(dg.t.cpu(), old_g.float()), tag + ': a buffer that was not handed in was written'
            if with_db:
                check(db.t, wb, F64_TOL[1] + F64_TOL[0] * want[1].abs() + (2 * U32 * wb.abs() if acc else 0.0), tag + ' dbeta')
                if not acc:
                    assert torch.equal(db.t.cpu(), dshift.float()), tag + ': dbeta is not dshift'


@pytest.mark.gpu
@pytest.mark.parametrize('shape', [(37, 3), (5, 260), (699393, 3)], ids=lambda s: '{}x{}'.format(*s))
def test_axpby_cols_null_operands(shape):
    """out = c0[c] + a c1[c] + x c2[c] with every combination of NULL a, x, c1, c2, c0 (c1 only with a, c2 only with x; all NULL
    gives zeros); the last shape has 2097152 + 1027 elements, past the 2048-workgroup cap, with all five operands."""
    ops, call, P, S, lib = _api()
    rows, C = shape
    g = gen(80 + C)
    a, x = randn32(g, rows, C), randn32(g, rows, C)
    c1, c2, c0 = randn32(g, C), randn32(g, C), randn32(g, C)
    ad, xd, c1d, c2d, c0d = (dev(t) for t in (a, x, c1, c2, c0))
    combos = [(ua, ux, u1, u2, u0) for ua in (0, 1) for ux in (0, 1) for u1 in ((0, 1) if ua else (0,)) for u2 in ((0, 1) if ux else (0,)) for u0 in (0, 1)]
    assert len(combos) == 18
    if rows > 1000:
        combos = [(1, 1, 1, 1, 1), (1, 1, 0, 1, 1)]    # all operands; and the BatchNorm backward's own call (c1 NULL)
    for ua, ux, u1, u2, u0 in combos:
        ta = (a * (c1 if u1 else 1.0)) if ua else torch.zeros_like(a)
        tx = (x * (c2 if u2 else 1.0)) if ux else torch.zeros_like(x)
        t0 = (c0 if u0 else torch.zeros_like(c0)).expand(rows, C)
        out = Guard(rows * C)
        call('ptts_axpby_cols', P(ad if ua else None), P(c1d if u1 else None), P(xd if ux else None), P(c2d if u2 else None), P(c0d if u0 else None),
             P(out.t), rows, C, S())
        tag = 'axpby_cols {} a{} c1{} x{} c2{} c0{}'.format(shape, ua, u1, ux, u2, u0)
        intact(tag, out)
        check(out.t, ta + tx + t0, 4 * U32 * (ta.abs() + tx.abs() + t0.abs()), tag)


# ---------------------------------------------------------------------------------------------------------------------------
# 3. WGAN-GP
# ---------------------------------------------------------------------------------------------------------------------------
def _gp_inputs(B, TD, seed=90):
    g = gen(seed + B)
    s = torch.linspace(0.5, 1.5, B, dtype=torch.float64) if B > 1 else torch.tensor([0.8], dtype=torch.float64)
    gg = torch.randn(B, TD, generator=g, dtype=torch.float64)
    gg = gg / gg.norm(dim=1, keepdim=True) * s[:, None]                 # norms from 0.5 to 1.5: both signs of 1 - n
    return r32(gg), randn32(g, B, TD), randn32(g, B, TD), rand32(g, B)


def _gp_reference(gg, up=3.0):
    gr = gg.clone().requires_grad_(True)
    n = torch.sqrt((gr * gr).sum(dim=1))
    pen = ((1 - n) ** 2).mean()
    (up * pen).backward()
    return pen.detach(), gr.grad


def _gp_kernels(gd, B, TD, up):
    """The four launches of ops.grad_penalty with guarded outputs: (penalty, dg)."""
    ops, call, P, S, lib = _api()
    sq, pen, coef, dg = Guard(B), Guard(1), Guard(B), Guard(B * TD)
    upd = dev(torch.tensor([up]))
    call('ptts_gp_sqnorm', P(gd), P(sq.t), B, TD, S())
    call('ptts_gp_penalty', P(sq.t), P(pen.t), P(coef.t), B, S())
    call('ptts_gp_scale_rows', P(gd), P(coef.t), P(upd), P(dg.t), B, TD, S())
    intact('gp kernels {}'.format((B, TD)), sq, pen, coef, dg)
    return pen.t.clone(), dg.t.view(B, TD).clone()


@pytest.mark.gpu
@pytest.mark.parametrize('shape', GP_SHAPES, ids=lambda s: '{}x{}'.format(*s))
def test_grad_penalty_forward_backward(shape):
    ops, call, P, S, lib = _api()
    B, TD = shape
    gg = _gp_inputs(B, TD)[0]
    pen_r, dg_r = _gp_reference(gg)
    gd = dev(gg).requires_grad_(True)
    pd = ops.grad_penalty(gd)
    (3.0 * pd).backward()
    check(pd, pen_r, (RT, AT), 'grad_penalty {} penalty'.format(shape))
    check(gd.grad, dg_r, (RT, AT), 'grad_penalty {} dg'.format(shape))
    pen_k, dg_k = _gp_kernels(gd.detach(), B, TD, 3.0)
    assert torch.equal(pen_k.view(()), pd.detach()) and torch.equal(dg_k, gd.grad), 'the guarded launches differ from ops.grad_penalty'


@pytest.mark.gpu
def test_grad_penalty_zero_gradient_sample():
    """A sample whose gradient is exactly zero: n = 0, (1 - n)^2 = 1 enters the penalty, which stays finite; its coefficient is
    2 (n - 1) / (n B) = -inf and its dg row -inf * 0 = NaN, as the derivative of K.sqrt at 0 makes it in the reference (the
    comment in gp_penalty_kernel).  Every other sample's row matches the oracle."""
    ops, call, P, S, lib = _api()
    B, TD = 5, 63
    gg = _gp_inputs(B, TD)[0]
    gg[2] = 0.0
    pen_r, dg_r = _gp_reference(gg)
    gd = dev(gg).requires_grad_(True)
    pd = ops.grad_penalty(gd)
    (3.0 * pd).backward()
    check(pd, pen_r, (RT, AT), 'grad_penalty zero sample penalty')
    keep = [0, 1, 3, 4]
    check(gd.grad[keep], dg_r[keep], (RT, AT), 'grad_penalty zero sample, other rows')
    assert not bool(torch.isfinite(gd.grad[2]).any()), 'the zero-gradient sample has finite dg'
    pen_k, dg_k = _gp_kernels(gd.detach(), B, TD, 3.0)
    assert torch.equal(pen_k.view(()), pd.detach()) and torch.equal(dg_k[keep], gd.grad[keep])


@pytest.mark.gpu
@pytest.mark.parametrize('shape', GP_SHAPES, ids=lambda s: '{}x{}'.format(*s))
def test_gp_interpolate(shape):
    """alpha real + (1 - alpha) fake per sample; alpha exactly 0 / 1 returns fake / real bit for bit (0 * x + 1 * y in float32, no
    contraction)."""
    ops, call, P, S, lib = _api()
    B, TD = shape
    _, real, fake, al = _gp_inputs(B, TD)
    rd, fd = dev(real), dev(fake)
    for name, a in (('random', al), ('zero', torch.zeros(B, dtype=torch.float64)), ('one', torch.ones(B, dtype=torch.float64)),
                    ('mixed', torch.tensor([float(i % 2) for i in range(B)], dtype=torch.float64))):
        out = Guard(B * TD, shape=(B, TD))
        got = ops.gp_interpolate(rd, fd, dev(a), out=out.t)
        intact('gp_interpolate {} {}'.format(shape, name), out)
        check(got, O.random_weighted_average(real.view(B, TD, 1), fake.view(B, TD, 1), a).view(B, TD), (RT, AT), 'gp_interpolate {} {}'.format(shape, name))
        if name != 'random':
            want = torch.where(a.view(B, 1) == 1, real, fake).float()
            assert torch.equal(got.cpu(), want), 'gp_interpolate {} alpha {}: not a copy'.format(shape, name)


# ---------------------------------------------------------------------------------------------------------------------------
# 4. losses
# ---------------------------------------------------------------------------------------------------------------------------
def _loss_checks(n, sign=-1.0):
    ops, call, P, S, lib = _api()
    v = r32(randn32(gen(100 + n % 1000), n) + 0.3)
    want = O.wasserstein_loss(sign, v)
    vd = dev(v).requires_grad_(True)
    wl = ops.wasserstein(vd, sign)
    (wl * 2).backward()
    check(wl, want, (RT, AT), 'wasserstein n={} sign={}'.format(n, sign))
    check(vd.grad, torch.full((n,), 2 * sign / n, dtype=torch.float64), (RT, AT * min(1.0, 100.0 / n)), 'wasserstein n={} gradient'.format(n))
    out = Guard(1)
    call('ptts_mean_scaled', P(vd.detach()), n, sign, P(out.t), S())
    intact('mean_scaled n={}'.format(n), out)
    check(out.t, want, (RT, AT), 'mean_scaled n={} guarded'.format(n))
    return wl.detach(), vd.detach()


@pytest.mark.gpu
@pytest.mark.parametrize('n', LOSS_N)
def test_wasserstein_loss(n):
    """sign * mean(v): one workgroup (n <= 4096), several, and past the cap of 256 (n > 1048576).  The gradient is sign / n for
    every element; its atol shrinks with 1 / n (AT * 100 / n beyond n = 100), otherwise it would pass a zero gradient."""
    _loss_checks(n, -1.0)
    _loss_checks(n, 1.0)


def _wlse_case(rows, D):
    g = gen(110 + D)
    return randn32(g, rows, D), randn32(g, rows, D), r32(rand32(g, D) + 0.1)


def _wlse_checks(rows, D, weighted):
    ops, call, P, S, lib = _api()
    y, yhat, w = _wlse_case(rows, D)
    n = rows * D
    yh = yhat.clone().requires_grad_(True)
    want = O.specweighted_lse_loss(y, yh, w) if weighted else ((y - yh) ** 2).mean()
    (want * 0.7).backward()
    yd, yhd, wd = dev(y), dev(yhat).requires_grad_(True), dev(w) if weighted else None
    loss = ops.wlse(yhd, yd, wd)
    (loss * 0.7).backward()
    tag = 'wlse {}x{} {}'.format(rows, D, 'weighted' if weighted else 'plain')
    check(loss, want.detach(), (RT, AT), tag)
    check(yhd.grad, yh.grad, (RT, AT * min(1.0, 100.0 / n)), tag + ' gradient')
    out, dyh = Guard(1), Guard(n)
    call('ptts_wlse_fwd', P(yd), P(yhd.detach()), P(wd), P(out.t), rows, D, S())
    call('ptts_wlse_bwd', P(yd), P(yhd.detach()), P(wd), None, P(dyh.t), rows, D, S())      # upstream NULL = 1
    intact(tag, out, dyh)
    check(out.t, want.detach(), (RT, AT), tag + ' guarded')
    check(dyh.t, yh.grad / 0.7, (RT, AT * min(1.0, 100.0 / n)), tag + ' guarded gradient, upstream NULL')
    return loss.detach(), yhd.detach(), yd, wd


@pytest.mark.gpu
@pytest.mark.parametrize('shape', WLSE_SHAPES, ids=lambda s: '{}x{}'.format(*s))
def test_wlse_loss(shape):
    """mean((y - yhat)^2 w[d]) with and without w, D = 1, 7, 86: one workgroup, several, past mean_scaled's element count and past
    the cap of 512 workgroups (n > 2097152) at each D; the backward's 2048-workgroup cap at the same sizes."""
    _wlse_checks(shape[0], shape[1], True)
    _wlse_checks(shape[0], shape[1], False)


@pytest.mark.gpu
@pytest.mark.parametrize('n', [257, 4097, 1048576 + 333, 2097152 + 333])
def test_losses_deterministic_mode(n):
    """ops.deterministic(True): one workgroup adds everything in a fixed order (the sizes of the default mode's one-workgroup,
    several-workgroup and capped launches).  The values meet the bounds of the default mode and a second run gives the same bits."""
    ops, call, P, S, lib = _api()
    old = ops.deterministic()
    try:
        ops.deterministic(True)
        assert lib.ptts_get_deterministic() == 1
        a, vd = _loss_checks(n)
        assert torch.equal(a, ops.wasserstein(vd, -1.0)), 'wasserstein: two deterministic runs differ'
        for rows, D, weighted in ((n, 1, True), (n, 1, False), ((n + 6) // 7, 7, True)):
            a, yhd, yd, wd = _wlse_checks(rows, D, weighted)
            assert torch.equal(a, ops.wlse(yhd, yd, wd)), 'wlse: two deterministic runs differ'
    finally:
        ops.deterministic(old)
    assert lib.ptts_get_deterministic() == int(old)


@pytest.mark.gpu
@pytest.mark.parametrize('T', [1, 33])
@pytest.mark.parametrize('B', [1, 5])
def test_wasserstein_pair(B, T):
    """(-mean(v[:B]), +mean(v[B:])) of the stacked critic output [2B, T, 1] against slicing in fp64: both values, the gradient with both
    outputs used, and with one of them unused (its half of dv is zero)."""
    ops, call, P, S, lib = _api()
    v = r32(randn32(gen(120 + B + T), 2 * B, T, 1) + 0.2)
    for use in ((1.5, -0.7), (1.5, None), (None, -0.7)):
        vr = v.clone().requires_grad_(True)
        lv, lf = -vr[:B].mean(), vr[B:].mean()
        sum(c * l for c, l in zip(use, (lv, lf)) if c is not None).backward()
        vd = dev(v).requires_grad_(True)
        dv_, df_ = ops.wasserstein_pair(vd, B)
        sum(c * l for c, l in zip(use, (dv_, df_)) if c is not None).backward()
        tag = 'wasserstein_pair B={} T={} use={}'.format(B, T, use)
        check(dv_, lv.detach(), (RT, AT), tag + ' first')
        check(df_, lf.detach(), (RT, AT), tag + ' second')
        check(vd.grad, vr.grad, (RT, AT * min(1.0, 100.0 / (B * T))), tag + ' gradient')
        for half, c in ((vd.grad[:B], use[0]), (vd.grad[B:], use[1])):
            if c is None:
                assert bool((half == 0).all()), tag + ': the unused half is not zero'


# ---------------------------------------------------------------------------------------------------------------------------
# 5. Adam and clip
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize('n', ADAM_N)
def test_adam_keras_step(n):
    """ops.adam_keras_step_ with the hyper-parameters of the three optimisers, from step 0 (t = 1) and from a device step of 9999
    (t = 10000), non-zero moments, every seventh gradient exactly zero, gscale = 0.25.  The fp64 reference takes the float32-rounded
    constants the kernel receives, so what is measured is the kernel's arithmetic.  Bounds of test_adam_keras_and_clip: p rtol 1e-5 /
    atol 1e-6, m and v rtol 1e-5 / atol 1e-7.  Gradients and first moments are of size 0.1 (weight gradients are far below 1): the
    two rounded float32 terms of m are then below 0.5 and their roundings (2 x 3e-8) stay inside atol 1e-7 where the sum cancels.
    The t = 10000 case meets these bounds (no measured bound was needed); its ratios are printed like the others."""
    ops, call, P, S, lib = _api()
    g = gen(130)
    p0, g0 = randn32(g, n), r32(torch.randn(n, generator=g, dtype=torch.float64) * 0.4)      # the device holds g / gscale
    g0[::7] = 0.0
    m0 = r32(torch.randn(n, generator=g, dtype=torch.float64) * 0.05)
    v0 = r32(torch.rand(n, generator=g, dtype=torch.float64) * 0.01 + 1e-4)
    gscale = 0.25
    gdv = dev(g0)
    for name, lr, b1, b2, eps in optimiser_hypers():
        for start in (0, 9999):
            pg, mg, vg, step = Guard(n), Guard(n), Guard(n), Guard(1, torch.int32)
            pg.t.copy_(p0); mg.t.copy_(m0); vg.t.copy_(v0); step.t.fill_(start)
            ops.adam_keras_step_(pg.t, gdv, mg.t, vg.t, step.t.view(()), lr, b1, b2, eps, gscale=gscale)
            tag = 'adam {} n={} t={}'.format(name, n, start + 1)
            intact(tag, pg, mg, vg, step)
            assert int(step.t.item()) == start + 1
            pw, mw, vw = adam_ref(p0, g0 * gscale, m0, v0, start + 1, f32(lr), f32(b1), f32(b2), f32(eps))
            check(pg.t, pw, (1e-5, 1e-6), tag + ' p')
            check(mg.t, mw, (1e-5, 1e-7), tag + ' m')
            check(vg.t, vw, (1e-5, 1e-7), tag + ' v')
            assert torch.equal(gdv.cpu(), g0.float()), tag + ': the gradient was written'


@pytest.mark.gpu
@pytest.mark.parametrize('n', ADAM_N)
def test_weight_clip(n):
    """ops.weight_clip_: values inside and exactly at the limits keep their bits, the rest become the limit; lo == hi makes everything
    that one value.  (A NaN weight becomes lo here -- fmaxf returns its other operand -- where torch.clamp keeps the NaN; the
    optimiser's NaN guard stops training before that matters, and the kernel is left as it is.)"""
    ops, call, P, S, lib = _api()
    lo, hi = -0.01, 0.01
    p = r32(torch.randn(n, generator=gen(140), dtype=torch.float64) * 0.02)
    p[::5] = f32(hi)
    p[1::5] = f32(lo)
    pg = Guard(n)
    pg.t.copy_(p)
    ops.weight_clip_(pg.t, lo, hi)
    intact('weight_clip n={}'.format(n), pg)
    want = p.float().clamp(f32(lo), f32(hi))
    assert torch.equal(pg.t.cpu(), want), 'weight_clip n={}: not clamp(p, lo, hi) bit for bit'.format(n)
    check(pg.t, p.clamp(lo, hi), (1e-6, 1e-7), 'weight_clip n={}'.format(n))
    inside = (p.float() >= f32(lo)) & (p.float() <= f32(hi))
    assert torch.equal(pg.t.cpu()[inside], p.float()[inside])
    pg.t.copy_(p)
    ops.weight_clip_(pg.t, 0.005, 0.005)
    intact('weight_clip lo == hi n={}'.format(n), pg)
    assert bool((pg.t == f32(0.005)).all())


# ---------------------------------------------------------------------------------------------------------------------------
# 6. gated product, affine_act forward
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize('n', GATED_N)
def test_gated_mul(n):
    """y = a sigmoid(b) and its backward: the tail alone (n < 4), body + tail, a whole number of float4, past the cap of 2048
    workgroups; b = +-30, +-88, +-89 (exp overflows float32 between the last two), +-100 spread over body and tail: nothing is NaN and
    the saturated values meet the default bound."""
    ops, call, P, S, lib = _api()
    g = gen(150)
    a, b, dy = r32(torch.randn(n, generator=g, dtype=torch.float64) * 2), r32(torch.randn(n, generator=g, dtype=torch.float64) * 3), randn32(g, n)
    sat = torch.tensor([100.0, -100.0, 30.0, -30.0, 88.0, -88.0, 89.0, -89.0], dtype=torch.float64)
    for k in range(min(n, 64)):
        b[(k * 7919) % n if n > 64 else k] = sat[k % 8]
    b[n - 1] = sat[(n - 1) % 2]
    ar, br = a.clone().requires_grad_(True), b.clone().requires_grad_(True)
    yr = ar * torch.sigmoid(br)
    yr.backward(dy)
    ad, bd = dev(a).requires_grad_(True), dev(b).requires_grad_(True)
    yd = ops.gated_mul(ad, bd)
    yd.backward(dev(dy))
    check(yd, yr.detach(), (RT, AT), 'gated_mul n={} y'.format(n))
    check(ad.grad, ar.grad, (RT, AT), 'gated_mul n={} da'.format(n))
    check(bd.grad, br.grad, (RT, AT), 'gated_mul n={} db'.format(n))
    y, da, db = Guard(n), Guard(n), Guard(n)
    call('ptts_gated_mul_fwd', P(ad.detach()), P(bd.detach()), P(y.t), n, S())
    call('ptts_gated_mul_bwd', P(dev(dy)), P(ad.detach()), P(bd.detach()), P(da.t), P(db.t), n, S())
    intact('gated_mul n={}'.format(n), y, da, db)
    assert torch.equal(y.t, yd.detach()) and torch.equal(da.t, ad.grad) and torch.equal(db.t, bd.grad), 'the guarded launches differ from ops.gated_mul'


@pytest.mark.gpu
def test_gated_mul_refuses_unaligned_operands():
    """The float4 kernels need 16-byte aligned operands and the launcher says so: a contiguous view at element offset 1, as either
    operand of ops.gated_mul, raises HipLibraryError (it is not copied, and nothing is computed from a misaligned address)."""
    ops, call, P, S, lib = _api()
    from percivaltts_amd._hip import HipLibraryError
    g = gen(151)
    a, b = randn32(g, 3, 7), randn32(g, 3, 7)
    for oa, ob in ((1, 0), (0, 1), (1, 1)):
        with pytest.raises(HipLibraryError, match='16-byte aligned'):
            ops.gated_mul(dev(a, oa), dev(b, ob))
    check(ops.gated_mul(dev(a), dev(b)), a * torch.sigmoid(b), (RT, AT), 'gated_mul aligned after the refusals')


AFFINE_FWD_CASES = [(37, 3, 0, 0), (37, 8, 1, 0), (37, 8, 0, 1), (37, 4, 0, 0), (5, 260, 0, 0), (1, 4, 0, 0), (1, 1, 0, 0),
                    (699051 + 342, 3, 0, 0), (1048576 + 257, 4, 0, 0), (16133, 260, 0, 0)]


@pytest.mark.gpu
@pytest.mark.parametrize('case', AFFINE_FWD_CASES, ids=lambda c: '{}x{}{}{}'.format(c[0], c[1], '+x1' if c[2] else '', '+y1' if c[3] else ''))
def test_affine_act_forward(case):
    """ptts_affine_act for the four activations, with and without scale / shift: the scalar kernel (C = 3, 1; C = 8 with x or y at
    element offset 1), the float4 kernel (C = 4, 260), and both past their 2048-workgroup caps (n > 2097152 scalar, n > 4194304
    float4); ops.affine_act gives the same bits."""
    ops, call, P, S, lib = _api()
    rows, C, xo, yo = case
    g = gen(160 + C)
    x, sc, sh = randn32(g, rows, C), r32(rand32(g, C) + 0.5), randn32(g, C)
    xd, scd, shd = dev(x, xo), dev(sc), dev(sh)
    big = rows * C > 100000
    for act, code in ACTS.items():
        for affine in ((True,) if (big and act is not None) else (True, False)):
            y = Guard(rows * C, off=yo)
            call('ptts_affine_act', P(xd), P(scd if affine else None), P(shd if affine else None), P(y.t), rows, C, code, ALPHA, S())
            tag = 'affine_act {} {} {}'.format(act, 'affine' if affine else 'plain', case)
            intact(tag, y)
            check(y.t, act_fwd_ref(x, sc if affine else None, sh if affine else None, act), (RT, AT), tag)
            if not yo:
                got = ops.affine_act(xd, scd if affine else None, shd if affine else None, act, ALPHA)
                assert torch.equal(got.reshape(-1), y.t), tag + ': ops.affine_act differs'
