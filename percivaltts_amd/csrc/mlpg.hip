// Maximum-likelihood parameter generation (MLPG): the step that turns a network's [T, K*D] statics + deltas into the [T, D]
// trajectory a vocoder reads.  This restates the arithmetic of the reference's external/merlin/mlpg_fast.py:95-135 (called from
// modeltts.py:163-179), which solves one feature at a time on the host through `bandmat`; here all B*D systems of a batch are
// solved at once, one lane each.
//
// For one utterance of L frames and one raw feature d, with K = 1 + number of windows streams (stream k is column k*D + d):
//   mu[t,k], var[t,k] mean and variance;  var[0,k] = var[L-1,k] = 1e11 for every k >= 1 (mlpg_fast.py:122-125)
//   W_0 = I;  W_k[t, t+j] = win_k[j+1], j in {-1,0,1}, taps outside [0, L) dropped (band_c_bm(u, l, .).T)
//   P = sum_k W_k^T diag(1/var[:,k]) W_k  (symmetric positive definite, half-bandwidth 2),  b = sum_k W_k^T (mu[:,k] / var[:,k])
//   c = P^-1 b
// With p_k[t] = 1/var[t,k], r_k[t] = mu[t,k] p_k[t] and (w0,w1,w2) = win_k, row i of the system is
//   P[i][i]   = p_0[i] + sum_k (w2^2 p_k[i-1] + w1^2 p_k[i] + w0^2 p_k[i+1])
//   P[i][i-1] = sum_k (w1 w2 p_k[i-1] + w0 w1 p_k[i])          (i >= 1)
//   P[i][i-2] = sum_k  w0 w2 p_k[i-1]                          (i >= 2)
//   b[i]      = r_0[i] + sum_k (w2 r_k[i-1] + w1 r_k[i] + w0 r_k[i+1])
// (frames outside [0, L) contribute nothing), so P is never materialised: a forward sweep forms row i from frames i-1, i, i+1,
// does the LDL^T step
//   f1 = P[i][i-1] - P[i][i-2] l1[i-1];  l1[i] = f1 / d[i-1];  l2[i] = P[i][i-2] / d[i-2]
//   d[i] = P[i][i] - l2[i] P[i][i-2] - l1[i] f1;  z[i] = b[i] - l1[i] z[i-1] - l2[i] z[i-2]
// with ONE reciprocal (1/d[i]) per row and leaves (z[i]/d[i], l1[i], l2[i]) in the workspace; the back sweep is
//   c[i] = z[i]/d[i] - l1[i+1] c[i+1] - l2[i+2] c[i+2].
//
// Everything between the loads and the store is fp64: cond(P) grows like 16 (std_static / std_acc)^2 and reaches ~1e7 for the
// spread of a real std4norm.dat, which an fp32 sweep cannot carry (tests/test_mlpg.py records how far off it is).  The operands
// and the result are fp32 in memory; fp32 -> fp64 is exact.
//
// One lane per system, lanes along d: a wave's loads of frame t are K contiguous runs of the [.., K*D] row and its stores one run
// of [.., D]; the workspace is laid out [t][3][B*D], so both sweeps are coalesced.  The row loads do not depend on the
// recurrence and are issued MLPG_PF rows ahead; the chain itself is serial.  No lane looks at another: the result of a system
// does not depend on what else is in the batch, and there is nothing for deterministic mode to switch.
#include "common.h"

namespace ptts {

constexpr int MLPG_PF = 4;          // rows per prefetch batch (one batch is in flight while the previous one is consumed)
constexpr double MLPG_EDGE_PREC = 1.0 / 100000000000.0;   // 1 / var at the first and last frame of the delta streams

struct MlpgWins {
    double w[2][3];
};

template <int K, bool PERFRAME>
struct MlpgRaw {
    float y[K];
    float v[PERFRAME ? K : 1];
};

// grid (ceil(D/64), B), 64 threads.  L = lengths[b] clamped to [0, T] (T without lengths).
template <int K, bool PERFRAME, bool AFFINE>
__global__ __launch_bounds__(64) void mlpg_kernel(const float* __restrict__ y, const float* __restrict__ mean,
                                                  const float* __restrict__ stdv, const float* __restrict__ var,
                                                  const MlpgWins wins, const int* __restrict__ lengths, float* __restrict__ out,
                                                  double* ws, int B, int T, int D) {
    const int d = blockIdx.x * 64 + threadIdx.x, b = blockIdx.y;
    if (d >= D) return;
    int L = T;
    if (lengths) {
        L = lengths[b];
        L = L < 0 ? 0 : (L > T ? T : L);
    }
    const long long KD = (long long)K * D;
    const size_t S = (size_t)B * D, s = (size_t)b * D + d;
    const float* yb = y + (long long)b * T * KD + d;
    const float* vb = PERFRAME ? var + (long long)b * T * KD + d : nullptr;
    float* ob = out + (long long)b * T * D + d;

    double mn[K], sd[K], pcol[K];
#pragma unroll
    for (int k = 0; k < K; ++k) {
        mn[k] = AFFINE ? (double)mean[k * D + d] : 0.0;
        sd[k] = AFFINE ? (double)stdv[k * D + d] : 1.0;
        pcol[k] = PERFRAME ? 0.0 : 1.0 / (double)var[k * D + d];
    }
    // products of the window taps, per delta stream
    double w22[K - 1], w11[K - 1], w00[K - 1], w12[K - 1], w01[K - 1], w02[K - 1], w0[K - 1], w1[K - 1], w2[K - 1];
#pragma unroll
    for (int k = 0; k < K - 1; ++k) {
        w0[k] = wins.w[k][0]; w1[k] = wins.w[k][1]; w2[k] = wins.w[k][2];
        w00[k] = w0[k] * w0[k]; w11[k] = w1[k] * w1[k]; w22[k] = w2[k] * w2[k];
        w01[k] = w0[k] * w1[k]; w12[k] = w1[k] * w2[k]; w02[k] = w0[k] * w2[k];
    }

    typedef MlpgRaw<K, PERFRAME> Raw;
    auto load_raw = [&](int t, Raw& r) {
#pragma unroll
        for (int k = 0; k < K; ++k) {
            r.y[k] = t < L ? yb[t * KD + k * D] : 0.f;
            if (PERFRAME) r.v[k] = t < L ? vb[t * KD + k * D] : 1.f;
        }
    };
    // p[k] = 1/var, r[k] = mu/var of frame t; zero for a frame outside the utterance
    auto convert = [&](int t, const Raw& raw, double* p, double* r) {
        const bool in = t < L, edge = t == 0 || t == L - 1;
#pragma unroll
        for (int k = 0; k < K; ++k) {
            const double mu = AFFINE ? (double)raw.y[k] * sd[k] + mn[k] : (double)raw.y[k];
            double pk = PERFRAME ? 1.0 / (double)raw.v[k] : pcol[k];
            if (k >= 1 && edge) pk = MLPG_EDGE_PREC;
            p[k] = in ? pk : 0.0;
            r[k] = in ? mu * pk : 0.0;
        }
    };

    // ---- forward sweep -------------------------------------------------------------------------------------------------
    double pp[K], rp[K], pc[K], rc[K], pn[K], rn[K];
#pragma unroll
    for (int k = 0; k < K; ++k) pp[k] = rp[k] = 0.0;
    Raw batch[MLPG_PF];
    {
        Raw r0;
        load_raw(0, r0);
#pragma unroll
        for (int u = 0; u < MLPG_PF; ++u) load_raw(1 + u, batch[u]);      // step i consumes frame i + 1
        convert(0, r0, pc, rc);
    }
    double l1p = 0.0, invd1 = 0.0, invd2 = 0.0, z1 = 0.0, z2 = 0.0;
    for (int i0 = 0; i0 < L; i0 += MLPG_PF) {
        Raw cur[MLPG_PF];
#pragma unroll
        for (int u = 0; u < MLPG_PF; ++u) cur[u] = batch[u];
#pragma unroll
        for (int u = 0; u < MLPG_PF; ++u) load_raw(i0 + MLPG_PF + 1 + u, batch[u]);
#pragma unroll
        for (int u = 0; u < MLPG_PF; ++u) {
            const int i = i0 + u;
            if (i < L) {
                convert(i + 1, cur[u], pn, rn);
                double a = pc[0], e1 = 0.0, e2 = 0.0, bb = rc[0];
#pragma unroll
                for (int k = 1; k < K; ++k) {
                    a += w22[k - 1] * pp[k] + w11[k - 1] * pc[k] + w00[k - 1] * pn[k];
                    e1 += w12[k - 1] * pp[k] + w01[k - 1] * pc[k];
                    e2 += w02[k - 1] * pp[k];
                    bb += w2[k - 1] * rp[k] + w1[k - 1] * rc[k] + w0[k - 1] * rn[k];
                }
                if (i < 1) e1 = 0.0;
                if (i < 2) e2 = 0.0;
                const double f1 = e1 - e2 * l1p;
                const double l1 = f1 * invd1, l2 = e2 * invd2;
                const double dd = a - l2 * e2 - l1 * f1;
                const double invd = 1.0 / dd;
                const double z = bb - l1 * z1 - l2 * z2;
                double* w = ws + (size_t)i * 3 * S + s;
                w[0] = z * invd;
                w[S] = l1;
                w[2 * S] = l2;
                l1p = l1; invd2 = invd1; invd1 = invd; z2 = z1; z1 = z;
#pragma unroll
                for (int k = 0; k < K; ++k) {
                    pp[k] = pc[k]; rp[k] = rc[k]; pc[k] = pn[k]; rc[k] = rn[k];
                }
            }
        }
    }

    // ---- back sweep: c[i] = q[i] - l1[i+1] c[i+1] - l2[i+2] c[i+2] ------------------------------------------------------------
    struct Row { double q, l1n, l2n; };
    auto load_row = [&](int i, Row& r) {
        const bool in = i >= 0;
        r.q = in ? ws[(size_t)i * 3 * S + s] : 0.0;
        r.l1n = in && i + 1 < L ? ws[((size_t)(i + 1) * 3 + 1) * S + s] : 0.0;
        r.l2n = in && i + 2 < L ? ws[((size_t)(i + 2) * 3 + 2) * S + s] : 0.0;
    };
    Row rb[MLPG_PF];
#pragma unroll
    for (int u = 0; u < MLPG_PF; ++u) load_row(L - 1 - u, rb[u]);
    double c1 = 0.0, c2 = 0.0;
    for (int i0 = L - 1; i0 >= 0; i0 -= MLPG_PF) {
        Row cur[MLPG_PF];
#pragma unroll
        for (int u = 0; u < MLPG_PF; ++u) cur[u] = rb[u];
#pragma unroll
        for (int u = 0; u < MLPG_PF; ++u) load_row(i0 - MLPG_PF - u, rb[u]);
#pragma unroll
        for (int u = 0; u < MLPG_PF; ++u) {
            const int i = i0 - u;
            if (i >= 0) {
                const double c = cur[u].q - cur[u].l1n * c1 - cur[u].l2n * c2;
                ob[(long long)i * D] = (float)c;
                c2 = c1; c1 = c;
            }
        }
    }
    for (int t = L; t < T; ++t) ob[(long long)t * D] = 0.f;
}

template <int K>
static void mlpg_launch(bool perframe, bool affine, dim3 grid, hipStream_t st, const float* y, const float* mean,
                        const float* stdv, const float* var, const MlpgWins& wins, const int* lengths, float* out, double* ws,
                        int B, int T, int D) {
#define PTTS_MLPG_GO(PF, AF) \
    hipLaunchKernelGGL((mlpg_kernel<K, PF, AF>), grid, dim3(64), 0, st, y, mean, stdv, var, wins, lengths, out, ws, B, T, D)
    if (perframe) { if (affine) PTTS_MLPG_GO(true, true); else PTTS_MLPG_GO(true, false); }
    else          { if (affine) PTTS_MLPG_GO(false, true); else PTTS_MLPG_GO(false, false); }
#undef PTTS_MLPG_GO
}

}  // namespace ptts

using namespace ptts;

extern "C" size_t ptts_mlpg_workspace_bytes(int B, int T, int D) {
    if (B < 1 || T < 1 || D < 1) return 16;
    return align_up((size_t)B * T * D * 3 * sizeof(double), 256);
}

extern "C" int ptts_mlpg(const float* y, const float* mean, const float* stdv, const float* var, int var_per_frame,
                         const float* wins, const int* lengths, float* out, void* workspace, size_t workspace_bytes, int B,
                         int T, int D, int K, void* stream) {
    PTTS_REQUIRE(y && var && wins && out, "mlpg: null tensor");
    PTTS_REQUIRE(B > 0 && T > 0 && D > 0, "mlpg: bad dims B=%d T=%d D=%d", B, T, D);
    PTTS_REQUIRE(K == 2 || K == 3, "mlpg: K=%d streams (statics + one or two three-tap windows are supported)", K);
    PTTS_REQUIRE((mean != nullptr) == (stdv != nullptr), "mlpg: mean and std go together (both or neither)");
    PTTS_REQUIRE(B <= 65535, "mlpg: B=%d exceeds the grid's second dimension", B);
    const size_t need = ptts_mlpg_workspace_bytes(B, T, D);
    if (!workspace || workspace_bytes < need) {
        set_error("mlpg: workspace %zu < %zu", workspace_bytes, need);
        return PTTS_EWORKSPACE;
    }
    MlpgWins w;
    for (int k = 0; k < 2; ++k)
        for (int j = 0; j < 3; ++j) w.w[k][j] = k < K - 1 ? (double)wins[k * 3 + j] : 0.0;
    const dim3 grid((D + 63) / 64, B);
    hipStream_t st = (hipStream_t)stream;
    if (K == 2) mlpg_launch<2>(var_per_frame != 0, mean != nullptr, grid, st, y, mean, stdv, var, w, lengths, out, (double*)workspace, B, T, D);
    else        mlpg_launch<3>(var_per_frame != 0, mean != nullptr, grid, st, y, mean, stdv, var, w, lengths, out, (double*)workspace, B, T, D);
    return check_launch("mlpg");
}
