// Feature composition: the corpus-wide pass that turns raw per-utterance feature rows into what the training reads and what
// generation de-normalises -- delta windows appended, per-column statistics, normalisation.  It restates the arithmetic of the
// reference's compose.py (windows :239-250, statistics :264-298, normalisers :34-183), which makes three sweeps over the files in
// numpy, one column at a time through scipy.signal.convolve; here a chunk of utterances is packed row-wise as [R, D] fp32 with an
// int32 offsets array [N+1] (utterance u owns rows offsets[u] .. offsets[u+1]-1, no padding) and each sweep is one launch.
//
// compose_windows, for an utterance of T frames, a column c and window k (taps w, fp64), t in 1..T-2:
//   reference order  YW[t] = -(w[2]*y[t-1] + w[1]*y[t] + w[0]*y[t+1])          (-scipy.signal.convolve(y, w)[2:-2])
//   MLPG order       YW[t] =   w[0]*y[t-1] + w[1]*y[t] + w[2]*y[t+1]           (W_k y of mlpg.hip)
//   YW[0] = YW[1], YW[T-1] = YW[T-2];  fp64, added left to right as written (from the
//   oldest frame, the order numpy's direct convolution takes), rounded once to fp32 into column (k+1)*D + c; column c is y itself.
// The two orders agree exactly for an antisymmetric window ([-0.5, 0, 0.5]) and are negatives of each other for a symmetric one
// ([1, -2, 1]).
//
// Statistics ride along while the values are in registers: min and max of the fp32 results (rounding is monotone, so these are the
// roundings of the fp64 extremes), the sum of the fp64 values before rounding.  Lanes lie along the columns, the four waves of a
// workgroup take the rows of ONE utterance t = wave, wave + 4, ...; the waves' accumulators are combined through LDS in wave order
// and stored as that utterance's partial in the caller's workspace ([N][W] per statistic).  A second, tiny launch adds the partials
// of the statistics utterances in utterance order onto the caller's running buffers.  The unit of the first stage is the utterance
// and not a tile of the packed rows on purpose: an utterance's partial is then a function of its own rows only, and the running
// sum is the same chain of additions however the corpus was cut into chunks -- compose.py's device-resident and streamed routes
// must write identical files.  No atomics anywhere; every store is a plain vector store.
//
// The three row loads of a window value are issued per row (centre clamped to 1..T-2, neighbours clamped into the utterance): the
// four waves work on adjacent rows, so two of the three are L1/L2 hits and HBM sees each input row once.
//
// compose_sqdev is the centred second pass (sum_r (double(y[r,c]) - mean[c])^2, mean in fp64) with the same two stages;
// compose_normalise is elementwise in fp32 in exactly numpy's operation order (-ffp-contract=off keeps the multiply and the add
// apart; hipcc's default fp32 division is the correctly rounded one), so its output equals numpy's bit for bit.
#include "common.h"

namespace ptts {

constexpr int CMP_WAVES = 4;            // waves per workgroup, rows of an utterance dealt round-robin to them
constexpr int CMP_MAX_K = 8;            // statics + up to seven windows

struct ComposeWins {
    double w[CMP_MAX_K - 1][3];
};

// utterance u of the chunk -> its row range, clamped into [0, R] so that a bad offsets array cannot reach outside the buffers
__device__ __forceinline__ void utt_rows(const int* __restrict__ offsets, int u, int R, int& s, int& e) {
    s = offsets[u];
    e = offsets[u + 1];
    s = s < 0 ? 0 : (s > R ? R : s);
    e = e < s ? s : (e > R ? R : e);
}

// grid (G, ceil(D/64)), block (64, CMP_WAVES).  part_* [N][K*D]; utterances >= n_stat write no partials.
__global__ __launch_bounds__(64 * CMP_WAVES) void compose_windows_kernel(
    const float* __restrict__ y, const int* __restrict__ offsets, const ComposeWins wins, const int mlpg_order,
    float* __restrict__ out, float* __restrict__ part_min, float* __restrict__ part_max, double* __restrict__ part_sum,
    const int n_stat, const int N, const int R, const int D, const int K) {
    __shared__ float s_min[CMP_WAVES][CMP_MAX_K][64], s_max[CMP_WAVES][CMP_MAX_K][64];
    __shared__ double s_sum[CMP_WAVES][CMP_MAX_K][64];
    const int lane = threadIdx.x, wave = threadIdx.y;
    const int c = blockIdx.y * 64 + lane;
    const bool live = c < D;
    const size_t KD = (size_t)K * D;
    for (int u = blockIdx.x; u < N; u += gridDim.x) {
        int s, e;
        utt_rows(offsets, u, R, s, e);
        const int T = e - s;
        const bool stat = u < n_stat;
        float mn[CMP_MAX_K], mx[CMP_MAX_K];
        double sm[CMP_MAX_K];
#pragma unroll
        for (int k = 0; k < CMP_MAX_K; ++k) { mn[k] = INFINITY; mx[k] = -INFINITY; sm[k] = 0.0; }
        if (live) {
            const float* yu = y + (size_t)s * D + c;
            float* ou = out + (size_t)s * KD + c;
#pragma unroll 2
            for (int t = wave; t < T; t += CMP_WAVES) {
                const float y0 = yu[(size_t)t * D];
                float* o = ou + (size_t)t * KD;
                o[0] = y0;
                mn[0] = y0 < mn[0] ? y0 : mn[0];
                mx[0] = y0 > mx[0] ? y0 : mx[0];
                sm[0] += (double)y0;
                if (K > 1) {
                    int cc = t < 1 ? 1 : t;
                    cc = cc > T - 2 ? T - 2 : cc;
                    cc = cc < 0 ? 0 : cc;
                    const int lo = cc > 0 ? cc - 1 : 0, hi = cc + 1 < T ? cc + 1 : T - 1;
                    const double yc = cc == t ? (double)y0 : (double)yu[(size_t)cc * D];
                    const double yp = (double)yu[(size_t)lo * D], yn = (double)yu[(size_t)hi * D];
#pragma unroll
                    for (int k = 1; k < CMP_MAX_K; ++k) {
                        if (k < K) {
                            const double w0 = wins.w[k - 1][0], w1 = wins.w[k - 1][1], w2 = wins.w[k - 1][2];
                            const double v = mlpg_order ? (w0 * yp + w1 * yc) + w2 * yn : -((w2 * yp + w1 * yc) + w0 * yn);
                            const float vf = (float)v;
                            o[(size_t)k * D] = vf;
                            mn[k] = vf < mn[k] ? vf : mn[k];
                            mx[k] = vf > mx[k] ? vf : mx[k];
                            sm[k] += v;
                        }
                    }
                }
            }
        }
        if (stat) {             // uniform over the workgroup
#pragma unroll
            for (int k = 0; k < CMP_MAX_K; ++k)
                if (k < K) { s_min[wave][k][lane] = mn[k]; s_max[wave][k][lane] = mx[k]; s_sum[wave][k][lane] = sm[k]; }
            __syncthreads();
            if (live) {
                // waves 0..CMP_WAVES-1 in order; wave w finishes streams w, w + CMP_WAVES, ...
                for (int k = wave; k < K; k += CMP_WAVES) {
                    float a = s_min[0][k][lane], b = s_max[0][k][lane];
                    double d = s_sum[0][k][lane];
#pragma unroll
                    for (int w = 1; w < CMP_WAVES; ++w) {
                        const float a2 = s_min[w][k][lane], b2 = s_max[w][k][lane];
                        a = a2 < a ? a2 : a;
                        b = b2 > b ? b2 : b;
                        d += s_sum[w][k][lane];
                    }
                    const size_t p = (size_t)u * KD + (size_t)k * D + c;
                    part_min[p] = a; part_max[p] = b; part_sum[p] = d;
                }
            }
            __syncthreads();
        }
    }
}

// one thread per column: the partials of utterances 0..n_stat-1, in that order, onto the running buffers
__global__ void compose_stats_finish_kernel(const float* __restrict__ part_min, const float* __restrict__ part_max,
                                            const double* __restrict__ part_sum, float* __restrict__ run_min,
                                            float* __restrict__ run_max, double* __restrict__ run_sum, int n_stat, int W) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= W) return;
    float a = run_min[c], b = run_max[c];
    double d = run_sum[c];
    for (int u = 0; u < n_stat; ++u) {
        const size_t p = (size_t)u * W + c;
        const float a2 = part_min[p], b2 = part_max[p];
        a = a2 < a ? a2 : a;
        b = b2 > b ? b2 : b;
        d += part_sum[p];
    }
    run_min[c] = a; run_max[c] = b; run_sum[c] = d;
}

// grid (G, ceil(W/64)), block (64, CMP_WAVES): utterance u < n_stat -> part [u][W]
__global__ __launch_bounds__(64 * CMP_WAVES) void compose_sqdev_kernel(const float* __restrict__ y, const int* __restrict__ offsets,
                                                                      const double* __restrict__ mean, double* __restrict__ part,
                                                                      const int n_stat, const int R, const int W) {
    __shared__ double s_sq[CMP_WAVES][64];
    const int lane = threadIdx.x, wave = threadIdx.y;
    const int c = blockIdx.y * 64 + lane;
    const bool live = c < W;
    const double m = live ? mean[c] : 0.0;
    for (int u = blockIdx.x; u < n_stat; u += gridDim.x) {
        int s, e;
        utt_rows(offsets, u, R, s, e);
        double sq = 0.0;
        if (live) {
            const float* yu = y + (size_t)s * W + c;
#pragma unroll 4
            for (int t = wave; t < e - s; t += CMP_WAVES) {
                const double d = (double)yu[(size_t)t * W] - m;
                sq += d * d;
            }
        }
        s_sq[wave][lane] = sq;
        __syncthreads();
        if (wave == 0 && live) {
            double d = s_sq[0][lane];
#pragma unroll
            for (int w = 1; w < CMP_WAVES; ++w) d += s_sq[w][lane];
            part[(size_t)u * W + c] = d;
        }
        __syncthreads();
    }
}

__global__ void compose_sqdev_finish_kernel(const double* __restrict__ part, double* __restrict__ run_sq, int n_stat, int W) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= W) return;
    double d = run_sq[c];
    for (int u = 0; u < n_stat; ++u) d += part[(size_t)u * W + c];
    run_sq[c] = d;
}

// grid (G, ceil(Wout/64)), block (64, CMP_WAVES); rows dealt to (workgroup, wave) round-robin.  Safe in place without keepidx:
// each element is read and written by the same thread.
template <int MODE>
__global__ __launch_bounds__(64 * CMP_WAVES) void compose_normalise_kernel(const float* y, const int* __restrict__ keepidx,
                                                                          const float* __restrict__ a, const float* __restrict__ b,
                                                                          const float scale, const float offset, float* out,
                                                                          const long long R, const int Win, const int Wout) {
    const int j = blockIdx.y * 64 + threadIdx.x;
    if (j >= Wout) return;
    int src = keepidx ? keepidx[j] : j;
    src = src < 0 ? 0 : (src >= Win ? Win - 1 : src);
    const float aj = a[j], bj = b[j];
    const long long step = (long long)gridDim.x * CMP_WAVES;
#pragma unroll 4
    for (long long r = (long long)blockIdx.x * CMP_WAVES + threadIdx.y; r < R; r += step) {
        const float v = y[r * Win + src];
        float q = (v - aj) / bj;
        if (MODE == PTTS_NORM_MINMAX) {
            q = q - 0.5f;
            q = q * 2.0f;
            q = q * scale;
            q = q + offset;
        }
        out[r * Wout + j] = q;
    }
}

static int device_cus() {
    static int cus = 0;
    if (cus == 0) {
        int dev = 0, n = 0;
        if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n < 1)
            n = 256;
        cus = n;
    }
    return cus;
}

// workgroups along the work items: about eight workgroups per CU over all column blocks, never more than there are items
static int walkers(long long items, int colblocks) {
    long long g = ((long long)device_cus() * 8 + colblocks - 1) / colblocks;
    g = g < 1 ? 1 : g;
    return (int)(items < g ? items : g);
}

}  // namespace ptts

using namespace ptts;

extern "C" size_t ptts_compose_windows_workspace_bytes(int N, int D, int K) {
    if (N < 1 || D < 1 || K < 1) return 16;
    return align_up((size_t)N * K * D * (2 * sizeof(float) + sizeof(double)), 256);
}

extern "C" int ptts_compose_windows(const float* y, const int* offsets, const double* wins, int mlpg_order, float* out,
                                    float* run_min, float* run_max, double* run_sum, int n_stat_utts, void* workspace,
                                    size_t workspace_bytes, int N, int R, int D, int K, void* stream) {
    PTTS_REQUIRE(y && offsets && out, "compose_windows: null tensor");
    PTTS_REQUIRE(N > 0 && R > 0 && D > 0, "compose_windows: bad dims N=%d R=%d D=%d", N, R, D);
    PTTS_REQUIRE(K >= 1 && K <= CMP_MAX_K, "compose_windows: K=%d streams (statics + up to %d three-tap windows)", K, CMP_MAX_K - 1);
    PTTS_REQUIRE(K == 1 || wins, "compose_windows: K=%d needs %d windows, got none", K, K - 1);
    PTTS_REQUIRE(out != y, "compose_windows: cannot run in place");
    PTTS_REQUIRE(n_stat_utts >= 0, "compose_windows: n_stat_utts=%d", n_stat_utts);
    const int n_stat = n_stat_utts < N ? n_stat_utts : N;
    PTTS_REQUIRE(n_stat == 0 || (run_min && run_max && run_sum), "compose_windows: statistics asked for without running buffers");
    const size_t W = (size_t)K * D;
    float* pmin = nullptr; float* pmax = nullptr; double* psum = nullptr;
    if (n_stat > 0) {
        const size_t need = ptts_compose_windows_workspace_bytes(n_stat, D, K);
        if (!workspace || workspace_bytes < need) {
            set_error("compose_windows: workspace %zu < %zu", workspace_bytes, need);
            return PTTS_EWORKSPACE;
        }
        psum = (double*)workspace;
        pmin = (float*)(psum + (size_t)n_stat * W);
        pmax = pmin + (size_t)n_stat * W;
    }
    ComposeWins w;
    for (int k = 0; k < CMP_MAX_K - 1; ++k)
        for (int j = 0; j < 3; ++j) w.w[k][j] = k < K - 1 ? wins[k * 3 + j] : 0.0;
    hipStream_t st = (hipStream_t)stream;
    const int cb = (D + 63) / 64;
    hipLaunchKernelGGL(compose_windows_kernel, dim3(walkers(N, cb), cb), dim3(64, CMP_WAVES), 0, st, y, offsets, w,
                       mlpg_order != 0, out, pmin, pmax, psum, n_stat, N, R, D, K);
    if (n_stat > 0)
        hipLaunchKernelGGL(compose_stats_finish_kernel, dim3((unsigned)((W + 255) / 256)), dim3(256), 0, st, pmin, pmax, psum,
                           run_min, run_max, run_sum, n_stat, (int)W);
    return check_launch("compose_windows");
}

extern "C" size_t ptts_compose_sqdev_workspace_bytes(int N, int W) {
    if (N < 1 || W < 1) return 16;
    return align_up((size_t)N * W * sizeof(double), 256);
}

extern "C" int ptts_compose_sqdev(const float* y, const int* offsets, const double* mean, double* run_sq, int n_stat_utts,
                                  void* workspace, size_t workspace_bytes, int N, int R, int W, void* stream) {
    PTTS_REQUIRE(y && offsets && mean && run_sq, "compose_sqdev: null tensor");
    PTTS_REQUIRE(N > 0 && R > 0 && W > 0, "compose_sqdev: bad dims N=%d R=%d W=%d", N, R, W);
    PTTS_REQUIRE(n_stat_utts >= 0, "compose_sqdev: n_stat_utts=%d", n_stat_utts);
    const int n_stat = n_stat_utts < N ? n_stat_utts : N;
    if (n_stat == 0) return PTTS_OK;
    const size_t need = ptts_compose_sqdev_workspace_bytes(n_stat, W);
    if (!workspace || workspace_bytes < need) {
        set_error("compose_sqdev: workspace %zu < %zu", workspace_bytes, need);
        return PTTS_EWORKSPACE;
    }
    hipStream_t st = (hipStream_t)stream;
    const int cb = (W + 63) / 64;
    hipLaunchKernelGGL(compose_sqdev_kernel, dim3(walkers(n_stat, cb), cb), dim3(64, CMP_WAVES), 0, st, y, offsets, mean,
                       (double*)workspace, n_stat, R, W);
    hipLaunchKernelGGL(compose_sqdev_finish_kernel, dim3((W + 255) / 256), dim3(256), 0, st, (const double*)workspace, run_sq,
                       n_stat, W);
    return check_launch("compose_sqdev");
}

extern "C" int ptts_compose_normalise(const float* y, const int* keepidx, const float* a, const float* b, int mode, float scale,
                                      float offset, float* out, long long R, int Win, int Wout, void* stream) {
    PTTS_REQUIRE(y && a && b && out, "compose_normalise: null tensor");
    PTTS_REQUIRE(R > 0 && Win > 0 && Wout > 0, "compose_normalise: bad dims R=%lld Win=%d Wout=%d", R, Win, Wout);
    PTTS_REQUIRE(mode == PTTS_NORM_MEANSTD || mode == PTTS_NORM_MINMAX, "compose_normalise: unknown mode %d", mode);
    PTTS_REQUIRE(keepidx || Wout == Win, "compose_normalise: Wout=%d differs from Win=%d without a keepidx", Wout, Win);
    PTTS_REQUIRE(!keepidx || out != y, "compose_normalise: a column gather cannot run in place");
    hipStream_t st = (hipStream_t)stream;
    const int cb = (Wout + 63) / 64;
    const dim3 grid(walkers((R + CMP_WAVES - 1) / CMP_WAVES, cb), cb), block(64, CMP_WAVES);
    if (mode == PTTS_NORM_MINMAX)
        hipLaunchKernelGGL((compose_normalise_kernel<PTTS_NORM_MINMAX>), grid, block, 0, st, y, keepidx, a, b, scale, offset, out, R, Win, Wout);
    else
        hipLaunchKernelGGL((compose_normalise_kernel<PTTS_NORM_MEANSTD>), grid, block, 0, st, y, keepidx, a, b, scale, offset, out, R, Win, Wout);
    return check_launch("compose_normalise");
}
