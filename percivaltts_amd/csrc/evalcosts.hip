// Evaluation costs of a ragged batch (zero-padded [B][T][...] with a length per row): the backward of the row mask and the
// per-row reductions behind OptimizerTTSWGAN.validation_costs_batch.  Every row's result depends on that row alone (one
// workgroup per row, fixed-order fp64 sums, no atomics), so an utterance costs the same bytes in any batch; nothing here
// goes to the host.  All of them are bandwidth-trivial single-pass kernels.
// Masked training adds the costs of the whole batch, means over its N real frames: the per-row means combined on the device
// (rows_combine_kernel) and the gradients of the two means, +0 on pad frames.
#include "common.h"
#include <cstdint>

namespace ptts {

constexpr int EC_THREADS = 256;     // elementwise pass
constexpr int EC_ROW_THREADS = 1024;  // one workgroup per row: 16 waves

static inline int ec_blocks(long long n, int per_thread) {
    long long b = (n + (long long)EC_THREADS * per_thread - 1) / ((long long)EC_THREADS * per_thread);
    if (b < 1) b = 1;
    if (b > 2048) b = 2048;   // grid-stride the rest
    return (int)b;
}

// dx[b,t,i] = t < lens[b] ? dy * act'(x * scale[c] + shift[c]) * scale[c] : +0, c = i % C; act in {none, lrelu}.  The indexing
// of affine_act_rows_kernel; VEC = 4 needs C % 4 == 0 (a float4 never crosses a frame).  Each lane reads its dy before it
// writes the same elements of dx, so dx == dy is allowed.
template <int VEC>
__global__ void affine_act_rows_bwd_kernel(const float* dy, const float* __restrict__ x, const float* __restrict__ scale,
                                           const float* __restrict__ shift, float* dx, const int* __restrict__ lens,
                                           long long nv, int T, int inner, int C, int act, float alpha) {
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < nv;
         i += (long long)gridDim.x * blockDim.x) {
        const long long e0 = i * VEC;
        const long long frame = e0 / inner;
        const int t = (int)(frame % T), b = (int)(frame / T);
        float g[VEC];
        if (t < lens[b]) {
            float p[VEC];
            if (VEC == 4) {
                const float4 d = *reinterpret_cast<const float4*>(dy + e0);
                g[0] = d.x; g[1 % VEC] = d.y; g[2 % VEC] = d.z; g[3 % VEC] = d.w;
                if (act == PTTS_ACT_LRELU) {
                    const float4 v = *reinterpret_cast<const float4*>(x + e0);
                    p[0] = v.x; p[1 % VEC] = v.y; p[2 % VEC] = v.z; p[3 % VEC] = v.w;
                }
            } else {
                g[0] = dy[e0];
                if (act == PTTS_ACT_LRELU) p[0] = x[e0];
            }
            const int c = (int)(e0 % C);
#pragma unroll
            for (int e = 0; e < VEC; ++e) {
                if (act == PTTS_ACT_LRELU) g[e] *= lrelu_d(scale ? p[e] * scale[c + e] + shift[c + e] : p[e], alpha);
                if (scale) g[e] *= scale[c + e];
            }
        } else {
#pragma unroll
            for (int e = 0; e < VEC; ++e) g[e] = 0.f;
        }
        if (VEC == 4) *reinterpret_cast<float4*>(dx + e0) = make_float4(g[0], g[1 % VEC], g[2 % VEC], g[3 % VEC]);
        else dx[e0] = g[0];
    }
}

// The workgroup's sum of one fp64 partial per lane: wave64 butterfly, then the 16 wave sums in the order of the waves
// (gp_sqnorm_kernel's scheme).  Valid in lane 0.
__device__ __forceinline__ double row_block_sum(double s, double* sh) {
    s = wave_sum(s);
    __syncthreads();      // (a second reduction of the same kernel reuses sh)
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = s;
    __syncthreads();
    double t = 0.0;
    if (threadIdx.x == 0) {
#pragma unroll
        for (int w = 0; w < EC_ROW_THREADS / 64; ++w) t += sh[w];
    }
    return t;
}

__device__ __forceinline__ long long row_count(const int* lens, int b, int T, int inner) {
    int len = lens[b];
    len = len < 0 ? 0 : (len > T ? T : len);      // never read past the row, whatever the caller passed
    return (long long)len * inner;
}

// out[b] = sign * mean of the first lens[b] frames of row b: they are the first lens[b] * inner elements of the row.
__global__ __launch_bounds__(EC_ROW_THREADS) void rows_mean_kernel(const float* __restrict__ v, const int* __restrict__ lens,
                                                                   int T, int inner, float sign, float* __restrict__ out) {
    __shared__ double sh[EC_ROW_THREADS / 64];
    const int b = blockIdx.x;
    const long long n = row_count(lens, b, T, inner);
    const float* p = v + (long long)b * T * inner;
    double s = 0.0;
    for (long long i = threadIdx.x; i < n; i += EC_ROW_THREADS) s += (double)p[i];
    const double t = row_block_sum(s, sh);
    if (threadIdx.x == 0) out[b] = (float)((double)sign * t / (double)n);
}

// One pass over the real frames of row b: the weighted mean square (specweighted_lse_loss of that utterance alone) and the
// unweighted sum of squares.  The difference is formed in fp64, where the square of a float difference loses nothing.
__global__ __launch_bounds__(EC_ROW_THREADS) void wlse_rows_kernel(const float* __restrict__ y, const float* __restrict__ yhat,
                                                                   const float* __restrict__ w, const int* __restrict__ lens,
                                                                   int T, int D, float* __restrict__ out_ls,
                                                                   double* __restrict__ out_sq) {
    __shared__ double sh[EC_ROW_THREADS / 64];
    const int b = blockIdx.x;
    const long long n = row_count(lens, b, T, D);
    const long long base = (long long)b * T * D;
    double sw = 0.0, sq = 0.0;
    for (long long i = threadIdx.x; i < n; i += EC_ROW_THREADS) {
        const double d = (double)y[base + i] - (double)yhat[base + i];
        const double d2 = d * d;
        sq += d2;
        sw += w ? d2 * (double)w[i % D] : d2;
    }
    if (out_ls) {
        const double t = row_block_sum(sw, sh);
        if (threadIdx.x == 0) out_ls[b] = (float)(t / (double)n);
    }
    if (out_sq) {
        const double t = row_block_sum(sq, sh);
        if (threadIdx.x == 0) out_sq[b] = t;
    }
}

__global__ void gp_penalty_rows_kernel(const float* __restrict__ sq, float* __restrict__ out, int B) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b < B) {
        const double d = 1.0 - sqrt((double)sq[b]);
        out[b] = (float)(d * d);
    }
}

// ---- masked training: the batch costs out of the per-row ones, and their backward ----
// out[0] = sum_b rows[b] * lens[b] / N in fp64, rows in index order: the mean over all N real frames of the batch from the
// per-row means of rows_mean_kernel / wlse_rows_kernel.  One wave.
__global__ __launch_bounds__(64) void rows_combine_kernel(const float* __restrict__ rows, const int* __restrict__ lens, int B,
                                                          int T, double inv_n, float* __restrict__ out) {
    double s = 0.0;
    for (int b = threadIdx.x; b < B; b += 64) {
        int len = lens[b];
        len = len < 0 ? 0 : (len > T ? T : len);
        s += (double)rows[b] * (double)len;
    }
    s = wave_sum(s);
    if (threadIdx.x == 0) out[0] = (float)(s * inv_n);
}

// dv[b,t,:] = t < lens[b] ? upstream[0] * coef : +0  (coef = sign / (N * inner), formed in fp64 on the host)
template <int VEC>
__global__ void rows_mean_bwd_kernel(const float* __restrict__ upstream, const int* __restrict__ lens, float* __restrict__ dv,
                                     long long nv, int T, int inner, float coef) {
    const float g = upstream ? upstream[0] * coef : coef;
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < nv;
         i += (long long)gridDim.x * blockDim.x) {
        const long long e0 = i * VEC;
        const long long frame = e0 / inner;
        const float v = (int)(frame % T) < lens[frame / T] ? g : 0.f;
        if (VEC == 4) *reinterpret_cast<float4*>(dv + e0) = make_float4(v, v, v, v);
        else dv[e0] = v;
    }
}

// dyhat[b,t,d] = t < lens[b] ? upstream[0] * 2 (yhat - y) w[d] * inv : +0  (inv = 1 / (N * D)); wlse_bwd_kernel's arithmetic
__global__ void wlse_rows_bwd_kernel(const float* __restrict__ y, const float* __restrict__ yhat, const float* __restrict__ w,
                                     const float* __restrict__ upstream, const int* __restrict__ lens,
                                     float* __restrict__ dyhat, long long n, int T, int D, float inv) {
    const float up = (upstream ? upstream[0] : 1.f) * inv;
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < n;
         i += (long long)gridDim.x * blockDim.x) {
        const long long frame = i / D;
        float g = 0.f;
        if ((int)(frame % T) < lens[frame / T]) g = up * 2.f * (yhat[i] - y[i]) * (w ? w[i % D] : 1.f);
        dyhat[i] = g;
    }
}

}  // namespace ptts

using namespace ptts;

extern "C" int ptts_affine_act_rows_bwd(const float* dy, const float* x, const float* scale, const float* shift, float* dx,
                                        const int* lens, int B, int T, int inner, int C, int act, float alpha,
                                        void* stream) {
    PTTS_REQUIRE(dy && dx && lens && B > 0 && T > 0 && inner > 0 && C > 0, "affine_act_rows_bwd: bad args");
    PTTS_REQUIRE(inner % C == 0, "affine_act_rows_bwd: inner=%d is no multiple of C=%d", inner, C);
    PTTS_REQUIRE((scale == nullptr) == (shift == nullptr), "affine_act_rows_bwd: scale/shift must come together");
    PTTS_REQUIRE(act == PTTS_ACT_NONE || act == PTTS_ACT_LRELU, "affine_act_rows_bwd: act=%d (none and lrelu only)", act);
    PTTS_REQUIRE(act == PTTS_ACT_NONE || x, "affine_act_rows_bwd: lrelu needs x");
    const long long n = (long long)B * T * inner;
    hipStream_t st = (hipStream_t)stream;
    if (C % 4 == 0 && ((uintptr_t)dy % 16 == 0) && ((uintptr_t)dx % 16 == 0) && ((uintptr_t)x % 16 == 0)) {
        hipLaunchKernelGGL(affine_act_rows_bwd_kernel<4>, dim3(ec_blocks(n / 4, 2)), dim3(EC_THREADS), 0, st, dy, x, scale,
                           shift, dx, lens, n / 4, T, inner, C, act, alpha);
    } else {
        hipLaunchKernelGGL(affine_act_rows_bwd_kernel<1>, dim3(ec_blocks(n, 4)), dim3(EC_THREADS), 0, st, dy, x, scale,
                           shift, dx, lens, n, T, inner, C, act, alpha);
    }
    return check_launch("affine_act_rows_bwd");
}

extern "C" int ptts_rows_mean(const float* v, const int* lens, int B, int T, int inner, float sign, float* out,
                              void* stream) {
    PTTS_REQUIRE(v && lens && out && B > 0 && T > 0 && inner > 0, "rows_mean: bad args");
    hipLaunchKernelGGL(rows_mean_kernel, dim3(B), dim3(EC_ROW_THREADS), 0, (hipStream_t)stream, v, lens, T, inner, sign,
                       out);
    return check_launch("rows_mean");
}

extern "C" int ptts_wlse_rows(const float* y, const float* yhat, const float* w, const int* lens, int B, int T, int D,
                              float* out_ls, double* out_sq, void* stream) {
    PTTS_REQUIRE(y && yhat && lens && B > 0 && T > 0 && D > 0, "wlse_rows: bad args");
    PTTS_REQUIRE(out_ls || out_sq, "wlse_rows: both outputs NULL");
    hipLaunchKernelGGL(wlse_rows_kernel, dim3(B), dim3(EC_ROW_THREADS), 0, (hipStream_t)stream, y, yhat, w, lens, T, D,
                       out_ls, out_sq);
    return check_launch("wlse_rows");
}

extern "C" int ptts_rows_combine(const float* rows, const int* lens, int B, int T, long long N, float* out, void* stream) {
    PTTS_REQUIRE(rows && lens && out && B > 0 && T > 0, "rows_combine: bad args");
    PTTS_REQUIRE(N > 0 && N <= (long long)B * T, "rows_combine: N=%lld real frames in a batch of %d x %d", N, B, T);
    hipLaunchKernelGGL(rows_combine_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, rows, lens, B, T, 1.0 / (double)N, out);
    return check_launch("rows_combine");
}

extern "C" int ptts_rows_mean_bwd(const float* upstream, const int* lens, int B, int T, int inner, float sign, long long N,
                                  float* dv, void* stream) {
    PTTS_REQUIRE(lens && dv && B > 0 && T > 0 && inner > 0, "rows_mean_bwd: bad args");
    PTTS_REQUIRE(N > 0 && N <= (long long)B * T, "rows_mean_bwd: N=%lld real frames in a batch of %d x %d", N, B, T);
    const long long n = (long long)B * T * inner;
    const float coef = (float)((double)sign / ((double)N * (double)inner));
    hipStream_t st = (hipStream_t)stream;
    if (inner % 4 == 0 && (uintptr_t)dv % 16 == 0)
        hipLaunchKernelGGL(rows_mean_bwd_kernel<4>, dim3(ec_blocks(n / 4, 2)), dim3(EC_THREADS), 0, st, upstream, lens, dv,
                           n / 4, T, inner, coef);
    else
        hipLaunchKernelGGL(rows_mean_bwd_kernel<1>, dim3(ec_blocks(n, 4)), dim3(EC_THREADS), 0, st, upstream, lens, dv, n, T,
                           inner, coef);
    return check_launch("rows_mean_bwd");
}

extern "C" int ptts_wlse_rows_bwd(const float* y, const float* yhat, const float* w, const float* upstream, const int* lens,
                                  int B, int T, int D, long long N, float* dyhat, void* stream) {
    PTTS_REQUIRE(y && yhat && lens && dyhat && B > 0 && T > 0 && D > 0, "wlse_rows_bwd: bad args");
    PTTS_REQUIRE(N > 0 && N <= (long long)B * T, "wlse_rows_bwd: N=%lld real frames in a batch of %d x %d", N, B, T);
    const long long n = (long long)B * T * D;
    hipLaunchKernelGGL(wlse_rows_bwd_kernel, dim3(ec_blocks(n, 4)), dim3(EC_THREADS), 0, (hipStream_t)stream, y, yhat, w,
                       upstream, lens, dyhat, n, T, D, (float)(1.0 / ((double)N * (double)D)));
    return check_launch("wlse_rows_bwd");
}

extern "C" int ptts_gp_penalty_rows(const float* sq, float* out, int B, void* stream) {
    PTTS_REQUIRE(sq && out && B > 0, "gp_penalty_rows: bad args");
    hipLaunchKernelGGL(gp_penalty_rows_kernel, dim3((B + EC_THREADS - 1) / EC_THREADS), dim3(EC_THREADS), 0,
                       (hipStream_t)stream, sq, out, B);
    return check_launch("gp_penalty_rows");
}
