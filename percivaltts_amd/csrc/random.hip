// The library's random numbers: a counter-based generator (Philox4x32-10, Salmon et al., "Parallel random numbers: as easy as
// 1, 2, 3", SC'11; the constants and the ten rounds of the Random123 distribution) and the two layers that draw from it,
// Dropout with Keras noise_shape = (batch, 1, None) (reference networktts.py:65-70, pDO) and the noise channels of
// GaussianNoiseInput (networktts.py:36-56).
//
// Every number is a pure function of (seed, call counter, index): no mask and no per-thread generator state is ever stored.
//   Philox counter = (index lo, index hi, call lo, call hi),  key = (seed lo, seed hi)
// The generator's state is a block of two 64-bit words in device memory, {seed, call counter}.  A forward entry point reads it
// in its main kernel, which also leaves the call counter it used in the caller's 8-byte word `used`, and then enqueues a
// one-thread kernel on the same stream that adds one to the counter.  The backward pass regenerates the mask from `used`.
// Inside a captured graph every replay therefore draws fresh numbers and its backward pass sees its own forward's mask.
// Calls that share a state block are meant to be ordered on one stream; two streams racing for it may draw the same call.
//
//   Dropout index:  the four words of Philox block (b0 + b) * ceil(D / 4) + (d >> 2) serve the columns 4 (d >> 2) .. + 3 of
//                   sample b0 + b; word w keeps its column where float(w >> 8) * 2^-24 < 1 - rate (all in fp32).
//   Normal index:   block e >> 2 serves the elements e & ~3 .. + 3 (e = i0 + i): Box-Muller on the word pairs (0, 1), (2, 3),
//                   u1 = ((w >> 8) + 1) * 2^-24 in (0, 1] for the logarithm, u2 = (w' >> 8) * 2^-24 in [0, 1) for the angle.
#include "common.h"

namespace ptts {

typedef unsigned long long u64;

struct Philox4 { unsigned w[4]; };

__device__ __forceinline__ Philox4 philox4x32_10(u64 index, u64 call, u64 seed) {
    unsigned c0 = (unsigned)index, c1 = (unsigned)(index >> 32), c2 = (unsigned)call, c3 = (unsigned)(call >> 32);
    unsigned k0 = (unsigned)seed, k1 = (unsigned)(seed >> 32);
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const unsigned hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
        const unsigned hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
        c0 = hi1 ^ c1 ^ k0; c1 = lo1; c2 = hi0 ^ c3 ^ k1; c3 = lo0;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    return Philox4{{c0, c1, c2, c3}};
}

__device__ __forceinline__ float u01(unsigned w) { return (float)(w >> 8) * 0x1p-24f; }            // [0, 1)
__device__ __forceinline__ float u01_open0(unsigned w) { return (float)((w >> 8) + 1u) * 0x1p-24f; } // (0, 1]

__global__ void rng_seed_kernel(u64* __restrict__ state, u64 seed, u64 counter) { state[0] = seed; state[1] = counter; }
__global__ void rng_advance_kernel(u64* __restrict__ state) { state[1] += 1; }

constexpr int DO_THREADS = 256;

// grid (time chunks, samples), 256 threads.  A workgroup owns CGW = min(ceil(D/4), 256) column groups at a time and R = 256 / CGW
// time rows per sweep; its first CGW threads draw the groups' masks once into LDS and all of them reuse these down the rows of
// the chunk.  VEC: D % 4 == 0 and 16-byte aligned pointers (one float4 per lane and row); otherwise up to four scalar accesses.
// FWD: the call counter comes from the state block and is left in `used`; else it is read from `used`.
template <bool VEC, bool FWD>
__global__ __launch_bounds__(DO_THREADS) void dropout_kernel(
    const float* __restrict__ x, const float* __restrict__ scale, const float* __restrict__ shift, float* __restrict__ y,
    const u64* __restrict__ state, u64* __restrict__ used, float keep, float inv_keep, float alpha, int mode,
    int B, int T, int D, long long b0, int rows_per_chunk) {
    __shared__ float msk[DO_THREADS * 4];
    const u64 seed = state[0];
    const u64 call = FWD ? state[1] : used[0];
    if (FWD && blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0) used[0] = call;
    const int DG = (D + 3) >> 2;
    const int CGW = DG < DO_THREADS ? DG : DO_THREADS;
    const int R = DO_THREADS / CGW;
    const int tid = threadIdx.x;
    const int cl = tid % CGW, tr = tid / CGW;      // (threads with tr >= R idle through the row loop)
    const int t_lo = blockIdx.x * rows_per_chunk;
    const int t_hi = t_lo + rows_per_chunk < T ? t_lo + rows_per_chunk : T;
    for (int b = blockIdx.y; b < B; b += gridDim.y) {
        for (int g0 = 0; g0 < DG; g0 += CGW) {
            if (tid < CGW && g0 + tid < DG) {
                const Philox4 p = philox4x32_10((u64)(b0 + b) * (u64)DG + (u64)(g0 + tid), call, seed);
#pragma unroll
                for (int e = 0; e < 4; ++e) msk[tid * 4 + e] = u01(p.w[e]) < keep ? inv_keep : 0.f;
            }
            __syncthreads();
            const int g = g0 + cl;
            if (tr < R && g < DG) {
                const int d = g * 4;
                float m[4], sc[4] = {1.f, 1.f, 1.f, 1.f}, sh[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int e = 0; e < 4; ++e) m[e] = msk[cl * 4 + e];
                const bool affine = mode == PTTS_IN_LRELU && scale != nullptr;
                if (affine) {
#pragma unroll
                    for (int e = 0; e < 4; ++e)
                        if (d + e < D) { sc[e] = scale[d + e]; sh[e] = shift[d + e]; }
                }
                for (int t = t_lo + tr; t < t_hi; t += R) {
                    const long long off = ((long long)b * T + t) * D + d;
                    float v[4];
                    if (VEC) {
                        const float4 q = *reinterpret_cast<const float4*>(x + off);
                        v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
                    } else {
#pragma unroll
                        for (int e = 0; e < 4; ++e) v[e] = d + e < D ? x[off + e] : 0.f;
                    }
                    if (mode == PTTS_IN_LRELU) {
#pragma unroll
                        for (int e = 0; e < 4; ++e) {
                            const float p = affine ? v[e] * sc[e] + sh[e] : v[e];
                            v[e] = lrelu(p, alpha);
                        }
                    }
#pragma unroll
                    for (int e = 0; e < 4; ++e) v[e] *= m[e];
                    if (VEC) {
                        *reinterpret_cast<float4*>(y + off) = make_float4(v[0], v[1], v[2], v[3]);
                    } else {
#pragma unroll
                        for (int e = 0; e < 4; ++e)
                            if (d + e < D) y[off + e] = v[e];
                    }
                }
            }
            __syncthreads();
        }
    }
}

static int dropout_launch(const char* what, bool fwd, const float* x, const float* scale, const float* shift, float* y,
                          const u64* state, u64* used, float rate, float alpha, int mode, int B, int T, int D, long long b0,
                          hipStream_t st) {
    const int DG = (D + 3) / 4;
    const int CGW = DG < DO_THREADS ? DG : DO_THREADS;
    const int R = DO_THREADS / CGW;
    // about 2048 workgroups (256 CUs x 8) where the tensor has them; a chunk is a whole number of R-row sweeps
    const int gy = B < 32768 ? B : 32768;
    long long chunks = (2048 + gy - 1) / gy;
    const long long sweeps = ((long long)T + R - 1) / R;
    if (chunks > sweeps) chunks = sweeps;
    const int rows_per_chunk = (int)((sweeps + chunks - 1) / chunks) * R;
    const int gx = (T + rows_per_chunk - 1) / rows_per_chunk;
    const float keep = 1.f - rate, inv_keep = 1.f / keep;
    const bool vec = D % 4 == 0 && (uintptr_t)x % 16 == 0 && (uintptr_t)y % 16 == 0;
    const dim3 grid(gx, gy), block(DO_THREADS);
#define PTTS_DO_LAUNCH(V, F)                                                                                                  \
    hipLaunchKernelGGL((dropout_kernel<V, F>), grid, block, 0, st, x, scale, shift, y, state, used, keep, inv_keep, alpha,    \
                       mode, B, T, D, b0, rows_per_chunk)
    if (vec) { if (fwd) PTTS_DO_LAUNCH(true, true); else PTTS_DO_LAUNCH(true, false); }
    else     { if (fwd) PTTS_DO_LAUNCH(false, true); else PTTS_DO_LAUNCH(false, false); }
#undef PTTS_DO_LAUNCH
    return check_launch(what);
}

constexpr int NF_THREADS = 256;

// One Philox block, four normals, one 16-byte store per lane and iteration.  Block kb covers the elements 4 kb .. 4 kb + 3 of the
// GLOBAL sequence; out[i] is element i0 + i, so the first and the last block of a launch may be partial (scalar stores).
__global__ __launch_bounds__(NF_THREADS) void normal_fill_kernel(
    float* __restrict__ out, const u64* __restrict__ state, u64* __restrict__ used, float stddev, long long i0, long long n) {
    const u64 seed = state[0], call = state[1];
    if (blockIdx.x == 0 && threadIdx.x == 0) used[0] = call;
    const long long kb_lo = i0 >> 2, kb_hi = (i0 + n - 1) >> 2;      // inclusive
    const bool aligned = (i0 & 3) == 0 && (uintptr_t)out % 16 == 0;
    for (long long kb = kb_lo + blockIdx.x * (long long)blockDim.x + threadIdx.x; kb <= kb_hi;
         kb += (long long)gridDim.x * blockDim.x) {
        const Philox4 p = philox4x32_10((u64)kb, call, seed);
        float z[4];
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const float r = stddev * sqrtf(-2.f * logf(u01_open0(p.w[2 * h])));
            float s, c;
            sincospif(2.f * u01(p.w[2 * h + 1]), &s, &c);
            z[2 * h] = r * c;
            z[2 * h + 1] = r * s;
        }
        const long long i = kb * 4 - i0;      // index in out of the block's first element (may be < 0 for the first block)
        if (aligned && i + 4 <= n) {
            *reinterpret_cast<float4*>(out + i) = make_float4(z[0], z[1], z[2], z[3]);
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e)
                if (i + e >= 0 && i + e < n) out[i + e] = z[e];
        }
    }
}

static int advance(u64* state, hipStream_t st, const char* what) {
    hipLaunchKernelGGL(rng_advance_kernel, dim3(1), dim3(1), 0, st, state);
    return check_launch(what);
}

}  // namespace ptts

using namespace ptts;

extern "C" int ptts_rng_seed(unsigned long long* state, unsigned long long seed, unsigned long long counter, void* stream) {
    PTTS_REQUIRE(state, "rng_seed: null state block");
    hipLaunchKernelGGL(rng_seed_kernel, dim3(1), dim3(1), 0, (hipStream_t)stream, state, seed, counter);
    return check_launch("rng_seed");
}

extern "C" int ptts_rng_state_get(const unsigned long long* state, unsigned long long* out_host, void* stream) {
    PTTS_REQUIRE(state && out_host, "rng_state_get: null pointer");
    hipError_t e = hipMemcpyAsync(out_host, state, 2 * sizeof(unsigned long long), hipMemcpyDeviceToHost, (hipStream_t)stream);
    if (e == hipSuccess) e = hipStreamSynchronize((hipStream_t)stream);
    if (e != hipSuccess) {
        set_error("rng_state_get: copy failed: %s", hipGetErrorString(e));
        return PTTS_ELAUNCH;
    }
    return PTTS_OK;
}

extern "C" int ptts_dropout_fwd(const float* x, const float* scale, const float* shift, float* y, unsigned long long* state,
                                unsigned long long* used, float rate, float alpha, int mode, int B, int T, int D,
                                long long b0, void* stream) {
    PTTS_REQUIRE(x && y && state && used, "dropout_fwd: null pointer");
    PTTS_REQUIRE(B >= 1 && T >= 1 && D >= 1 && b0 >= 0, "dropout_fwd: bad shape B=%d T=%d D=%d b0=%lld", B, T, D, b0);
    PTTS_REQUIRE(rate >= 0.f && rate < 1.f, "dropout_fwd: rate %g outside [0, 1)", (double)rate);
    PTTS_REQUIRE(mode == PTTS_IN_NONE || mode == PTTS_IN_LRELU, "dropout_fwd: unknown input mode %d", mode);
    PTTS_REQUIRE((scale == nullptr) == (shift == nullptr), "dropout_fwd: scale/shift must come together");
    PTTS_REQUIRE(mode == PTTS_IN_LRELU || scale == nullptr, "dropout_fwd: scale/shift need PTTS_IN_LRELU");
    hipStream_t st = (hipStream_t)stream;
    const int rc = dropout_launch("dropout_fwd", true, x, scale, shift, y, state, used, rate, alpha, mode, B, T, D, b0, st);
    if (rc != PTTS_OK) return rc;
    return advance(state, st, "dropout_fwd (counter)");
}

extern "C" int ptts_dropout_bwd(const float* dy, float* da, const unsigned long long* used, const unsigned long long* state,
                                float rate, int B, int T, int D, long long b0, void* stream) {
    PTTS_REQUIRE(dy && da && used && state, "dropout_bwd: null pointer");
    PTTS_REQUIRE(B >= 1 && T >= 1 && D >= 1 && b0 >= 0, "dropout_bwd: bad shape B=%d T=%d D=%d b0=%lld", B, T, D, b0);
    PTTS_REQUIRE(rate >= 0.f && rate < 1.f, "dropout_bwd: rate %g outside [0, 1)", (double)rate);
    return dropout_launch("dropout_bwd", false, dy, nullptr, nullptr, da, state, const_cast<unsigned long long*>(used), rate, 0.f,
                          PTTS_IN_NONE, B, T, D, b0, (hipStream_t)stream);
}

extern "C" int ptts_normal_fill(float* out, unsigned long long* state, unsigned long long* used, float stddev, long long i0,
                                long long n, void* stream) {
    PTTS_REQUIRE(out && state && used, "normal_fill: null pointer");
    PTTS_REQUIRE(n >= 1 && i0 >= 0, "normal_fill: bad range i0=%lld n=%lld", i0, n);
    PTTS_REQUIRE(stddev >= 0.f, "normal_fill: stddev %g < 0", (double)stddev);
    hipStream_t st = (hipStream_t)stream;
    const long long nblk = ((i0 + n - 1) >> 2) - (i0 >> 2) + 1;
    long long g = (nblk + NF_THREADS - 1) / NF_THREADS;
    if (g > 2048) g = 2048;
    hipLaunchKernelGGL(normal_fill_kernel, dim3((int)g), dim3(NF_THREADS), 0, st, out, state, used, stddev, i0, n);
    const int rc = check_launch("normal_fill");
    if (rc != PTTS_OK) return rc;
    return advance(state, st, "normal_fill (counter)");
}
