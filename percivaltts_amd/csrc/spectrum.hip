// Spectral envelope decompression and the mel-cepstral post-filter: the frame-wise part of the reference's vocoder.synthesis
// (vocoders.py:147-166 decompress_spectrum; external/merlin/generate_pp.py mcep_postproc_sptk, seven SPTK command lines through
// temporary files).  Notation: L = dftlen, K = L/2 + 1 bins, w_k = 2 pi k / L, warped frequency
//   wt_k = w_k + 2 atan2(alpha sin w_k, 1 - alpha cos w_k).
//
// mcep -> spectrum:      logA[t,k] = sum_m c[t,m] cos(m wt_k),   A = exp(logA)
// post-filter (pf):      c' = c * [1, 1, pf, pf, ...];  r0(c) = (1/L) (E_0 + E_{K-1} + 2 sum_{0<k<K-1} E_k),  E_k = exp(2 logA_k(c))
//                        out_0 = c_0 + ln(r0(c) / r0(c')) / 2,  out_m = c'_m  (m >= 1)
//                        logA_k(c') = pf logA_k(c) - (pf - 1) (c_0 + c_1 cos wt_k): both energies come from ONE product row.
// fwbnd -> spectrum:     logA[t,k] = linear interpolation (in Hz) of the nb band values at k fs / L, band centres
//                        f_b = 700 (exp(b mel(fs/2) / ((nb-1) 1127)) - 1), mel(f) = 1127 ln(1 + f/700)
// fwbnd post-filter:     with q_k the trapezoid weights of the nodes wt_k on [0, pi],
//                        c_0 = (1/pi) sum q_k logA_k,  c_1 = (2/pi) sum q_k logA_k cos wt_k,
//                        logA'_k = pf logA_k - (pf - 1) (c_0 + c_1 cos wt_k),  A_k = exp(logA'_k + ln(r0(logA) / r0(logA')) / 2)
//
// The product logA = c . cos(m wt_k) is a [T, M1] x [M1, K] matrix product whose second operand depends on (alpha, dftlen, M1)
// only: ptts_mcep_table builds it once ([M1][Kp] fp32, Kp = K rounded up to 4, zero beyond K; cos in fp64, rounded once), the
// caller keeps it.  A workgroup takes SPEC_TT consecutive frames over all bins; a thread holds SPEC_TT x 4 fp64 accumulators
// (4 consecutive bins), so one 16-byte table load feeds 32 fp64 FMAs and the cepstra are broadcast from LDS.  Accumulation, exp
// and log are fp64, the result is rounded to fp32 once: the table's rounding (2^-25 per term, m >= 1) is what is left besides.
// A frame's reductions (energies, c_0 / c_1) stay inside its workgroup: wave butterflies, then the waves' partials added in wave
// order through LDS.  No atomics; a frame's result does not depend on T, on its position or on what else is in the batch.
// With the post-filter the spectrum kernels recompute the product for the store pass instead of keeping [frames, K] values.
//
// spectrum -> mcep:      with v_k = ln max(|x_k|, FLT_MIN) (or x_k, a logarithm already), C[m,k] = cos(m wt_k), q_k as above:
//                        c = argmin sum_k q_k (v_k - sum_m c_m C[m,k])^2 = W v,  W = G^-1 C diag(q),  G = C diag(q) C^T
//                        the exact left inverse of mcep -> spectrum (log) for a cepstrum of the same order.  G is well conditioned
//                        (cond about 2) while M1 <= floor((L/2) (1 - |alpha|) / (1 + |alpha|)): beyond that the widest node
//                        spacing on the warped axis no longer resolves cos(m wt) and G turns singular.
// W depends on (M1, alpha, dftlen) only: ptts_spec2mcep_table builds it once, in fp64 throughout.  The nodes wt_k, q_k; the sums
// S_n = sum_k q_k cos(n wt_k), n <= 2 M1 - 2, which hold all of G because cos a cos b = (cos(a - b) + cos(a + b)) / 2; the
// Cholesky factor of G in one workgroup (left-looking, a thread owns a row); W by a forward and a backward substitution per bin
// column, S2M_BN columns per workgroup with the right-hand sides in LDS.  The factor is stored mirrored, A[c][r] = L[max][min],
// so that both substitutions read the contiguous column A[j][.] at step j.
// The fit itself is a [T, K] x [K, M1] product with K the reduction axis: a workgroup takes SPEC_TT frames, stages their v over
// S2M_KC bins in LDS as fp64 (one log per element), and a thread owns one coefficient m and every (256 / MW)-th bin of the chunk,
// MW = M1 rounded up to a power of two (256 at the most; beyond it blockIdx.y picks the coefficients).  W is stored [K][M1p] so
// that the threads of a bin read neighbouring addresses.  A coefficient's partial sums meet in a fixed order: butterflies between
// the lanes of a wave that share m, then the groups' partials in group order through LDS.
//
// Rows of the output are K floats long and K is odd, so only every fourth row starts on a 16-byte boundary: the stores are
// 16 bytes wide with 4-byte alignment (dword-aligned vector stores are legal on gfx950 global memory); a wave's store covers one
// contiguous KiB.
#include "common.h"

namespace ptts {

constexpr int SPEC_TT = 8;              // frames per workgroup
constexpr int SPEC_MAX_THREADS = 256;   // a thread owns 4 consecutive bins of every pass of 4 * blockDim.x bins
constexpr int SPEC_MAX_M1 = 512;        // cepstra staged in LDS as fp64 [M1][SPEC_TT]: 32 KiB at the most
constexpr int SPEC_MAX_NB = 1024;       // bands staged in LDS as fp32 [SPEC_TT][nb]: 32 KiB at the most
constexpr int SPEC_MAX_DFTLEN = 1 << 20;
constexpr int FW_ROWS = 4;              // rows of the fwbnd table: band index, fraction, cos wt_k, q_k
constexpr double SPEC_PI = 3.14159265358979323846;
constexpr double SPEC_FLT_MIN = 1.17549435082228751e-38;
constexpr int S2M_KC = 256;             // bins of a staged chunk of ptts_spec2mcep: fp64 [S2M_KC][SPEC_TT], 16 KiB
constexpr int S2M_BN = 8;               // bin columns a workgroup of the table's substitutions solves
constexpr size_t S2M_MAX_TABLE_BYTES = (size_t)32 << 20;    // W and the scratch behind it

typedef float f32x4_a4 __attribute__((ext_vector_type(4), aligned(4)));

__device__ __forceinline__ double warp_freq(int k, int L, double alpha) {
    const double w = 2.0 * SPEC_PI * (double)k / (double)L;
    return w + 2.0 * atan2(alpha * sin(w), 1.0 - alpha * cos(w));
}

// q_k: the trapezoid weight of node wt = wt_k among the nodes wt_0 .. wt_{K-1} on [0, pi]
__device__ __forceinline__ double warp_weight(int k, int K, int L, double alpha, double wt) {
    const double below = k > 0 ? warp_freq(k - 1, L, alpha) : wt, above = k < K - 1 ? warp_freq(k + 1, L, alpha) : wt;
    return 0.5 * (above - below);
}

// [M1][Kp] fp32: cos(m wt_k), 0 for K <= k < Kp
__global__ void mcep_table_kernel(float* __restrict__ tab, int M1, int K, int Kp, int L, double alpha) {
    const int k = blockIdx.x * blockDim.x + threadIdx.x, m = blockIdx.y;
    if (k >= Kp) return;
    tab[(size_t)m * Kp + k] = k < K ? (float)cos((double)m * warp_freq(k, L, alpha)) : 0.f;
}

__device__ __forceinline__ double band_centre(int b, int nb, double melmax) {
    return 700.0 * (exp((double)b * melmax / ((double)(nb - 1) * 1127.0)) - 1.0);
}

// [FW_ROWS][Kp] fp64: lower band b_k (0 .. nb-2), fraction in [0, 1], cos wt_k, q_k; zeros for K <= k < Kp
__global__ void fwbnd_table_kernel(double* __restrict__ tab, int nb, double fs, double alpha, int K, int Kp, int L) {
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= Kp) return;
    double idx = 0.0, frac = 0.0, cw = 0.0, q = 0.0;
    if (k < K) {
        const double melmax = 1127.0 * log(1.0 + 0.5 * fs / 700.0);
        const double f = (double)k * fs / (double)L;
        int b = (int)floor(1127.0 * log(1.0 + f / 700.0) / melmax * (double)(nb - 1));
        b = b < 0 ? 0 : (b > nb - 2 ? nb - 2 : b);
        while (b > 0 && f < band_centre(b, nb, melmax)) --b;
        while (b < nb - 2 && f >= band_centre(b + 1, nb, melmax)) ++b;
        const double lo = band_centre(b, nb, melmax), hi = band_centre(b + 1, nb, melmax);
        frac = (f - lo) / (hi - lo);
        frac = frac < 0.0 ? 0.0 : (frac > 1.0 ? 1.0 : frac);
        idx = (double)b;
        const double wt = warp_freq(k, L, alpha);
        cw = cos(wt);
        q = warp_weight(k, K, L, alpha, wt);
    }
    tab[k] = idx;
    tab[(size_t)Kp + k] = frac;
    tab[2 * (size_t)Kp + k] = cw;
    tab[3 * (size_t)Kp + k] = q;
}

// Sum v[t] over the workgroup, for NV vectors at once: butterflies inside the waves, the waves' partials through LDS in wave
// order.  Every thread gets the totals.  red: [SPEC_MAX_THREADS/64][NV][SPEC_TT].
template <int NV>
__device__ __forceinline__ void block_sums(double (&v)[NV][SPEC_TT], double* red) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nwaves = blockDim.x >> 6;
#pragma unroll
    for (int i = 0; i < NV; ++i)
#pragma unroll
        for (int t = 0; t < SPEC_TT; ++t) {
            const double s = wave_sum(v[i][t]);
            if (lane == 0) red[(wave * NV + i) * SPEC_TT + t] = s;
        }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < NV; ++i)
#pragma unroll
        for (int t = 0; t < SPEC_TT; ++t) {
            double s = red[i * SPEC_TT + t];
            for (int w = 1; w < nwaves; ++w) s += red[(w * NV + i) * SPEC_TT + t];
            v[i][t] = s;
        }
    __syncthreads();
}

// weight of bin k in r0's symmetric sum
__device__ __forceinline__ double r0_weight(int k, int K) { return (k == 0 || k == K - 1) ? 1.0 : 2.0; }

__device__ __forceinline__ void store_bins(float* __restrict__ row, int k0, int K, const double (&v)[4], bool log_out) {
    float o[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) o[j] = (float)(log_out ? v[j] : exp(v[j]));
    if (k0 + 3 < K) {
        f32x4_a4 q;
        q.x = o[0]; q.y = o[1]; q.z = o[2]; q.w = o[3];
        *reinterpret_cast<f32x4_a4*>(row + k0) = q;
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (k0 + j < K) row[k0 + j] = o[j];
    }
}

// logA of SPEC_TT frames x 4 bins from k0: acc[t][j] = sum_m sc[m][t] * tab[m][k0 + j]
__device__ __forceinline__ void mcep_product(const double* __restrict__ sc, const float* __restrict__ tab, int M1, int Kp, int k0,
                                             double (&acc)[SPEC_TT][4]) {
#pragma unroll
    for (int t = 0; t < SPEC_TT; ++t)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[t][j] = 0.0;
    const float* tp = tab + k0;
#pragma unroll 2
    for (int m = 0; m < M1; ++m) {
        const float4 tv = *reinterpret_cast<const float4*>(tp + (size_t)m * Kp);
        const double d[4] = {(double)tv.x, (double)tv.y, (double)tv.z, (double)tv.w};
#pragma unroll
        for (int t = 0; t < SPEC_TT; ++t) {
            const double cv = sc[m * SPEC_TT + t];
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[t][j] = fma(cv, d[j], acc[t][j]);
        }
    }
}

// One workgroup: frames blockIdx.x * SPEC_TT ..., every bin.  SPEC = false: out [T, M1], the post-filtered cepstrum.
// SPEC = true: out [T, K], the envelope (log_out: its logarithm), post-filtered when `postfilter`.
// dynamic LDS: M1 * SPEC_TT doubles.
template <bool SPEC>
__global__ __launch_bounds__(SPEC_MAX_THREADS) void mcep_kernel(const float* __restrict__ mcep, const float* __restrict__ tab,
                                                                float* __restrict__ out, const int T, const int M1, const int K,
                                                                const int Kp, const bool log_out, const bool postfilter,
                                                                const double pf) {
    extern __shared__ double sc[];                                  // [M1][SPEC_TT]; frames behind T are zeros
    __shared__ double red[(SPEC_MAX_THREADS / 64) * 2 * SPEC_TT];
    const int tid = threadIdx.x, nthr = blockDim.x;
    const long long t0 = (long long)blockIdx.x * SPEC_TT;
    for (int i = tid; i < M1 * SPEC_TT; i += nthr) {
        const int t = i / M1, m = i - t * M1;
        sc[m * SPEC_TT + t] = t0 + t < T ? (double)mcep[(size_t)(t0 + t) * M1 + m] : 0.0;
    }
    __syncthreads();

    double delta[SPEC_TT];
#pragma unroll
    for (int t = 0; t < SPEC_TT; ++t) delta[t] = 0.0;
    if (!SPEC || postfilter) {
        double e[2][SPEC_TT];
#pragma unroll
        for (int t = 0; t < SPEC_TT; ++t) e[0][t] = e[1][t] = 0.0;
        for (int k0 = tid * 4; k0 < K; k0 += nthr * 4) {
            double acc[SPEC_TT][4];
            mcep_product(sc, tab, M1, Kp, k0, acc);
            const float4 c1 = *reinterpret_cast<const float4*>(tab + (size_t)Kp + k0);      // cos wt_k
            const double cw[4] = {(double)c1.x, (double)c1.y, (double)c1.z, (double)c1.w};
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                if (k0 + j < K) {
                    const double w = r0_weight(k0 + j, K);
#pragma unroll
                    for (int t = 0; t < SPEC_TT; ++t) {
                        const double la = acc[t][j];
                        const double lb = pf * la - (pf - 1.0) * fma(sc[SPEC_TT + t], cw[j], sc[t]);
                        e[0][t] += w * exp(2.0 * la);
                        e[1][t] += w * exp(2.0 * lb);
                    }
                }
            }
        }
        block_sums<2>(e, red);
#pragma unroll
        for (int t = 0; t < SPEC_TT; ++t) delta[t] = 0.5 * log(e[0][t] / e[1][t]);
    }

    if (!SPEC) {
        // thread t < SPEC_TT parks its frame's delta where the row writers find it
        if (tid < SPEC_TT) {
#pragma unroll
            for (int t = 0; t < SPEC_TT; ++t)
                if (t == tid) red[t] = delta[t];
        }
        __syncthreads();
        for (int i = tid; i < M1 * SPEC_TT; i += nthr) {
            const int t = i / M1, m = i - t * M1;
            if (t0 + t < T) {
                const double c = sc[m * SPEC_TT + t];
                out[(size_t)(t0 + t) * M1 + m] = (float)(m == 0 ? c + red[t] : (m == 1 ? c : pf * c));
            }
        }
        return;
    }

    for (int k0 = tid * 4; k0 < K; k0 += nthr * 4) {
        double acc[SPEC_TT][4];
        mcep_product(sc, tab, M1, Kp, k0, acc);
        double cw[4] = {0.0, 0.0, 0.0, 0.0};
        if (postfilter) {
            const float4 c1 = *reinterpret_cast<const float4*>(tab + (size_t)Kp + k0);
            cw[0] = (double)c1.x; cw[1] = (double)c1.y; cw[2] = (double)c1.z; cw[3] = (double)c1.w;
        }
#pragma unroll
        for (int t = 0; t < SPEC_TT; ++t) {
            if (t0 + t < T) {
                double v[4];
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    v[j] = postfilter ? (pf * acc[t][j] - (pf - 1.0) * fma(sc[SPEC_TT + t], cw[j], sc[t])) + delta[t] : acc[t][j];
                store_bins(out + (size_t)(t0 + t) * K, k0, K, v, log_out);
            }
        }
    }
}

// logA of SPEC_TT frames x 4 bins from k0 by interpolation between the bands; sf [SPEC_TT][nb]
__device__ __forceinline__ void fwbnd_interp(const float* __restrict__ sf, const double* __restrict__ tab, int nb, int Kp, int k0,
                                             double (&la)[SPEC_TT][4]) {
    const double4 bi = *reinterpret_cast<const double4*>(tab + k0);
    const double4 fr = *reinterpret_cast<const double4*>(tab + (size_t)Kp + k0);
    int b[4] = {(int)bi.x, (int)bi.y, (int)bi.z, (int)bi.w};
#pragma unroll
    for (int j = 0; j < 4; ++j) b[j] = b[j] < 0 ? 0 : (b[j] > nb - 2 ? nb - 2 : b[j]);      // whatever the table holds
    const double f[4] = {fr.x, fr.y, fr.z, fr.w};
#pragma unroll
    for (int t = 0; t < SPEC_TT; ++t)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const double lo = (double)sf[t * nb + b[j]], hi = (double)sf[t * nb + b[j] + 1];
            la[t][j] = fma(f[j], hi - lo, lo);
        }
}

// dynamic LDS: SPEC_TT * nb floats
__global__ __launch_bounds__(SPEC_MAX_THREADS) void fwbnd_kernel(const float* __restrict__ fw, const double* __restrict__ tab,
                                                                 float* __restrict__ out, const int T, const int nb, const int K,
                                                                 const int Kp, const bool log_out, const bool postfilter,
                                                                 const double pf) {
    extern __shared__ float sf[];                                   // [SPEC_TT][nb]; frames behind T are zeros
    __shared__ double red[(SPEC_MAX_THREADS / 64) * 2 * SPEC_TT];
    const int tid = threadIdx.x, nthr = blockDim.x;
    const long long t0 = (long long)blockIdx.x * SPEC_TT;
    for (int i = tid; i < nb * SPEC_TT; i += nthr) {
        const int t = i / nb;
        sf[i] = t0 + t < T ? fw[(size_t)t0 * nb + i] : 0.f;
    }
    __syncthreads();

    double c0[SPEC_TT], c1[SPEC_TT], delta[SPEC_TT];
#pragma unroll
    for (int t = 0; t < SPEC_TT; ++t) c0[t] = c1[t] = delta[t] = 0.0;
    if (postfilter) {
        double s[2][SPEC_TT];
#pragma unroll
        for (int t = 0; t < SPEC_TT; ++t) s[0][t] = s[1][t] = 0.0;
        for (int k0 = tid * 4; k0 < K; k0 += nthr * 4) {
            double la[SPEC_TT][4];
            fwbnd_interp(sf, tab, nb, Kp, k0, la);
            const double4 cw4 = *reinterpret_cast<const double4*>(tab + 2 * (size_t)Kp + k0);
            const double4 q4 = *reinterpret_cast<const double4*>(tab + 3 * (size_t)Kp + k0);
            const double cw[4] = {cw4.x, cw4.y, cw4.z, cw4.w}, q[4] = {q4.x, q4.y, q4.z, q4.w};      // q = 0 beyond K
#pragma unroll
            for (int j = 0; j < 4; ++j)
#pragma unroll
                for (int t = 0; t < SPEC_TT; ++t) {
                    const double ql = q[j] * la[t][j];
                    s[0][t] += ql;
                    s[1][t] += ql * cw[j];
                }
        }
        block_sums<2>(s, red);
#pragma unroll
        for (int t = 0; t < SPEC_TT; ++t) { c0[t] = s[0][t] / SPEC_PI; c1[t] = 2.0 * s[1][t] / SPEC_PI; }

        double e[2][SPEC_TT];
#pragma unroll
        for (int t = 0; t < SPEC_TT; ++t) e[0][t] = e[1][t] = 0.0;
        for (int k0 = tid * 4; k0 < K; k0 += nthr * 4) {
            double la[SPEC_TT][4];
            fwbnd_interp(sf, tab, nb, Kp, k0, la);
            const double4 cw4 = *reinterpret_cast<const double4*>(tab + 2 * (size_t)Kp + k0);
            const double cw[4] = {cw4.x, cw4.y, cw4.z, cw4.w};
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                if (k0 + j < K) {
                    const double w = r0_weight(k0 + j, K);
#pragma unroll
                    for (int t = 0; t < SPEC_TT; ++t) {
                        const double lb = pf * la[t][j] - (pf - 1.0) * fma(c1[t], cw[j], c0[t]);
                        e[0][t] += w * exp(2.0 * la[t][j]);
                        e[1][t] += w * exp(2.0 * lb);
                    }
                }
            }
        }
        block_sums<2>(e, red);
#pragma unroll
        for (int t = 0; t < SPEC_TT; ++t) delta[t] = 0.5 * log(e[0][t] / e[1][t]);
    }

    for (int k0 = tid * 4; k0 < K; k0 += nthr * 4) {
        double la[SPEC_TT][4];
        fwbnd_interp(sf, tab, nb, Kp, k0, la);
        double cw[4] = {0.0, 0.0, 0.0, 0.0};
        if (postfilter) {
            const double4 cw4 = *reinterpret_cast<const double4*>(tab + 2 * (size_t)Kp + k0);
            cw[0] = cw4.x; cw[1] = cw4.y; cw[2] = cw4.z; cw[3] = cw4.w;
        }
#pragma unroll
        for (int t = 0; t < SPEC_TT; ++t) {
            if (t0 + t < T) {
                double v[4];
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    v[j] = postfilter ? (pf * la[t][j] - (pf - 1.0) * fma(c1[t], cw[j], c0[t])) + delta[t] : la[t][j];
                store_bins(out + (size_t)(t0 + t) * K, k0, K, v, log_out);
            }
        }
    }
}

// ---- spectrum -> mcep: the table ----
// nodes [2][Kp] fp64: wt_k, q_k; zeros for K <= k < Kp
__global__ void s2m_nodes_kernel(double* __restrict__ nodes, int K, int Kp, int L, double alpha) {
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= Kp) return;
    double wt = 0.0, q = 0.0;
    if (k < K) {
        wt = warp_freq(k, L, alpha);
        q = warp_weight(k, K, L, alpha, wt);
    }
    nodes[k] = wt;
    nodes[(size_t)Kp + k] = q;
}

// S[n] = sum_k q_k cos(n wt_k), one workgroup per n: butterflies, then the waves' partials in wave order
__global__ __launch_bounds__(SPEC_MAX_THREADS) void s2m_sums_kernel(const double* __restrict__ nodes, double* __restrict__ S, int K,
                                                                   int Kp) {
    __shared__ double red[SPEC_MAX_THREADS / 64];
    const int tid = threadIdx.x, n = blockIdx.x;
    double s = 0.0;
    for (int k = tid; k < K; k += SPEC_MAX_THREADS) s += nodes[(size_t)Kp + k] * cos((double)n * nodes[k]);
    s = wave_sum(s);
    if ((tid & 63) == 0) red[tid >> 6] = s;
    __syncthreads();
    if (tid == 0) {
        double t = red[0];
        for (int w = 1; w < SPEC_MAX_THREADS / 64; ++w) t += red[w];
        S[n] = t;
    }
}

// One workgroup.  A [M1][M1]: G[r][c] = (S[r-c] + S[r+c]) / 2 goes to A[c][r], r >= c, and is factored in place, G = L L^T,
// left-looking: at column j the thread of row i >= j subtracts sum_{k<j} L[i][k] L[j][k] (A[k][i]: neighbouring threads,
// neighbouring addresses).  L[i][j] is stored at A[j][i] and at A[i][j].  M1 <= 2 * SPEC_MAX_THREADS rows.
__global__ __launch_bounds__(SPEC_MAX_THREADS) void s2m_factor_kernel(const double* __restrict__ S, double* A, int M1) {
    __shared__ double pivot;
    const int tid = threadIdx.x;
    for (int idx = tid; idx < M1 * M1; idx += SPEC_MAX_THREADS) {
        const int c = idx / M1, r = idx - c * M1;
        if (r >= c) A[idx] = 0.5 * (S[r - c] + S[r + c]);
    }
    __syncthreads();
    for (int j = 0; j < M1; ++j) {
        double s[2] = {0.0, 0.0};
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const int i = j + tid + u * SPEC_MAX_THREADS;
            if (i < M1) {
                double acc = A[(size_t)j * M1 + i];
                for (int k = 0; k < j; ++k) acc -= A[(size_t)k * M1 + i] * A[(size_t)k * M1 + j];
                s[u] = acc;
            }
        }
        if (tid == 0) pivot = sqrt(s[0]);       // row j itself
        __syncthreads();
        const double d = pivot;
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const int i = j + tid + u * SPEC_MAX_THREADS;
            if (i < M1) {
                const double v = i == j ? d : s[u] / d;
                A[(size_t)j * M1 + i] = v;
                A[(size_t)i * M1 + j] = v;
            }
        }
        __syncthreads();
    }
}

// W[k][.] = G^-1 (q_k cos(m wt_k))_m for the S2M_BN bins from blockIdx.x * S2M_BN: L y = b, then L^T x = y, column-oriented, the
// right-hand sides B [M1][S2M_BN] in LDS (dynamic: M1 * S2M_BN doubles).  A thread owns a bin and every (256 / S2M_BN)-th row;
// the pivot's division is repeated by every thread that needs it and written once, after the sweep.
__global__ __launch_bounds__(SPEC_MAX_THREADS) void s2m_solve_kernel(const double* __restrict__ nodes, const double* __restrict__ A,
                                                                    double* __restrict__ W, int M1, int M1p, int K, int Kp) {
    extern __shared__ double B[];
    constexpr int NR = SPEC_MAX_THREADS / S2M_BN;
    const int tid = threadIdx.x, b = tid % S2M_BN, r = tid / S2M_BN;
    const int k0 = blockIdx.x * S2M_BN;
    for (int i = tid; i < M1 * S2M_BN; i += SPEC_MAX_THREADS) {
        const int m = i / S2M_BN, k = k0 + i % S2M_BN;
        B[i] = k < K ? nodes[(size_t)Kp + k] * cos((double)m * nodes[k]) : 0.0;
    }
    __syncthreads();
    for (int j = 0; j < M1; ++j) {
        const double* col = A + (size_t)j * M1;
        const double xj = B[j * S2M_BN + b] / col[j];
        for (int i = j + 1 + r; i < M1; i += NR) B[i * S2M_BN + b] -= col[i] * xj;
        __syncthreads();
    }
    for (int i = tid; i < M1 * S2M_BN; i += SPEC_MAX_THREADS) {
        const int m = i / S2M_BN;
        B[i] /= A[(size_t)m * M1 + m];
    }
    __syncthreads();
    for (int j = M1 - 1; j >= 0; --j) {
        const double* col = A + (size_t)j * M1;                     // col[i] = L[j][i] for i < j
        const double xj = B[j * S2M_BN + b] / col[j];
        for (int i = r; i < j; i += NR) B[i * S2M_BN + b] -= col[i] * xj;
        __syncthreads();
    }
    for (int i = tid; i < M1p * S2M_BN; i += SPEC_MAX_THREADS) {
        const int bb = i / M1p, m = i - bb * M1p, k = k0 + bb;
        if (k < K) W[(size_t)k * M1p + m] = m < M1 ? B[m * S2M_BN + bb] / A[(size_t)m * M1 + m] : 0.0;
    }
}

// ---- spectrum -> mcep: the product ----
// One workgroup of SPEC_MAX_THREADS threads: frames blockIdx.x * SPEC_TT ..., coefficients blockIdx.y * MW ... (MW a power of
// two, 2 .. 256).  Thread tid: coefficient tid % MW, bins tid / MW, + 256 / MW, ... of every chunk.
__global__ __launch_bounds__(SPEC_MAX_THREADS) void spec2mcep_kernel(const float* __restrict__ x, const double* __restrict__ W,
                                                                    float* __restrict__ out, const int T, const int M1,
                                                                    const int M1p, const int K, const int MW, const bool is_log) {
    __shared__ double sv[S2M_KC * SPEC_TT];                         // [bin][frame]; frames behind T and bins behind K are zeros
    __shared__ double red[SPEC_MAX_THREADS * SPEC_TT];              // [group][MW][SPEC_TT], groups * MW <= SPEC_MAX_THREADS
    const int tid = threadIdx.x;
    const int ml = tid & (MW - 1), slice = tid / MW, nslices = SPEC_MAX_THREADS / MW;
    const int m = blockIdx.y * MW + ml;
    const long long t0 = (long long)blockIdx.x * SPEC_TT;
    double acc[SPEC_TT];
#pragma unroll
    for (int t = 0; t < SPEC_TT; ++t) acc[t] = 0.0;

    for (int k0 = 0; k0 < K; k0 += S2M_KC) {
        const int nk = K - k0 < S2M_KC ? K - k0 : S2M_KC;
        __syncthreads();                                            // the chunk before is used up
        for (int i = tid; i < S2M_KC * SPEC_TT; i += SPEC_MAX_THREADS) {
            const int t = i / S2M_KC, kk = i - t * S2M_KC;
            double v = 0.0;
            if (t0 + t < T && kk < nk) {
                v = (double)x[(size_t)(t0 + t) * K + k0 + kk];
                if (!is_log) {
                    v = fabs(v);
                    v = log(v > SPEC_FLT_MIN ? v : SPEC_FLT_MIN);
                }
            }
            sv[kk * SPEC_TT + t] = v;
        }
        __syncthreads();
        if (m < M1) {
            const double* wp = W + (size_t)k0 * M1p + m;
            for (int kk = slice; kk < nk; kk += nslices) {
                const double w = wp[(size_t)kk * M1p];
#pragma unroll
                for (int t = 0; t < SPEC_TT; ++t) acc[t] = fma(w, sv[kk * SPEC_TT + t], acc[t]);
            }
        }
    }

    // the slices of one coefficient: first those inside a wave (MW < 64), then one partial per group of max(MW, 64) threads
    const int GW = MW > 64 ? MW : 64, group = tid / GW, ngroups = SPEC_MAX_THREADS / GW;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1)
        if (o >= MW) {
#pragma unroll
            for (int t = 0; t < SPEC_TT; ++t) acc[t] += __shfl_xor(acc[t], o, 64);
        }
    if (tid - group * GW < MW) {
#pragma unroll
        for (int t = 0; t < SPEC_TT; ++t) red[(group * MW + ml) * SPEC_TT + t] = acc[t];
    }
    __syncthreads();
    for (int i = tid; i < MW * SPEC_TT; i += SPEC_MAX_THREADS) {
        const int t = i / MW, c = i - t * MW, mo = blockIdx.y * MW + c;
        if (mo < M1 && t0 + t < T) {
            double s = red[c * SPEC_TT + t];
            for (int g = 1; g < ngroups; ++g) s += red[(g * MW + c) * SPEC_TT + t];
            out[(size_t)(t0 + t) * M1 + mo] = (float)s;
        }
    }
}

static int spec_padded_bins(int dftlen) { return (dftlen / 2 + 1 + 3) / 4 * 4; }

// threads of a workgroup: one per 4 bins, whole waves, at most SPEC_MAX_THREADS
static int spec_threads(int K) {
    const int want = ((K + 3) / 4 + 63) / 64 * 64;
    return want > SPEC_MAX_THREADS ? SPEC_MAX_THREADS : want;
}

static bool spec_dftlen_ok(int dftlen) { return dftlen >= 8 && dftlen % 2 == 0 && dftlen <= SPEC_MAX_DFTLEN; }
static bool spec_alpha_ok(double alpha) { return alpha > -1.0 && alpha < 1.0; }

}  // namespace ptts

using namespace ptts;

extern "C" size_t ptts_mcep_table_bytes(int M1, int dftlen) {
    if (M1 < 2 || M1 > SPEC_MAX_M1 || !spec_dftlen_ok(dftlen)) return 16;
    return align_up((size_t)M1 * spec_padded_bins(dftlen) * sizeof(float), 256);
}

extern "C" int ptts_mcep_table(float* table, size_t table_bytes, int M1, double alpha, int dftlen, void* stream) {
    PTTS_REQUIRE(M1 >= 2 && M1 <= SPEC_MAX_M1, "mcep_table: M1=%d outside [2, %d]", M1, SPEC_MAX_M1);
    PTTS_REQUIRE(spec_dftlen_ok(dftlen), "mcep_table: dftlen=%d (even, 8 .. %d)", dftlen, SPEC_MAX_DFTLEN);
    PTTS_REQUIRE(spec_alpha_ok(alpha), "mcep_table: |alpha|=%g is not below 1", alpha);
    PTTS_REQUIRE(table && ((size_t)table & 15) == 0, "mcep_table: null or unaligned table");
    PTTS_REQUIRE(table_bytes >= ptts_mcep_table_bytes(M1, dftlen), "mcep_table: table %zu < %zu bytes", table_bytes,
                 ptts_mcep_table_bytes(M1, dftlen));
    const int K = dftlen / 2 + 1, Kp = spec_padded_bins(dftlen);
    hipLaunchKernelGGL(mcep_table_kernel, dim3((Kp + 255) / 256, M1), dim3(256), 0, (hipStream_t)stream, table, M1, K, Kp, dftlen,
                       alpha);
    return check_launch("mcep_table");
}

extern "C" size_t ptts_fwbnd_table_bytes(int dftlen) {
    if (!spec_dftlen_ok(dftlen)) return 16;
    return align_up((size_t)FW_ROWS * spec_padded_bins(dftlen) * sizeof(double), 256);
}

extern "C" int ptts_fwbnd_table(double* table, size_t table_bytes, int nb, double fs, double alpha, int dftlen, void* stream) {
    PTTS_REQUIRE(nb >= 2 && nb <= SPEC_MAX_NB, "fwbnd_table: nb=%d outside [2, %d]", nb, SPEC_MAX_NB);
    PTTS_REQUIRE(fs > 0.0 && fs < 1e9, "fwbnd_table: fs=%g", fs);
    PTTS_REQUIRE(spec_dftlen_ok(dftlen), "fwbnd_table: dftlen=%d (even, 8 .. %d)", dftlen, SPEC_MAX_DFTLEN);
    PTTS_REQUIRE(spec_alpha_ok(alpha), "fwbnd_table: |alpha|=%g is not below 1", alpha);
    PTTS_REQUIRE(table && ((size_t)table & 31) == 0, "fwbnd_table: null or unaligned table");
    PTTS_REQUIRE(table_bytes >= ptts_fwbnd_table_bytes(dftlen), "fwbnd_table: table %zu < %zu bytes", table_bytes,
                 ptts_fwbnd_table_bytes(dftlen));
    const int K = dftlen / 2 + 1, Kp = spec_padded_bins(dftlen);
    hipLaunchKernelGGL(fwbnd_table_kernel, dim3((Kp + 255) / 256), dim3(256), 0, (hipStream_t)stream, table, nb, fs, alpha, K, Kp,
                       dftlen);
    return check_launch("fwbnd_table");
}

// the checks the three mcep entry points share; 1: nothing to do
static int mcep_args(const char* what, const void* in, const void* out, int T, int M1, double alpha, int dftlen, double pf_coef,
                     const float* table, size_t table_bytes) {
    PTTS_REQUIRE(T >= 0, "%s: T=%d", what, T);
    PTTS_REQUIRE(M1 >= 2 && M1 <= SPEC_MAX_M1, "%s: M1=%d outside [2, %d] (the post-filter's weights start 1 1)", what, M1, SPEC_MAX_M1);
    PTTS_REQUIRE(spec_dftlen_ok(dftlen), "%s: dftlen=%d (even, 8 .. %d)", what, dftlen, SPEC_MAX_DFTLEN);
    PTTS_REQUIRE(spec_alpha_ok(alpha), "%s: |alpha|=%g is not below 1", what, alpha);
    PTTS_REQUIRE(pf_coef > 0.0 && pf_coef < 1e6, "%s: pf_coef=%g", what, pf_coef);
    if (T == 0) return 1;
    PTTS_REQUIRE(in && out && table, "%s: null tensor", what);
    PTTS_REQUIRE(((size_t)table & 15) == 0 && table_bytes >= ptts_mcep_table_bytes(M1, dftlen),
                 "%s: the table of ptts_mcep_table(M1=%d, dftlen=%d) needs %zu aligned bytes, got %zu", what, M1, dftlen,
                 ptts_mcep_table_bytes(M1, dftlen), table_bytes);
    return 0;
}

extern "C" int ptts_mcep_postfilter(const float* mcep, float* out, int T, int M1, double alpha, int dftlen, double pf_coef,
                                    const float* table, size_t table_bytes, void* stream) {
    const int rc = mcep_args("mcep_postfilter", mcep, out, T, M1, alpha, dftlen, pf_coef, table, table_bytes);
    if (rc != 0) return rc < 0 ? rc : PTTS_OK;
    const int K = dftlen / 2 + 1;
    hipLaunchKernelGGL((mcep_kernel<false>), dim3((T + SPEC_TT - 1) / SPEC_TT), dim3(spec_threads(K)),
                       (size_t)M1 * SPEC_TT * sizeof(double), (hipStream_t)stream, mcep, table, out, T, M1, K,
                       spec_padded_bins(dftlen), false, true, pf_coef);
    return check_launch("mcep_postfilter");
}

extern "C" int ptts_mcep2spec(const float* mcep, float* spec, int T, int M1, double alpha, int dftlen, int log_out, int postfilter,
                              double pf_coef, const float* table, size_t table_bytes, void* stream) {
    const int rc = mcep_args("mcep2spec", mcep, spec, T, M1, alpha, dftlen, pf_coef, table, table_bytes);
    if (rc != 0) return rc < 0 ? rc : PTTS_OK;
    const int K = dftlen / 2 + 1;
    hipLaunchKernelGGL((mcep_kernel<true>), dim3((T + SPEC_TT - 1) / SPEC_TT), dim3(spec_threads(K)),
                       (size_t)M1 * SPEC_TT * sizeof(double), (hipStream_t)stream, mcep, table, spec, T, M1, K,
                       spec_padded_bins(dftlen), log_out != 0, postfilter != 0, pf_coef);
    return check_launch("mcep2spec");
}

extern "C" int ptts_fwbnd2spec(const float* fw, float* spec, int T, int nb, double fs, double alpha, int dftlen, int log_out,
                               int postfilter, double pf_coef, const double* table, size_t table_bytes, void* stream) {
    PTTS_REQUIRE(T >= 0, "fwbnd2spec: T=%d", T);
    PTTS_REQUIRE(nb >= 2 && nb <= SPEC_MAX_NB, "fwbnd2spec: nb=%d outside [2, %d]", nb, SPEC_MAX_NB);
    PTTS_REQUIRE(fs > 0.0 && fs < 1e9, "fwbnd2spec: fs=%g", fs);
    PTTS_REQUIRE(spec_dftlen_ok(dftlen), "fwbnd2spec: dftlen=%d (even, 8 .. %d)", dftlen, SPEC_MAX_DFTLEN);
    PTTS_REQUIRE(spec_alpha_ok(alpha), "fwbnd2spec: |alpha|=%g is not below 1", alpha);
    PTTS_REQUIRE(pf_coef > 0.0 && pf_coef < 1e6, "fwbnd2spec: pf_coef=%g", pf_coef);
    if (T == 0) return PTTS_OK;
    PTTS_REQUIRE(fw && spec && table, "fwbnd2spec: null tensor");
    PTTS_REQUIRE(((size_t)table & 31) == 0 && table_bytes >= ptts_fwbnd_table_bytes(dftlen),
                 "fwbnd2spec: the table of ptts_fwbnd_table(dftlen=%d) needs %zu aligned bytes, got %zu", dftlen,
                 ptts_fwbnd_table_bytes(dftlen), table_bytes);
    const int K = dftlen / 2 + 1;
    hipLaunchKernelGGL(fwbnd_kernel, dim3((T + SPEC_TT - 1) / SPEC_TT), dim3(spec_threads(K)), (size_t)nb * SPEC_TT * sizeof(float),
                       (hipStream_t)stream, fw, table, spec, T, nb, K, spec_padded_bins(dftlen), log_out != 0, postfilter != 0,
                       pf_coef);
    return check_launch("fwbnd2spec");
}

// the table of ptts_spec2mcep_table in doubles: W [K][M1p], the nodes [2][Kp], S [2 M1p], A [M1][M1]
static int s2m_padded_order(int M1) { return (M1 + 3) / 4 * 4; }
static size_t s2m_nodes_offset(int M1, int dftlen) { return (size_t)(dftlen / 2 + 1) * s2m_padded_order(M1); }
static size_t s2m_sums_offset(int M1, int dftlen) { return s2m_nodes_offset(M1, dftlen) + 2 * (size_t)spec_padded_bins(dftlen); }
static size_t s2m_factor_offset(int M1, int dftlen) { return s2m_sums_offset(M1, dftlen) + 2 * (size_t)s2m_padded_order(M1); }

// the largest M1 whose G is well conditioned
static int s2m_order_limit(double alpha, int dftlen) {
    return (int)floor((double)(dftlen / 2) * (1.0 - fabs(alpha)) / (1.0 + fabs(alpha)));
}

extern "C" size_t ptts_spec2mcep_table_bytes(int M1, int dftlen) {
    if (M1 < 2 || M1 > SPEC_MAX_M1 || !spec_dftlen_ok(dftlen)) return 16;
    return align_up((s2m_factor_offset(M1, dftlen) + (size_t)M1 * M1) * sizeof(double), 256);
}

// the checks of (M1, alpha, dftlen) the two spec2mcep entry points share
static int s2m_args(const char* what, int M1, double alpha, int dftlen) {
    PTTS_REQUIRE(M1 >= 2 && M1 <= SPEC_MAX_M1, "%s: M1=%d outside [2, %d]", what, M1, SPEC_MAX_M1);
    PTTS_REQUIRE(spec_dftlen_ok(dftlen), "%s: dftlen=%d (even, 8 .. %d)", what, dftlen, SPEC_MAX_DFTLEN);
    PTTS_REQUIRE(spec_alpha_ok(alpha), "%s: |alpha|=%g is not below 1", what, alpha);
    PTTS_REQUIRE(M1 <= s2m_order_limit(alpha, dftlen),
                 "%s: M1=%d above floor((dftlen/2) (1 - |alpha|) / (1 + |alpha|)) = %d: the fit is singular beyond it", what, M1,
                 s2m_order_limit(alpha, dftlen));
    PTTS_REQUIRE(ptts_spec2mcep_table_bytes(M1, dftlen) <= S2M_MAX_TABLE_BYTES, "%s: the table of M1=%d, dftlen=%d takes %zu bytes, above %zu",
                 what, M1, dftlen, ptts_spec2mcep_table_bytes(M1, dftlen), S2M_MAX_TABLE_BYTES);
    return PTTS_OK;
}

extern "C" int ptts_spec2mcep_table(double* table, size_t table_bytes, int M1, double alpha, int dftlen, void* stream) {
    const int rc = s2m_args("spec2mcep_table", M1, alpha, dftlen);
    if (rc != PTTS_OK) return rc;
    PTTS_REQUIRE(table && ((size_t)table & 31) == 0, "spec2mcep_table: null or unaligned table");
    PTTS_REQUIRE(table_bytes >= ptts_spec2mcep_table_bytes(M1, dftlen), "spec2mcep_table: table %zu < %zu bytes", table_bytes,
                 ptts_spec2mcep_table_bytes(M1, dftlen));
    const int K = dftlen / 2 + 1, Kp = spec_padded_bins(dftlen), M1p = s2m_padded_order(M1);
    double* nodes = table + s2m_nodes_offset(M1, dftlen);
    double* S = table + s2m_sums_offset(M1, dftlen);
    double* A = table + s2m_factor_offset(M1, dftlen);
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(s2m_nodes_kernel, dim3((Kp + 255) / 256), dim3(256), 0, st, nodes, K, Kp, dftlen, alpha);
    hipLaunchKernelGGL(s2m_sums_kernel, dim3(2 * M1 - 1), dim3(SPEC_MAX_THREADS), 0, st, nodes, S, K, Kp);
    hipLaunchKernelGGL(s2m_factor_kernel, dim3(1), dim3(SPEC_MAX_THREADS), 0, st, S, A, M1);
    hipLaunchKernelGGL(s2m_solve_kernel, dim3((K + S2M_BN - 1) / S2M_BN), dim3(SPEC_MAX_THREADS), (size_t)M1 * S2M_BN * sizeof(double),
                       st, nodes, A, table, M1, M1p, K, Kp);
    return check_launch("spec2mcep_table");
}

extern "C" int ptts_spec2mcep(const float* x, float* out, int T, int M1, double alpha, int dftlen, int is_log, const double* table,
                              size_t table_bytes, void* stream) {
    PTTS_REQUIRE(T >= 0, "spec2mcep: T=%d", T);
    const int rc = s2m_args("spec2mcep", M1, alpha, dftlen);
    if (rc != PTTS_OK) return rc;
    if (T == 0) return PTTS_OK;
    PTTS_REQUIRE(x && out && table, "spec2mcep: null tensor");
    PTTS_REQUIRE(((size_t)table & 31) == 0 && table_bytes >= ptts_spec2mcep_table_bytes(M1, dftlen),
                 "spec2mcep: the table of ptts_spec2mcep_table(M1=%d, dftlen=%d) needs %zu aligned bytes, got %zu", M1, dftlen,
                 ptts_spec2mcep_table_bytes(M1, dftlen), table_bytes);
    int MW = 2;
    while (MW < M1 && MW < SPEC_MAX_THREADS) MW *= 2;
    hipLaunchKernelGGL(spec2mcep_kernel, dim3((T + SPEC_TT - 1) / SPEC_TT, (M1 + MW - 1) / MW), dim3(SPEC_MAX_THREADS), 0,
                       (hipStream_t)stream, x, table, out, T, M1, s2m_padded_order(M1), dftlen / 2 + 1, MW, is_log != 0);
    return check_launch("spec2mcep");
}
