// What the two waveform synthesisers share (pulsesynth.hip for the PML parameters, worldsynth.hip for the WORLD parameters),
// on the in-LDS transforms of realfft.h and the scaffold of frame.h: the minimum-phase chain, the pulse's stretch of the noise and
// its normalisation, the high-pass gain, the segment's write-out and the launch of a segments kernel.  Notation as there:
// L = dftlen, M = L/2 complex points, K = M + 1 bins, a spectrum at bit-reversed addresses with X_0 and X_M in slot 0.  fp64
// throughout; every device routine but hp_gain is called by the whole workgroup.
#pragma once
#include "common.h"
#include "frame.h"

namespace ptts {

constexpr int PS_THREADS = 256;

// hp_k = (1 + (tc / tan(pi k / L))^8)^(-1/2), hp_0 = 0; tc = tan(pi fcut / fs)
__device__ __forceinline__ double hp_gain(int k, int L, double tc) {
    double hp = 0.0;
    if (k > 0) {
        double s, c;
        sincospi((double)k / (double)L, &s, &c);
        const double r = tc * c / s, r2 = r * r, r4 = r2 * r2;
        hp = 1.0 / sqrt(1.0 + r4 * r4);
    }
    return hp;
}

// The noise segment, packed: position p of the frame holds g[start + p] for lb <= start + p < rb, tapered over `taper` samples at
// both ends where the segment is long enough for it.
__device__ __forceinline__ void noise_fill(double2* bufn, const float* __restrict__ noise, int start, int lb, int rb, int taper, int M) {
    const long long p0 = (long long)lb - start, p1 = (long long)rb - start;
    const int len = rb - lb;
    const bool tapered = taper > 0 && len >= 2 * (taper + 1);
    for (int i = threadIdx.x; i < M; i += blockDim.x) {
        double v[2];
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const long long p = 2 * (long long)i + h;
            v[h] = 0.0;
            if (p >= p0 && p < p1) {
                const int q = (int)(p - p0);
                double g = (double)noise[(long long)lb + q];
                if (tapered) {
                    if (q <= taper) g *= 0.5 - 0.5 * cospi((double)q / (double)taper);
                    if (len - 1 - q <= taper) g *= 0.5 - 0.5 * cospi((double)(len - 1 - q) / (double)taper);
                }
                v[h] = g;
            }
        }
        bufn[i] = make_double2(v[0], v[1]);
    }
}

// bufn (the packed noise segment) -> its bins N_k; returns the factor that scales them to the mean spectral energy of a Dirac
// (0 for an empty or all-zero segment).  The energy is summed in a fixed order.
__device__ __forceinline__ double noise_spectrum(double2* bufn, const double2* wq, int logM, double* red) {
    const int M = 1 << logM, L = M << 1;
    fft_forward(bufn, wq, logM);
    unpack_real(bufn, logM);
    double e = 0.0;
    for (int k = threadIdx.x; k < M; k += blockDim.x) {
        const double2 z = bufn[bitrev(k, logM)];
        e += k == 0 ? z.x * z.x + z.y * z.y : 2.0 * (z.x * z.x + z.y * z.y);
    }
    e = block_sum(e, red) / (double)L;
    return e > 0.0 ? 1.0 / sqrt(e) : 0.0;
}

// Minimum phase: la(k), 0 <= k <= M, the real log-amplitudes -> bufe = E, |E_k| = exp(la_k):
// c = irfft(la); c[1..M-1] *= 2, c[M+1..] = 0; E = exp(rfft(c)).  The last pass is not followed by a barrier.
template <class LogAmplitude>
__device__ __forceinline__ void minimum_phase(double2* bufe, const double2* wq, int logM, LogAmplitude la) {
    const int M = 1 << logM, L = M << 1, tid = threadIdx.x, nthr = blockDim.x;
    // la is real: the packed spectrum of c = irfft(la)
    for (int k = tid; k <= (M >> 1); k += nthr) {
        const double lk = la(k), lm = la(M - k);
        double2 zk, zm;
        pack_pair(make_double2(lk, 0.0), make_double2(lm, 0.0), pair_twiddle(k, L), zk, zm);
        if (k == 0) {
            bufe[0] = make_double2(0.5 * (lk + lm), 0.5 * (lk - lm));
        } else {
            bufe[bitrev(k, logM)] = zk;
            if (k != (M >> 1)) bufe[bitrev(M - k, logM)] = zm;
        }
    }
    fft_inverse(bufe, wq, logM);
    // c[2i] + i c[2i+1] = bufe[i] / M; fold the cepstrum onto its causal half
    const double inv_m = 1.0 / (double)M;
    for (int i = tid; i < M; i += nthr) {
        const double2 z = bufe[i];
        double2 o = make_double2(0.0, 0.0);
        if (i == 0) o = make_double2(z.x * inv_m, 2.0 * z.y * inv_m);
        else if (i < (M >> 1)) o = make_double2(2.0 * z.x * inv_m, 2.0 * z.y * inv_m);
        else if (i == (M >> 1)) o = make_double2(z.x * inv_m, 0.0);
        bufe[i] = o;
    }
    fft_forward(bufe, wq, logM);
    unpack_real(bufe, logM);
    for (int k = tid; k < M; k += nthr) {
        const int r = bitrev(k, logM);
        const double2 c = bufe[r];
        if (k == 0) {
            bufe[0] = make_double2(exp(c.x), exp(c.y));       // E_0 and E_M, both real
        } else {
            double s, cs;
            sincos(c.y, &s, &cs);
            const double m = exp(c.x);
            bufe[r] = make_double2(m * cs, m * s);
        }
    }
}

// seg[n, 0 .. winlen) out of buf, M times the packed segment as fft_inverse leaves it
__device__ __forceinline__ void write_segment(const double2* buf, int M, float* seg, int n, int W, int winlen) {
    const int tid = threadIdx.x, nthr = blockDim.x;
    const double inv_m = 1.0 / (double)M;
    float* out = seg + (size_t)n * W;
    for (int p = tid; p < winlen; p += nthr) {
        const double2 z = buf[p >> 1];
        out[p] = (float)(((p & 1) ? z.y : z.x) * inv_m);
    }
}

// The entry point of a segments kernel: one workgroup per pulse with (2 M + M/4) double2 of dynamic LDS.  rows: the [T,K] rows
// beside the envelope, the noise mask or the aperiodicity.
template <auto Kernel>
int launch_segments(const char* name, const float* spec, const float* rows, const float* noise, const int* itab, const double* dtab,
                    int P, int T, int dftlen, double fs, long long wavlen, float* seg, int W, void* stream) {
    PTTS_REQUIRE(P >= 0 && T >= 0 && wavlen >= 0, "%s: P=%d T=%d wavlen=%lld", name, P, T, wavlen);
    const int logL = frame_log2(dftlen);
    PTTS_REQUIRE(logL > 0, "%s: dftlen=%d is not a power of two in [%d, %d]", name, dftlen, FRAME_MIN_DFTLEN, FRAME_MAX_DFTLEN);
    PTTS_REQUIRE(fs > 0.0 && fs < 1e9, "%s: fs=%g", name, fs);
    PTTS_REQUIRE(W >= 1 && W <= dftlen, "%s: W=%d outside [1, dftlen]", name, W);
    if (P == 0 || T == 0) return PTTS_OK;
    PTTS_REQUIRE(spec && rows && itab && dtab && seg && (noise || wavlen == 0), "%s: null tensor", name);
    const int M = dftlen / 2;
    const int lds = (2 * M + M / 4) * (int)sizeof(double2);
    const int rc = reserve_lds<Kernel>(name, lds);
    if (rc != PTTS_OK) return rc;
    const int taper = (int)floor(0.001 * fs + 0.5);
    hipLaunchKernelGGL(Kernel, dim3(P), dim3(frame_threads(M, PS_THREADS)), (size_t)lds, (hipStream_t)stream, spec, rows, noise, itab,
                       dtab, P, T, logL - 1, fs, taper, wavlen, seg, W);
    return check_launch(name);
}

}  // namespace ptts
