// Pulse-and-noise waveform synthesis of the PML vocoder (the step behind the reference's vocoders.py:194-206, whose
// pulsemodel submodule is absent from the reference checkout: the definition is this build's own).
// Notation: L = dftlen, M = L/2, K = M + 1 bins, P pulses, one table row {start, winlen, lb, rb, fr | delay, f0} per pulse.
//
// noise mask       [T,nb] -> [T,K]: band values interpolated at k fs / L (band / fraction rows of ptts_fwbnd_table), bins below
//                  int(2 f0 L / fs) zeroed, thresholded at 0.5, smoothed along k by the 17 taps h = w * w, w = hanning(9) / 4,
//                  over the odd extension of the row (what a forward-backward pass of w does), clipped to [0, 1].
// segment of pulse n, row fr of the envelope and of the mask:
//                  la_k = ln(max(SPEC_k hp_k, 1e-10)),  hp_k = (1 + (tan(pi fcut / fs) / tan(pi k / L))^8)^(-1/2), fcut = f0_n / 2
//                  c = irfft(la); c[1..M-1] *= 2, c[M+1..] = 0;  E = exp(rfft(c))              (minimum phase)
//                  x = the normals g[lb..rb) at lb - start, tapered over 1 ms at both ends; N = rfft(x), scaled to the mean
//                  spectral energy of a Dirac;  D_k = exp(-2 pi i delay k / L)
//                  seg = irfft(E ((1 - m) D + m N))[0 .. winlen)
// overlap-add      wav[j] = sum_n seg_n[j - start_n], in pulse order.
//
// The real transform of length L is the in-LDS radix-2 transform of realfft.h on the packed sequence (M = L/2 complex points, a
// spectrum at bit-reversed addresses, X_0 and X_M in slot 0).  One workgroup per pulse holds two such
// buffers (E and the noise / the product) and a quarter circle of twiddles: 2.25 M complex fp64 = 72 KiB at L = 4096, 144 KiB at 8192.
// Arithmetic is fp64 throughout, the segment is rounded to fp32 once.  The noise energy is summed inside the workgroup in a fixed
// order (wave butterflies, then wave order through LDS); the overlap-add gathers, so nothing here uses an atomic and a result does
// not depend on the grid.
#include "common.h"
#include "synthchain.h"

namespace ptts {

constexpr int PS_ITAB_ROWS = 5, PS_DTAB_ROWS = 2;      // {start, winlen, lb, rb, fr} int32 [5][P]; {delay, f0} fp64 [2][P]
constexpr int NM_TAPS = 17, NM_HALF = 8;
constexpr int NM_MAX_NB = 1024;

struct NmTaps { double h[NM_TAPS]; };

// ln(max(SPEC_k hp_k, 1e-10)); tc = tan(pi fcut / fs)
__device__ __forceinline__ double log_amplitude(const float* __restrict__ row, int k, int L, double tc) {
    const double v = (double)row[k] * hp_gain(k, L, tc);
    return log(v > 1e-10 ? v : 1e-10);
}

// One workgroup per pulse.  dynamic LDS: (2 M + M/4) double2.
__global__ __launch_bounds__(PS_THREADS) void pulse_segments_kernel(const float* __restrict__ spec, const float* __restrict__ mask,
                                                                    const float* __restrict__ noise, const int* __restrict__ itab,
                                                                    const double* __restrict__ dtab, const int P, const int T,
                                                                    const int logM, const double fs, const int taper,
                                                                    const long long wavlen, float* __restrict__ seg, const int W) {
    extern __shared__ double2 lds[];
    __shared__ double red[PS_THREADS / 64];
    const int M = 1 << logM, L = M << 1, K = M + 1;
    double2* bufe = lds;            // the minimum-phase chain, E at the end
    double2* bufn = lds + M;        // the noise, then the product
    double2* wq = lds + 2 * M;
    const int n = blockIdx.x, tid = threadIdx.x, nthr = blockDim.x;
    const int start = itab[n], winlen = itab[P + n], lb = itab[2 * P + n], rb = itab[3 * P + n], fr = itab[4 * P + n];
    const double delay = dtab[n], f0 = dtab[P + n];
    // a row the host checks would have refused: nothing of it is read or written
    if (winlen < 1 || winlen > W || winlen > L || fr < 0 || fr >= T || lb < 0 || rb > wavlen || rb < lb || !(f0 > 0.0)) return;
    const float* srow = spec + (size_t)fr * K;
    const float* mrow = mask + (size_t)fr * K;

    fill_twiddles(wq, M);
    noise_fill(bufn, noise, start, lb, rb, taper, M);

    double s0, c0;
    sincospi(0.5 * f0 / fs, &s0, &c0);
    const double tc = s0 / c0;
    minimum_phase(bufe, wq, logM, [&](int k) { return log_amplitude(srow, k, L, tc); });
    const double gain = noise_spectrum(bufn, wq, logM, red);

    // S = E ((1 - m) D + m N), packed for the inverse transform in the same pass
    for (int k = tid; k <= (M >> 1); k += nthr) {
        const int km = M - k, rk = bitrev(k, logM), rm = k == 0 ? 0 : bitrev(km, logM);
        const double mk = (double)mrow[k], mm = (double)mrow[km];
        double sk, ck, sm, cm;
        sincospi(2.0 * delay * (double)k / (double)L, &sk, &ck);
        sincospi(2.0 * delay * (double)km / (double)L, &sm, &cm);
        if (k == 0) {
            const double2 ev = bufe[0], nv = bufn[0];
            const double x0 = ev.x * ((1.0 - mk) + mk * gain * nv.x);
            const double xm = ev.y * ((1.0 - mm) * cm + mm * gain * nv.y);      // the real part: what irfft reads of bin M
            bufn[0] = make_double2(0.5 * (x0 + xm), 0.5 * (x0 - xm));
        } else {
            const double2 nk = bufn[rk], nm = bufn[rm];
            const double2 xk = cmul(bufe[rk], make_double2((1.0 - mk) * ck + mk * gain * nk.x, -(1.0 - mk) * sk + mk * gain * nk.y));
            const double2 xm = cmul(bufe[rm], make_double2((1.0 - mm) * cm + mm * gain * nm.x, -(1.0 - mm) * sm + mm * gain * nm.y));
            double2 zk, zm;
            pack_pair(xk, xm, pair_twiddle(k, L), zk, zm);
            bufn[rk] = zk;
            if (k != (M >> 1)) bufn[rm] = zm;
        }
    }
    fft_inverse(bufn, wq, logM);
    write_segment(bufn, M, seg, n, W, winlen);
}

// One lane per sample: the pulses whose window covers it lie between two binary searches over the ascending starts.
__global__ __launch_bounds__(256) void pulse_overlap_add_kernel(const float* __restrict__ seg, const int* __restrict__ itab, const int P,
                                                                const int W, float* __restrict__ wav, const long long wavlen) {
    const long long j = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= wavlen) return;
    const int* start = itab;
    const int* winlen = itab + P;
    int lo = 0, hi = P;                                 // first pulse with start > j - W
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if ((long long)start[mid] > j - W) hi = mid; else lo = mid + 1;
    }
    const int first = lo;
    hi = P;                                             // first pulse with start > j
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if ((long long)start[mid] > j) hi = mid; else lo = mid + 1;
    }
    double acc = 0.0;
    for (int n = first; n < lo; ++n) {
        const long long off = j - start[n];
        const int wl = winlen[n];
        if (off >= 0 && off < wl && wl <= W) acc += (double)seg[(size_t)n * W + off];
    }
    wav[j] = (float)acc;
}

// One workgroup per frame.  dynamic LDS: (K + 2 NM_HALF) floats (the thresholded row and its extension) + nb floats.
__global__ __launch_bounds__(256) void noise_mask_kernel(const float* __restrict__ nmb, const float* __restrict__ f0,
                                                         const double* __restrict__ tab, float* __restrict__ out, const int nb,
                                                         const int K, const int Kp, const int L, const double fs, const NmTaps taps) {
    extern __shared__ float nm_lds[];
    float* x = nm_lds + NM_HALF;                        // x[-8 .. K + 8)
    float* sb = nm_lds + K + 2 * NM_HALF;               // the frame's bands
    const int t = blockIdx.x, tid = threadIdx.x, nthr = blockDim.x;
    for (int i = tid; i < nb; i += nthr) sb[i] = nmb[(size_t)t * nb + i];
    __syncthreads();
    const int kcut = (int)(2.0 * (double)f0[t] * (double)L / fs);
    for (int k = tid; k < K; k += nthr) {
        int b;
        double fr;
        band_of(tab, Kp, nb, k, b, fr);
        const double lo = (double)sb[b], hi = (double)sb[b + 1];
        const double v = fma(fr, hi - lo, lo);
        x[k] = (k >= kcut && v > 0.5) ? 1.f : 0.f;
    }
    __syncthreads();
    if (tid < NM_HALF) {
        const int j = tid + 1;
        x[-j] = 2.f * x[0] - x[j];
        x[K - 1 + j] = 2.f * x[K - 1] - x[K - 1 - j];
    }
    __syncthreads();
    for (int k = tid; k < K; k += nthr) {
        double acc = 0.0;
#pragma unroll
        for (int i = 0; i < NM_TAPS; ++i) acc += taps.h[i] * (double)x[k + i - NM_HALF];
        out[(size_t)t * K + k] = (float)(acc < 0.0 ? 0.0 : (acc > 1.0 ? 1.0 : acc));
    }
}

}  // namespace ptts

using namespace ptts;

extern "C" int ptts_noise_mask(const float* nmb, const float* f0, float* out, int T, int nb, double fs, int dftlen,
                               const double* table, size_t table_bytes, void* stream) {
    PTTS_REQUIRE(T >= 0, "noise_mask: T=%d", T);
    PTTS_REQUIRE(nb >= 2 && nb <= NM_MAX_NB, "noise_mask: nb=%d outside [2, %d]", nb, NM_MAX_NB);
    PTTS_REQUIRE(fs > 0.0 && fs < 1e9, "noise_mask: fs=%g", fs);
    PTTS_REQUIRE(frame_log2(dftlen) > 0, "noise_mask: dftlen=%d is not a power of two in [%d, %d]", dftlen, FRAME_MIN_DFTLEN,
                 FRAME_MAX_DFTLEN);
    if (T == 0) return PTTS_OK;
    PTTS_REQUIRE(nmb && f0 && out && table, "noise_mask: null tensor");
    const int K = dftlen / 2 + 1, Kp = (K + 3) / 4 * 4;
    PTTS_REQUIRE(((size_t)table & 31) == 0 && table_bytes >= ptts_fwbnd_table_bytes(dftlen),
                 "noise_mask: the table of ptts_fwbnd_table(dftlen=%d) needs %zu aligned bytes, got %zu", dftlen,
                 ptts_fwbnd_table_bytes(dftlen), table_bytes);
    // h = w * w, w = hanning(9) / 4
    NmTaps taps;
    double w[9];
    for (int i = 0; i < 9; ++i) w[i] = (0.5 - 0.5 * cos(2.0 * 3.14159265358979323846 * i / 8.0)) / 4.0;
    for (int i = 0; i < NM_TAPS; ++i) {
        double s = 0.0;
        for (int j = 0; j < 9; ++j)
            if (i - j >= 0 && i - j < 9) s += w[j] * w[i - j];
        taps.h[i] = s;
    }
    const size_t lds = (size_t)(K + 2 * NM_HALF + nb) * sizeof(float);
    hipLaunchKernelGGL(noise_mask_kernel, dim3(T), dim3(256), lds, (hipStream_t)stream, nmb, f0, table, out, nb, K, Kp, dftlen, fs,
                       taps);
    return check_launch("noise_mask");
}

extern "C" int ptts_pulse_segments(const float* spec, const float* mask, const float* noise, const int* itab, const double* dtab,
                                   int P, int T, int dftlen, double fs, long long wavlen, float* seg, int W, void* stream) {
    return launch_segments<pulse_segments_kernel>("pulse_segments", spec, mask, noise, itab, dtab, P, T, dftlen, fs, wavlen, seg, W, stream);
}

extern "C" int ptts_pulse_overlap_add(const float* seg, const int* itab, int P, int W, float* wav, long long wavlen, void* stream) {
    PTTS_REQUIRE(P >= 0 && W >= 1 && wavlen >= 0, "pulse_overlap_add: P=%d W=%d wavlen=%lld", P, W, wavlen);
    if (wavlen == 0) return PTTS_OK;
    PTTS_REQUIRE(wav && (P == 0 || (seg && itab)), "pulse_overlap_add: null tensor");
    PTTS_REQUIRE((wavlen + 255) / 256 < (1LL << 31), "pulse_overlap_add: wavlen=%lld", wavlen);
    hipLaunchKernelGGL(pulse_overlap_add_kernel, dim3((unsigned)((wavlen + 255) / 256)), dim3(256), 0, (hipStream_t)stream, seg, itab,
                       P, W, wav, wavlen);
    return check_launch("pulse_overlap_add");
}
