// Periodic-plus-aperiodic waveform synthesis for the WORLD parameters (ln f0 | spec | aperiodicity [dB] | vuv; the step behind the
// reference's vocoders.py:300-330, which calls pyworld: the definition is this build's own, modelled on the published WORLD
// synthesis).  Notation: L = dftlen, M = L/2, K = M + 1 bins, P pulses, one table row
// {start, winlen, lb, rb, fr, i0, i1, v | delay, f0, w} per pulse.
//
// aperiodicity rows [T,A] dB -> [T,K]: 10^(x/20) per band, those values interpolated at k fs / L (band / fraction rows of
//                  ptts_fwbnd_table), clipped to [0, 1]; the row of an unvoiced frame (vuv < 0.5) is 1 throughout.
// segment of pulse n, rows i0 and i1 of the envelope and of the aperiodicity blended with the weight w:
//                  s_k = (1 - w) SPEC[i0,k] + w SPEC[i1,k], a_k likewise
//                  E_a = minphase(ln max(s_k a_k, 1e-10))
//                  E_p = minphase(ln max(s_k sqrt(1 - a_k^2) hp_k, 1e-10)) for a voiced pulse (v = 1), hp the high-pass at f0_n / 2;
//                        0 for an unvoiced one, whose chain is not run
//                  N, D as in pulsesynth.hip;  seg = irfft(E_p D + E_a N)[0 .. winlen)
// overlap-add      ptts_pulse_overlap_add of pulsesynth.hip: the first two table rows are its start and winlen.
//
// One workgroup per pulse on the in-LDS transforms of realfft.h, with the two buffers and the quarter circle of
// pulse_segments_kernel (2.25 M complex fp64 = 72 KiB at L = 4096): buffer A runs the E_a chain, buffer B takes the noise, becomes
// N and then E_a N, buffer A runs the E_p chain, B += E_p D while it is packed, B is transformed back: six transforms for a voiced
// pulse, four for an unvoiced one.  fp64 arithmetic, the segment is rounded to fp32 once; the noise energy is summed in the fixed
// order of block_sum (frame.h); no atomics, a result does not depend on the grid.
#include "common.h"
#include "synthchain.h"

namespace ptts {

// the table: {start, winlen, lb, rb, fr, i0, i1, v} int32 [8][P]; {delay, f0, w} fp64 [3][P]
constexpr int AR_MAX_NB = 1024;

// One workgroup per pulse.  dynamic LDS: (2 M + M/4) double2.
__global__ __launch_bounds__(PS_THREADS) void world_segments_kernel(const float* __restrict__ spec, const float* __restrict__ aper,
                                                                    const float* __restrict__ noise, const int* __restrict__ itab,
                                                                    const double* __restrict__ dtab, const int P, const int T,
                                                                    const int logM, const double fs, const int taper,
                                                                    const long long wavlen, float* __restrict__ seg, const int W) {
    extern __shared__ double2 lds[];
    __shared__ double red[PS_THREADS / 64];
    const int M = 1 << logM, L = M << 1, K = M + 1;
    double2* bufa = lds;            // the minimum-phase chains: E_a, then E_p
    double2* bufb = lds + M;        // the noise, E_a N, the sum
    double2* wq = lds + 2 * M;
    const int n = blockIdx.x, tid = threadIdx.x, nthr = blockDim.x;
    const int start = itab[n], winlen = itab[P + n], lb = itab[2 * P + n], rb = itab[3 * P + n], fr = itab[4 * P + n];
    const int i0 = itab[5 * P + n], i1 = itab[6 * P + n], voiced = itab[7 * P + n];
    const double delay = dtab[n], f0 = dtab[P + n], w = dtab[2 * P + n];
    // a row the host checks would have refused: nothing of it is read or written
    if (winlen < 1 || winlen > W || winlen > L || fr < 0 || fr >= T || i0 < 0 || i0 >= T || i1 < 0 || i1 >= T || lb < 0 ||
        rb > wavlen || rb < lb || (rb > lb && (lb < start || (long long)rb - start > L)) || !(f0 > 0.0) || !(w >= 0.0 && w <= 1.0))
        return;
    const float* s0row = spec + (size_t)i0 * K;
    const float* s1row = spec + (size_t)i1 * K;
    const float* a0row = aper + (size_t)i0 * K;
    const float* a1row = aper + (size_t)i1 * K;
    const double w0 = 1.0 - w;

    fill_twiddles(wq, M);
    noise_fill(bufb, noise, start, lb, rb, taper, M);

    // A: E_a
    minimum_phase(bufa, wq, logM, [&](int k) {
        const double s = w0 * (double)s0row[k] + w * (double)s1row[k], a = w0 * (double)a0row[k] + w * (double)a1row[k];
        const double v = s * a;
        return log(v > 1e-10 ? v : 1e-10);
    });
    // B: N, then E_a N (slot 0 holds bins 0 and M, both real in both factors)
    const double gain = noise_spectrum(bufb, wq, logM, red);
    for (int k = tid; k < M; k += nthr) {
        const int r = bitrev(k, logM);
        const double2 e = bufa[r], z = bufb[r];
        bufb[r] = k == 0 ? make_double2(e.x * (gain * z.x), e.y * (gain * z.y)) : cmul(e, make_double2(gain * z.x, gain * z.y));
    }
    __syncthreads();
    // A: E_p
    if (voiced) {
        double sn, cs;
        sincospi(0.5 * f0 / fs, &sn, &cs);
        const double tc = sn / cs;
        minimum_phase(bufa, wq, logM, [&](int k) {
            const double s = w0 * (double)s0row[k] + w * (double)s1row[k], a = w0 * (double)a0row[k] + w * (double)a1row[k];
            const double p = 1.0 - a * a;
            const double v = s * sqrt(p > 0.0 ? p : 0.0) * hp_gain(k, L, tc);
            return log(v > 1e-10 ? v : 1e-10);
        });
        __syncthreads();
    }

    // S = E_p D + E_a N, packed for the inverse transform in the same pass
    for (int k = tid; k <= (M >> 1); k += nthr) {
        const int km = M - k, rk = bitrev(k, logM), rm = k == 0 ? 0 : bitrev(km, logM);
        if (k == 0) {
            const double2 b = bufb[0];
            double x0 = b.x, xm = b.y;
            if (voiced) {
                const double2 ev = bufa[0];
                x0 += ev.x;
                xm += ev.y * cospi(delay);                          // the real part: what irfft reads of bin M
            }
            bufb[0] = make_double2(0.5 * (x0 + xm), 0.5 * (x0 - xm));
        } else {
            double2 xk = bufb[rk], xm = bufb[rm];
            if (voiced) {
                double sk, ck, sm, cm;
                sincospi(2.0 * delay * (double)k / (double)L, &sk, &ck);
                sincospi(2.0 * delay * (double)km / (double)L, &sm, &cm);
                xk = cadd(xk, cmul(bufa[rk], make_double2(ck, -sk)));
                xm = cadd(xm, cmul(bufa[rm], make_double2(cm, -sm)));
            }
            double2 zk, zm;
            pack_pair(xk, xm, pair_twiddle(k, L), zk, zm);
            bufb[rk] = zk;
            if (k != (M >> 1)) bufb[rm] = zm;
        }
    }
    fft_inverse(bufb, wq, logM);
    write_segment(bufb, M, seg, n, W, winlen);
}

// One workgroup per frame.  dynamic LDS: nb doubles (the frame's bands as amplitudes).
__global__ __launch_bounds__(256) void aper_rows_kernel(const float* __restrict__ aper, const float* __restrict__ vuv,
                                                        const double* __restrict__ tab, float* __restrict__ out, const int nb,
                                                        const int K, const int Kp) {
    extern __shared__ double ar_lds[];
    const int t = blockIdx.x, tid = threadIdx.x, nthr = blockDim.x;
    const bool voiced = (double)vuv[t] >= 0.5;
    if (!voiced) {
        for (int k = tid; k < K; k += nthr) out[(size_t)t * K + k] = 1.f;
        return;
    }
    for (int i = tid; i < nb; i += nthr) ar_lds[i] = pow(10.0, (double)aper[(size_t)t * nb + i] / 20.0);
    __syncthreads();
    for (int k = tid; k < K; k += nthr) {
        int b;
        double fr;
        band_of(tab, Kp, nb, k, b, fr);
        const double lo = ar_lds[b], hi = ar_lds[b + 1];
        const double v = fma(fr, hi - lo, lo);
        out[(size_t)t * K + k] = (float)(v < 0.0 ? 0.0 : (v > 1.0 ? 1.0 : v));
    }
}

}  // namespace ptts

using namespace ptts;

extern "C" int ptts_aper_rows(const float* aper, const float* vuv, float* out, int T, int nb, double fs, int dftlen,
                              const double* table, size_t table_bytes, void* stream) {
    PTTS_REQUIRE(T >= 0, "aper_rows: T=%d", T);
    PTTS_REQUIRE(nb >= 2 && nb <= AR_MAX_NB, "aper_rows: nb=%d outside [2, %d]", nb, AR_MAX_NB);
    PTTS_REQUIRE(fs > 0.0 && fs < 1e9, "aper_rows: fs=%g", fs);
    PTTS_REQUIRE(frame_log2(dftlen) > 0, "aper_rows: dftlen=%d is not a power of two in [%d, %d]", dftlen, FRAME_MIN_DFTLEN,
                 FRAME_MAX_DFTLEN);
    if (T == 0) return PTTS_OK;
    PTTS_REQUIRE(aper && vuv && out && table, "aper_rows: null tensor");
    const int K = dftlen / 2 + 1, Kp = (K + 3) / 4 * 4;
    PTTS_REQUIRE(((size_t)table & 31) == 0 && table_bytes >= ptts_fwbnd_table_bytes(dftlen),
                 "aper_rows: the table of ptts_fwbnd_table(dftlen=%d) needs %zu aligned bytes, got %zu", dftlen,
                 ptts_fwbnd_table_bytes(dftlen), table_bytes);
    hipLaunchKernelGGL(aper_rows_kernel, dim3(T), dim3(256), (size_t)nb * sizeof(double), (hipStream_t)stream, aper, vuv, table, out,
                       nb, K, Kp);
    return check_launch("aper_rows");
}

extern "C" int ptts_world_segments(const float* spec, const float* aper, const float* noise, const int* itab, const double* dtab,
                                   int P, int T, int dftlen, double fs, long long wavlen, float* seg, int W, void* stream) {
    return launch_segments<world_segments_kernel>("world_segments", spec, aper, noise, itab, dtab, P, T, dftlen, fs, wavlen, seg, W, stream);
}
