// Waveform analysis for the WORLD parameters: the counterpart of worldsynth.hip (the step behind the reference's
// vocoders.py:234-284, which calls pyworld: the definition is this build's own; the envelope is modelled on
// CheapTrick, Morise 2015, the aperiodicity is the build's own estimator in the place of D4C).
// Notation: L = dftlen, M = L/2, K = M + 1 bins, rnd(x) = floor(x + 0.5); frame i sits at t_i = i shift, c = rnd(t_i fs).
//
// window           hw = int(1.5 fs / r), w_j = (0.5 + 0.5 cos(pi j / (hw + 1))) / sqrt(0.75 (hw + 1)), j = -hw .. hw (sum w^2 = 1),
//                  frame at centre c: x[j mod L] = wav[c + j] w_j (zero-phase placement, samples outside [0, N) are 0)
// envelope         r = rate_i (f0_i for a voiced frame, 500 Hz for an unvoiced one), X = rfft(frame at c), P_k = |X_k|^2
//   DC correction  kappa = r L / fs;  k < kappa: P_k += P(kappa - k), P(y) = P_j + (y - j) (P_{j+1} - P_j), j = int(y), uncorrected
//   smoothing      d = r L / (3 fs);  S_k = (1 / 2d) * integral over [k - d, k + d] of the piecewise constant P (bin j on
//                  [j - 1/2, j + 1/2), mirrored at 0 and at M): a direct sum, bins ascending, fractional weights at both ends
//   gain           la_k = ln max(sqrt(S_k fs / r), 1e-10)
//   lifter         c = irfft(la);  c_q *= sinc(r q / fs) (1 - 2 q1 + 2 q1 cos(2 pi r q / fs)), q1 = -0.15, q = min(q, L - q);
//                  ln SPEC[i,k] = Re rfft(c)_k
// aperiodicity     voiced frame: T0 = fs / f0_i, n0 = rnd(T0), delta = T0 - n0, c1 = c - (n0 >> 1), c2 = c1 + n0, r = f0_i;
//                  X1 = rfft(frame at c1), X2_k = rfft(frame at c2)_k exp(+2 pi i k delta / L)
//                  D_k = |X1_k - X2_k|^2 / 2, E_k = (|X1_k|^2 + |X2_k|^2) / 2
//                  rho_b = sum_k W[k,b] D_k / sum_k W[k,b] E_k over the bins k >= f0_i L / fs, ascending (W: the hat weights of
//                  analysis.hip, from the band / fraction rows of ptts_fwbnd_table)
//                  aper[i,b] = 10 log10(clip(rho_b, 1e-6, 1)); a band whose denominator is not positive takes rho of the nearest
//                  band above it that has one, 0 dB if there is none
//                  unvoiced frame (voiced_i < 0.5): 0 dB throughout, no transform is run
//
// Integer decisions (c, hw, n0, every bin index) are taken in fp64 from the fp32 inputs with the operation order written here (the
// build has no fused contraction), so that a host restatement takes the same ones.  Arithmetic is fp64, results are rounded to fp32
// once.  One workgroup per frame on the in-LDS transforms of realfft.h.
//   envelope:      ONE packed buffer, the quarter circle and K doubles of P: 28 M + 8 bytes = 57 352 B (56 KiB) at L = 4096, two
//                  workgroups per CU of 160 KiB; 114 696 B at L = 8192, one.  Three transforms per frame.
//   aperiodicity:  TWO packed buffers, the quarter circle, two slots for bin M and nb doubles: 36 M + 32 + 8 nb bytes = 73 760 B
//                  (72 KiB) + 8 nb at L = 4096, two workgroups per CU; 147 488 B + 8 nb <= 155 680 B at L = 8192, one.  Two
//                  transforms per voiced frame, run side by side; the second buffer then takes the band axis (lower band and
//                  fraction of every bin), so that the band sums, one lane per band, walk LDS and not the table in memory.
// Both fit at L = 8192, so dftlen is not capped below the 8192 of the other transform kernels.  Every sum runs in a fixed order
// inside one lane (bins ascending; a band's sum is cut into G stretches of its bins, G a function of nb and L, each summed by one
// lane, and one lane adds the G partial sums in order); nothing here uses an atomic and a result does not depend on the grid.
#include "common.h"
#include "frame.h"

namespace ptts {

constexpr int WA_THREADS = 256;
constexpr int WA_MAX_NB = 1024;
constexpr double WA_Q1 = -0.15;                         // the lifter's q1
constexpr double WA_PI = 3.14159265358979323846;

__device__ __forceinline__ double wa_mag2(double2 z) { return z.x * z.x + z.y * z.y; }

// |X_k|^2 of the unpacked spectrum, 0 <= k <= M.  Not wa_mag2(spectrum_bin()): bins 0 and M are x * x, without a + 0 * 0 behind it.
__device__ __forceinline__ double wa_power_bin(const double2* a, int k, int logM) {
    const int M = 1 << logM;
    if (k <= 0) return a[0].x * a[0].x;
    if (k >= M) return a[0].y * a[0].y;
    return wa_mag2(a[bitrev(k, logM)]);
}

// The window of frame_fill for half width hw: w_j = (0.5 + 0.5 cos(pi j / (hw + 1))) / sqrt(0.75 (hw + 1))
__device__ __forceinline__ auto wa_hann(int hw) {
    const double wnorm = 1.0 / sqrt(0.75 * (double)(hw + 1));
    return [=](int j) { return (0.5 + 0.5 * cospi((double)j / (double)(hw + 1))) * wnorm; };
}

// the window of a frame at rate r: false for a frame the host checks would have refused
__device__ __forceinline__ bool wa_window(double r, double fs, int L, int& hw) {
    if (!(r > 0.0) || !(r < 0.5 * fs)) return false;
    const double hwd = 1.5 * fs / r;
    if (!(hwd < (double)L) || 2 * (int)hwd + 1 > L) return false;
    hw = (int)hwd;
    return true;
}

// S_k: the mean of the piecewise constant P over [k - d, k + d], mirrored at 0 and at M (d < M)
__device__ __forceinline__ double wa_smooth(const double* P, int k, double d, int M) {
    const double lo = (double)k - d, hi = (double)k + d;
    const int jlo = (int)floor(lo + 0.5), jhi = (int)floor(hi + 0.5);
    auto at = [&](int j) {
        j = j < 0 ? -j : j;
        j = j > M ? 2 * M - j : j;
        return P[j < 0 ? 0 : j];
    };
    double s;
    if (jlo == jhi) {
        s = at(jlo) * (hi - lo);
    } else {
        s = at(jlo) * (((double)jlo + 0.5) - lo);
        for (int j = jlo + 1; j < jhi; ++j) s += at(j);
        s += at(jhi) * (hi - ((double)jhi - 0.5));
    }
    return s / (2.0 * d);
}

// the lifter at the symmetric quefrency q
__device__ __forceinline__ double wa_lifter(int q, double r, double fs) {
    const double x = r * (double)q / fs;
    const double sinc = q == 0 ? 1.0 : sinpi(x) / (WA_PI * x);
    return sinc * ((1.0 - 2.0 * WA_Q1) + 2.0 * WA_Q1 * cospi(2.0 * x));
}

// Frame i of one utterance: wav [N] its samples, ratev and spec its own rows.  The workgroup's work; dynamic LDS:
// (M + M/4) double2 + K doubles.
__device__ __forceinline__ void world_envelope_frame(const float* __restrict__ wav, const long long N, const float* __restrict__ ratev,
                                                     float* __restrict__ spec, const int i, const int logM, const double shift,
                                                     const double fs, const bool log_out) {
    extern __shared__ double2 lds[];
    const int M = 1 << logM, L = M << 1, K = M + 1, Mq = M >> 2;
    double2* a = lds;
    double2* wq = lds + M;
    double* P = reinterpret_cast<double*>(lds + M + Mq);
    const int tid = threadIdx.x, nthr = blockDim.x;
    const double r = (double)ratev[i];
    int hw;
    // a frame the host checks would have refused: nothing of it is read or written
    if (!wa_window(r, fs, L, hw)) return;
    const long long c = (long long)rnd((double)i * shift * fs);

    fill_twiddles(wq, M);
    frame_fill(a, wav, N, c, hw, M, wa_hann(hw));
    fft_forward(a, wq, logM);
    unpack_real(a, logM);

    // P with the DC correction, read off the uncorrected bins of a (kappa < M: j + 1 <= M)
    const double kappa = r * (double)L / fs;
    for (int k = tid; k < K; k += nthr) {
        double p = wa_power_bin(a, k, logM);
        if ((double)k < kappa) {
            const double y = kappa - (double)k;
            int j = (int)y;
            j = j > M - 1 ? M - 1 : j;
            const double p0 = wa_power_bin(a, j, logM), p1 = wa_power_bin(a, j + 1, logM);
            p += p0 + (y - (double)j) * (p1 - p0);
        }
        P[k] = p;
    }
    __syncthreads();

    // la is real: the packed spectrum of c = irfft(la)
    const double d = r * (double)L / (3.0 * fs), gain = fs / r;
    for (int k = tid; k <= (M >> 1); k += nthr) {
        double la[2];
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            const double amp = sqrt(wa_smooth(P, q == 0 ? k : M - k, d, M) * gain);
            la[q] = log(amp > 1e-10 ? amp : 1e-10);
        }
        if (k == 0) {
            a[0] = make_double2(0.5 * (la[0] + la[1]), 0.5 * (la[0] - la[1]));
        } else {
            double2 zk, zm;
            pack_pair(make_double2(la[0], 0.0), make_double2(la[1], 0.0), pair_twiddle(k, L), zk, zm);
            a[bitrev(k, logM)] = zk;
            if (k != (M >> 1)) a[bitrev(M - k, logM)] = zm;
        }
    }
    fft_inverse(a, wq, logM);
    // c[2n] + i c[2n+1] = a[n] / M
    const double inv_m = 1.0 / (double)M;
    for (int n = tid; n < M; n += nthr) {
        const double2 z = a[n];
        const int q0 = 2 * n, q1 = 2 * n + 1;
        a[n] = make_double2(z.x * inv_m * wa_lifter(q0 <= M ? q0 : L - q0, r, fs), z.y * inv_m * wa_lifter(q1 <= M ? q1 : L - q1, r, fs));
    }
    fft_forward(a, wq, logM);
    unpack_real(a, logM);

    float* srow = spec + (size_t)i * K;
    for (int k = tid; k < K; k += nthr) {
        const double v = k == 0 ? a[0].x : (k == M ? a[0].y : a[bitrev(k, logM)].x);
        srow[k] = (float)(log_out ? v : exp(v));
    }
}

// One workgroup per frame.
__global__ __launch_bounds__(WA_THREADS) void world_envelope_kernel(const float* __restrict__ wav, const long long N,
                                                                    const float* __restrict__ ratev, float* __restrict__ spec,
                                                                    const int logM, const double shift, const double fs,
                                                                    const bool log_out) {
    world_envelope_frame(wav, N, ratev, spec, blockIdx.x, logM, shift, fs, log_out);
}

// One workgroup per frame of the packed batch.
__global__ __launch_bounds__(WA_THREADS) void world_envelope_batch_kernel(const float* __restrict__ wav, const long long* __restrict__ wav_off,
                                                                          const long long wav_total, const long long* __restrict__ frame_off,
                                                                          const int B, const int T, const float* __restrict__ ratev,
                                                                          float* __restrict__ spec, const int logM, const double shift,
                                                                          const double fs, const bool log_out) {
    const PackedFrame f = packed_frame(wav_off, wav_total, frame_off, B, T, blockIdx.x);
    if (!f.ok) return;
    world_envelope_frame(wav + f.woff, f.N, ratev + f.foff, spec + (size_t)f.foff * ((1 << logM) + 1), f.i, logM, shift, fs, log_out);
}

// Frame i of one utterance: wav [N] its samples, f0v, voicedv and aper its own rows.  The workgroup's work; dynamic LDS:
// (2 M + M/4 + 2) double2 + nb doubles.
__device__ __forceinline__ void world_aperiodicity_frame(const float* __restrict__ wav, const long long N, const float* __restrict__ f0v,
                                                         const float* __restrict__ voicedv, float* __restrict__ aper, const int i,
                                                         const int nb, const int Kp, const int logM, const double shift,
                                                         const double fs, const double* __restrict__ fw) {
    extern __shared__ double2 lds[];
    const int M = 1 << logM, L = M << 1, K = M + 1, Mq = M >> 2;
    double2* a1 = lds;                  // X1, then (D_k, E_k) at the bit-reversed address of k, bin 0 in slot 0
    double2* a2 = lds + M;              // X2, then (lower band, fraction) of bin k at k: the band axis, staged for the band sums
    double2* wq = lds + 2 * M;
    double2* xm = lds + 2 * M + Mq;     // bin M: (D_M, E_M), (lower band, fraction)
    double* rho = reinterpret_cast<double*>(lds + 2 * M + Mq + 2);
    const int tid = threadIdx.x, nthr = blockDim.x;
    float* row = aper + (size_t)i * nb;
    if (!((double)voicedv[i] >= 0.5)) {
        for (int b = tid; b < nb; b += nthr) row[b] = 0.f;
        return;
    }
    const double f0 = (double)f0v[i];
    int hw;
    // a frame the host checks would have refused: nothing of it is read or written
    if (!wa_window(f0, fs, L, hw)) return;
    const long long c = (long long)rnd((double)i * shift * fs);
    const double T0 = fs / f0, n0d = rnd(T0), delta = T0 - n0d;
    const long long n0 = (long long)n0d, c1 = c - (n0 >> 1), c2 = c1 + n0;

    fill_twiddles(wq, M);
    frame_fill(a1, wav, N, c1, hw, M, wa_hann(hw));
    frame_fill(a2, wav, N, c2, hw, M, wa_hann(hw));
    fft_forward2(a1, a2, wq, logM);
    unpack_real(a1, logM);
    unpack_real(a2, logM);

    // (D_k, E_k) in the place of X1_k
    for (int k = tid; k < M; k += nthr) {
        double s, cs;
        if (k == 0) {
            const double2 x1 = a1[0], x2 = a2[0];
            sincospi(delta, &s, &cs);                           // bin M: 2 pi M delta / L = pi delta
            const double d0 = x1.x - x2.x, dr = x1.y - x2.y * cs, di = -x2.y * s;
            a1[0] = make_double2(0.5 * (d0 * d0), 0.5 * (x1.x * x1.x + x2.x * x2.x));
            xm[0] = make_double2(0.5 * (dr * dr + di * di), 0.5 * (x1.y * x1.y + x2.y * x2.y));
        } else {
            const int rk = bitrev(k, logM);
            const double2 x1 = a1[rk], x2 = a2[rk];
            sincospi(2.0 * (double)k * delta / (double)L, &s, &cs);
            a1[rk] = make_double2(0.5 * wa_mag2(csub(x1, cmul(x2, make_double2(cs, s)))), 0.5 * (wa_mag2(x1) + wa_mag2(x2)));
        }
    }
    __syncthreads();
    // the band axis out of global memory, once per workgroup: the band sums below walk LDS alone
    for (int k = tid; k < K; k += nthr) {
        int b;
        double fr;
        band_of(fw, Kp, nb, k, b, fr);
        (k < M ? a2[k] : xm[1]) = make_double2((double)b, fr);
    }
    __syncthreads();

    // W[k,b] = 1 - fraction where b is the bin's lower band, the fraction where it is the band above; the band index ascends with
    // k, so band b's bins are the run between two binary searches; the bins below f0 (k < kappa) carry no weight
    const double kappa = f0 * (double)L / fs;
    const int kmin = (int)ceil(kappa);
    auto first_bin = [&](int want) {
        int lo = 0, hi = K;
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if ((int)(mid < M ? a2[mid] : xm[1]).x >= want) hi = mid; else lo = mid + 1;
        }
        return lo;
    };
    // G lanes of one wave share a band (G a power of two, as many as the workgroup has for nb bands, a function of nb and L
    // alone): lane g sums the g-th of G equal stretches of the band's bins, ascending, and the band's first lane adds the G
    // partial sums, ascending.  Every lane of a wave runs the same number of rounds, so the shuffles see all of them.
    int G = 1;
    while (G < 64 && nb * (G << 1) <= nthr) G <<= 1;
    const int units = nb * G;
    for (int u0 = 0; u0 < units; u0 += nthr) {
        const int u = u0 + tid, b = u / G, g = u % G;
        double num = 0.0, den = 0.0;
        if (u < units) {
            int lo = first_bin(b - 1);
            const int hi = first_bin(b + 1);
            lo = lo < kmin ? kmin : lo;
            const int piece = hi > lo ? (hi - lo + G - 1) / G : 0, k0 = lo + g * piece, k1 = k0 + piece < hi ? k0 + piece : hi;
            for (int k = k0; k < k1; ++k) {
                const double2 wt = k < M ? a2[k] : xm[1];
                const int bk = (int)wt.x;
                const double w = bk == b ? 1.0 - wt.y : (bk == b - 1 ? wt.y : 0.0);
                const double2 de = k == 0 ? a1[0] : (k == M ? xm[0] : a1[bitrev(k, logM)]);
                num += w * de.x;
                den += w * de.y;
            }
        }
        const int first = (tid & 63) - g;
        double tnum = 0.0, tden = 0.0;
        for (int j = 0; j < G; ++j) {
            tnum += __shfl(num, first + j, 64);
            tden += __shfl(den, first + j, 64);
        }
        if (u < units && g == 0) rho[b] = tden > 0.0 ? tnum / tden : -1.0;
    }
    __syncthreads();
    for (int b = tid; b < nb; b += nthr) {
        double r = rho[b];
        for (int bb = b + 1; r < 0.0 && bb < nb; ++bb) r = rho[bb];
        double db = 0.0;
        if (!(r < 0.0)) {
            r = r < 1e-6 ? 1e-6 : (r > 1.0 ? 1.0 : r);
            db = 10.0 * log10(r);
        }
        row[b] = (float)db;
    }
}

// One workgroup per frame.
__global__ __launch_bounds__(WA_THREADS) void world_aperiodicity_kernel(const float* __restrict__ wav, const long long N,
                                                                        const float* __restrict__ f0v,
                                                                        const float* __restrict__ voicedv, float* __restrict__ aper,
                                                                        const int nb, const int Kp, const int logM,
                                                                        const double shift, const double fs,
                                                                        const double* __restrict__ fw) {
    world_aperiodicity_frame(wav, N, f0v, voicedv, aper, blockIdx.x, nb, Kp, logM, shift, fs, fw);
}

// One workgroup per frame of the packed batch.
__global__ __launch_bounds__(WA_THREADS) void world_aperiodicity_batch_kernel(const float* __restrict__ wav, const long long* __restrict__ wav_off,
                                                                              const long long wav_total, const long long* __restrict__ frame_off,
                                                                              const int B, const int T, const float* __restrict__ f0v,
                                                                              const float* __restrict__ voicedv, float* __restrict__ aper,
                                                                              const int nb, const int Kp, const int logM, const double shift,
                                                                              const double fs, const double* __restrict__ fw) {
    const PackedFrame f = packed_frame(wav_off, wav_total, frame_off, B, T, blockIdx.x);
    if (!f.ok) return;
    world_aperiodicity_frame(wav + f.woff, f.N, f0v + f.foff, voicedv + f.foff, aper + (size_t)f.foff * nb, f.i, nb, Kp, logM, shift, fs, fw);
}

}  // namespace ptts

using namespace ptts;

extern "C" int ptts_world_envelope(const float* wav, long long N, const float* rate, float* spec, int T, double shift, double fs,
                                   int dftlen, int log_out, void* stream) {
    PTTS_REQUIRE(T >= 0 && N >= 0, "world_envelope: T=%d N=%lld", T, N);
    const int logL = frame_log2(dftlen);
    PTTS_REQUIRE(logL > 0, "world_envelope: dftlen=%d is not a power of two in [%d, %d]", dftlen, FRAME_MIN_DFTLEN, FRAME_MAX_DFTLEN);
    PTTS_REQUIRE(fs > 0.0 && fs < 1e9, "world_envelope: fs=%g", fs);
    PTTS_REQUIRE(shift > 0.0 && shift < 1e3, "world_envelope: shift=%g", shift);
    if (T == 0) return PTTS_OK;
    PTTS_REQUIRE(rate && spec && (wav || N == 0), "world_envelope: null tensor");
    const int M = dftlen / 2;
    const int lds = (M + M / 4) * (int)sizeof(double2) + (M + 1) * (int)sizeof(double);
    const int rc = reserve_lds<world_envelope_kernel>("world_envelope", lds);
    if (rc != PTTS_OK) return rc;
    hipLaunchKernelGGL(world_envelope_kernel, dim3(T), dim3(frame_threads(M, WA_THREADS)), (size_t)lds, (hipStream_t)stream, wav, N, rate,
                       spec, logL - 1, shift, fs, log_out != 0);
    return check_launch("world_envelope");
}

extern "C" int ptts_world_aperiodicity(const float* wav, long long N, const float* f0, const float* voiced, float* aper, int T, int nb,
                                       double shift, double fs, int dftlen, const double* fwtable, size_t fwtable_bytes,
                                       void* stream) {
    PTTS_REQUIRE(T >= 0 && N >= 0, "world_aperiodicity: T=%d N=%lld", T, N);
    PTTS_REQUIRE(nb >= 2 && nb <= WA_MAX_NB, "world_aperiodicity: nb=%d outside [2, %d]", nb, WA_MAX_NB);
    const int logL = frame_log2(dftlen);
    PTTS_REQUIRE(logL > 0, "world_aperiodicity: dftlen=%d is not a power of two in [%d, %d]", dftlen, FRAME_MIN_DFTLEN,
                 FRAME_MAX_DFTLEN);
    PTTS_REQUIRE(fs > 0.0 && fs < 1e9, "world_aperiodicity: fs=%g", fs);
    PTTS_REQUIRE(shift > 0.0 && shift < 1e3, "world_aperiodicity: shift=%g", shift);
    if (T == 0) return PTTS_OK;
    PTTS_REQUIRE(f0 && voiced && aper && (wav || N == 0), "world_aperiodicity: null tensor");
    PTTS_REQUIRE(fwtable && ((size_t)fwtable & 31) == 0 && fwtable_bytes >= ptts_fwbnd_table_bytes(dftlen),
                 "world_aperiodicity: the table of ptts_fwbnd_table(dftlen=%d) needs %zu aligned bytes, got %zu", dftlen,
                 ptts_fwbnd_table_bytes(dftlen), fwtable_bytes);
    const int M = dftlen / 2, Kp = (M + 1 + 3) / 4 * 4;
    const int lds = (2 * M + M / 4 + 2) * (int)sizeof(double2) + nb * (int)sizeof(double);
    const int rc = reserve_lds<world_aperiodicity_kernel>("world_aperiodicity", lds);
    if (rc != PTTS_OK) return rc;
    hipLaunchKernelGGL(world_aperiodicity_kernel, dim3(T), dim3(frame_threads(M, WA_THREADS)), (size_t)lds, (hipStream_t)stream, wav, N,
                       f0, voiced, aper, nb, Kp, logL - 1, shift, fs, fwtable);
    return check_launch("world_aperiodicity");
}

extern "C" int ptts_world_envelope_batch(const float* wav, const long long* wav_off, long long wav_total, const long long* frame_off, int B,
                                         int T, const float* rate, float* spec, double shift, double fs, int dftlen, int log_out,
                                         void* stream) {
    PTTS_REQUIRE(T >= 0 && wav_total >= 0 && B >= 0 && B <= PACKED_MAX_UTTS, "world_envelope_batch: T=%d wav_total=%lld B=%d", T, wav_total, B);
    const int logL = frame_log2(dftlen);
    PTTS_REQUIRE(logL > 0, "world_envelope_batch: dftlen=%d is not a power of two in [%d, %d]", dftlen, FRAME_MIN_DFTLEN, FRAME_MAX_DFTLEN);
    PTTS_REQUIRE(fs > 0.0 && fs < 1e9, "world_envelope_batch: fs=%g", fs);
    PTTS_REQUIRE(shift > 0.0 && shift < 1e3, "world_envelope_batch: shift=%g", shift);
    if (T == 0 || B == 0) return PTTS_OK;
    PTTS_REQUIRE(rate && spec && wav_off && frame_off && (wav || wav_total == 0), "world_envelope_batch: null tensor");
    const int M = dftlen / 2;
    const int lds = (M + M / 4) * (int)sizeof(double2) + (M + 1) * (int)sizeof(double);
    const int rc = reserve_lds<world_envelope_batch_kernel>("world_envelope_batch", lds);
    if (rc != PTTS_OK) return rc;
    hipLaunchKernelGGL(world_envelope_batch_kernel, dim3(T), dim3(frame_threads(M, WA_THREADS)), (size_t)lds, (hipStream_t)stream, wav, wav_off,
                       wav_total, frame_off, B, T, rate, spec, logL - 1, shift, fs, log_out != 0);
    return check_launch("world_envelope_batch");
}

extern "C" int ptts_world_aperiodicity_batch(const float* wav, const long long* wav_off, long long wav_total, const long long* frame_off,
                                             int B, int T, const float* f0, const float* voiced, float* aper, int nb, double shift,
                                             double fs, int dftlen, const double* fwtable, size_t fwtable_bytes, void* stream) {
    PTTS_REQUIRE(T >= 0 && wav_total >= 0 && B >= 0 && B <= PACKED_MAX_UTTS, "world_aperiodicity_batch: T=%d wav_total=%lld B=%d", T, wav_total,
                 B);
    PTTS_REQUIRE(nb >= 2 && nb <= WA_MAX_NB, "world_aperiodicity_batch: nb=%d outside [2, %d]", nb, WA_MAX_NB);
    const int logL = frame_log2(dftlen);
    PTTS_REQUIRE(logL > 0, "world_aperiodicity_batch: dftlen=%d is not a power of two in [%d, %d]", dftlen, FRAME_MIN_DFTLEN,
                 FRAME_MAX_DFTLEN);
    PTTS_REQUIRE(fs > 0.0 && fs < 1e9, "world_aperiodicity_batch: fs=%g", fs);
    PTTS_REQUIRE(shift > 0.0 && shift < 1e3, "world_aperiodicity_batch: shift=%g", shift);
    if (T == 0 || B == 0) return PTTS_OK;
    PTTS_REQUIRE(f0 && voiced && aper && wav_off && frame_off && (wav || wav_total == 0), "world_aperiodicity_batch: null tensor");
    PTTS_REQUIRE(fwtable && ((size_t)fwtable & 31) == 0 && fwtable_bytes >= ptts_fwbnd_table_bytes(dftlen),
                 "world_aperiodicity_batch: the table of ptts_fwbnd_table(dftlen=%d) needs %zu aligned bytes, got %zu", dftlen,
                 ptts_fwbnd_table_bytes(dftlen), fwtable_bytes);
    const int M = dftlen / 2, Kp = (M + 1 + 3) / 4 * 4;
    const int lds = (2 * M + M / 4 + 2) * (int)sizeof(double2) + nb * (int)sizeof(double);
    const int rc = reserve_lds<world_aperiodicity_batch_kernel>("world_aperiodicity_batch", lds);
    if (rc != PTTS_OK) return rc;
    hipLaunchKernelGGL(world_aperiodicity_batch_kernel, dim3(T), dim3(frame_threads(M, WA_THREADS)), (size_t)lds, (hipStream_t)stream, wav,
                       wav_off, wav_total, frame_off, B, T, f0, voiced, aper, nb, Kp, logL - 1, shift, fs, fwtable);
    return check_launch("world_aperiodicity_batch");
}
