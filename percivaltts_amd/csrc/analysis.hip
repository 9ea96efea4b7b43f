// Waveform analysis for the PML parameters: the counterpart of pulsesynth.hip (the step behind the reference's run.py:146-153,
// whose pulsemodel submodule is absent from the reference checkout: the definition is this build's own).
// Notation: L = dftlen, M = L/2, K = M + 1 bins, rnd(x) = floor(x + 0.5); frame i sits at t_i = i shift and has f0_i Hz.
//
// frame spectrum   c = rnd(t_i fs), hw = int(1.5 fs / f0_i), w = blackman(2 hw + 1) / (0.84 hw) (0.84 hw is the window's sum),
//                  x[j mod L] = wav[c + j] w[j + hw], j = -hw .. hw (zero-phase placement, samples outside [0, N) are 0), X = rfft(x)
// harmonics        H_i = floor((fs/2 - f0_i/2) / f0_i);  p_h = max |X_k|, k in [rnd((h - 1/2) f0_i L / fs), rnd((h + 1/2) f0_i L / fs)),
//                  a_h = ln(max(p_h fs / f0_i, 1e-10)), h = 1 .. H_i
// envelope         ln SPEC[i,k] = a_h interpolated linearly at k fs / L between the h f0_i, held below f0_i and above H_i f0_i
// phasor           k_h = rnd(h f0_i L / fs), z = X[k_{h+1}] conj(X[k_h]) conj(X[k_1]), u[i,h-1] = z / |z| ((0,0) where |z| < 1e-300),
//                  h = 1 .. H_i - 1; the columns behind are (0,0)
// coherence        J_i = max(2, rnd(1 / (f0_i shift))), R[i,h-1] = |sum_m u[m,h-1]| / n over the n frames m in [i-J_i, i+J_i] that exist
//                  and have h < H_m, in ascending m; 1 for h >= H_i.  Harmonic h is noisy iff R < exp(-0.75^2 / 2).
// bin mask         bin k takes the flag of h = clip(floor(k fs / (L f0_i)), 1, H_i - 1)
// band axis        W[k,b]: the hat weight with which ptts_fwbnd2spec reads band b at bin k (1 - fraction at the bin's lower band,
//                  the fraction at the band above), from the band / fraction rows of ptts_fwbnd_table
// noise bands      NM[i,b] = sum_k W[k,b] mask[i,k] / sum_k W[k,b]
// compression      mean: out[t,b] = sum_k W[k,b] x[t,k] / sum_k W[k,b];  lsq: (W^T W) y = W^T v, v = ln max(|x|, FLT_MIN) or x itself.
//                  W^T W is tridiagonal; ptts_fwbnd_compress_table factorises it once (the Thomas recurrences, fp64).
//
// Integer decisions (c, hw, H_i, J_i, every bin index) are taken in fp64 from the fp32 inputs with the operation order written
// here (the build has no fused contraction), so that a host restatement takes the same ones.  Arithmetic is fp64, results are
// rounded to fp32 once.  One workgroup per frame holds ONE packed L-point buffer, a quarter circle of twiddles and the a_h:
// 1.25 M complex fp64 = 40 KiB at L = 4096, 80 KiB at 8192.  Every sum runs in a fixed order inside one lane (bins ascending,
// frames ascending); nothing here uses an atomic and a result does not depend on the grid.
#include "common.h"
#include "frame.h"

namespace ptts {

constexpr int AN_THREADS = 256;
constexpr int AN_MAX_HCAP = 8192;                       // harmonics a frame may have: below K at the largest dftlen
constexpr int AN_MAX_NB = 1024;
constexpr int CT_ROWS = 6;                              // rows of the compress table: klo, khi, sum_k W, e_b, 1 / m_b, c'_b
constexpr int CT_FRAMES = AN_THREADS / 64;              // frames of one ptts_fwbnd_compress workgroup: a wave each
constexpr double AN_NOISY_BELOW = 0.75483960198900735;  // exp(-0.75^2 / 2)
constexpr double AN_FLT_MIN = 1.17549435082228751e-38;

// H = floor((fs/2 - f0/2) / f0) as a double; f0 > 0
__device__ __forceinline__ double harmonics_of(double f0, double fs) { return floor((0.5 * fs - 0.5 * f0) / f0); }

// Frame i of one utterance: wav [N] its samples, f0v, spec and u its own rows.  The workgroup's work; dynamic LDS:
// (M + M/4) double2 + (Hcap + 2) doubles.
__device__ __forceinline__ void frame_harmonics_frame(const float* __restrict__ wav, const long long N, const float* __restrict__ f0v,
                                                      float* __restrict__ spec, float* __restrict__ u, const int i, const int Hcap,
                                                      const int logM, const double shift, const double fs, const bool log_out) {
    extern __shared__ double2 lds[];
    const int M = 1 << logM, L = M << 1, K = M + 1, Mq = M >> 2;
    double2* a = lds;
    double2* wq = lds + M;
    double* ah = reinterpret_cast<double*>(lds + M + Mq);       // a_h at [h], h = 1 .. H
    const int tid = threadIdx.x, nthr = blockDim.x;
    const double f0 = (double)f0v[i];
    // a frame the host checks would have refused: nothing of it is read or written
    if (!(f0 > 0.0) || !(f0 < fs)) return;
    const double hwd = 1.5 * fs / f0, Hd = harmonics_of(f0, fs);
    if (!(hwd < (double)L) || 2 * (int)hwd + 1 > L || !(Hd >= 1.0) || !(Hd <= (double)(Hcap + 1))) return;
    const int hw = (int)hwd, H = (int)Hd;
    const long long c = (long long)rnd((double)i * shift * fs);

    fill_twiddles(wq, M);
    const double wnorm = 1.0 / (0.84 * (double)hw);
    frame_fill(a, wav, N, c, hw, M, [&](int j) {        // blackman(2 hw + 1) / (0.84 hw)
        const double r = (double)(j + hw) / (double)hw;
        return (0.42 - 0.5 * cospi(r) + 0.08 * cospi(2.0 * r)) * wnorm;
    });
    fft_forward(a, wq, logM);
    unpack_real(a, logM);

    for (int h = 1 + tid; h <= H; h += nthr) {
        long long lo = (long long)rnd(((double)h - 0.5) * f0 * (double)L / fs), hi = (long long)rnd(((double)h + 0.5) * f0 * (double)L / fs);
        lo = lo < 0 ? 0 : lo;
        hi = hi > K ? K : hi;
        double p2 = 0.0;
        for (long long k = lo; k < hi; ++k) {
            const double2 x = spectrum_bin(a, (int)k, logM);
            const double m2 = x.x * x.x + x.y * x.y;
            p2 = m2 > p2 ? m2 : p2;
        }
        const double amp = sqrt(p2) * fs / f0;
        ah[h] = log(amp > 1e-10 ? amp : 1e-10);
    }
    __syncthreads();

    float* urow = u + (size_t)i * Hcap * 2;
    const long long k1l = (long long)rnd(1.0 * f0 * (double)L / fs);
    const int k1 = (int)(k1l > M ? M : k1l);
    for (int j = tid; j < Hcap; j += nthr) {
        const int h = j + 1;
        double2 o = make_double2(0.0, 0.0);
        if (h <= H - 1) {
            long long ka = (long long)rnd((double)h * f0 * (double)L / fs), kb = (long long)rnd((double)(h + 1) * f0 * (double)L / fs);
            ka = ka > M ? M : ka;
            kb = kb > M ? M : kb;
            const double2 z = cmul(cmul(spectrum_bin(a, (int)kb, logM), cconj(spectrum_bin(a, (int)ka, logM))),
                                   cconj(spectrum_bin(a, k1, logM)));
            const double mag = hypot(z.x, z.y);
            if (!(mag < 1e-300)) o = make_double2(z.x / mag, z.y / mag);
        }
        urow[2 * j] = (float)o.x;
        urow[2 * j + 1] = (float)o.y;
    }

    float* srow = spec + (size_t)i * K;
    for (int k = tid; k < K; k += nthr) {
        const double x = (double)k * fs / (double)L / f0;
        double v;
        if (x < 1.0) v = ah[1];
        else if (x >= (double)H) v = ah[H];
        else {
            const int h0 = (int)x;
            v = ah[h0] + (x - (double)h0) * (ah[h0 + 1] - ah[h0]);
        }
        srow[k] = (float)(log_out ? v : exp(v));
    }
}

// One workgroup per frame.
__global__ __launch_bounds__(AN_THREADS) void frame_harmonics_kernel(const float* __restrict__ wav, const long long N,
                                                                     const float* __restrict__ f0v, float* __restrict__ spec,
                                                                     float* __restrict__ u, const int Hcap, const int logM,
                                                                     const double shift, const double fs, const bool log_out) {
    frame_harmonics_frame(wav, N, f0v, spec, u, blockIdx.x, Hcap, logM, shift, fs, log_out);
}

// One workgroup per frame of the packed batch.
__global__ __launch_bounds__(AN_THREADS) void frame_harmonics_batch_kernel(const float* __restrict__ wav, const long long* __restrict__ wav_off,
                                                                           const long long wav_total, const long long* __restrict__ frame_off,
                                                                           const int B, const int T, const float* __restrict__ f0v,
                                                                           float* __restrict__ spec, float* __restrict__ u, const int Hcap,
                                                                           const int logM, const double shift, const double fs,
                                                                           const bool log_out) {
    const PackedFrame f = packed_frame(wav_off, wav_total, frame_off, B, T, blockIdx.x);
    if (!f.ok) return;
    frame_harmonics_frame(wav + f.woff, f.N, f0v + f.foff, spec + (size_t)f.foff * ((1 << logM) + 1), u + (size_t)f.foff * Hcap * 2, f.i, Hcap,
                          logM, shift, fs, log_out);
}

// W[k,b] from the band / fraction rows of the fwbnd table (band indices clamped, whatever the table holds)
__device__ __forceinline__ double hat_weight(const double* __restrict__ fw, int Kp, int nb, int k, int b) {
    int bk;
    double fr;
    band_of(fw, Kp, nb, k, bk, fr);
    return bk == b ? 1.0 - fr : (bk == b - 1 ? fr : 0.0);
}

// the bins [lo, hi) of band b, clamped to [0, K]
__device__ __forceinline__ void band_bins(const double* __restrict__ ct, int nbp, int b, int K, int& lo, int& hi) {
    const double l = ct[b], h = ct[(size_t)nbp + b];
    lo = l >= 0.0 && l <= (double)K ? (int)l : K;
    hi = h >= 0.0 && h <= (double)K ? (int)h : K;
}

// The scalars of a ptts_phase_coherence launch that every frame shares
struct CoherenceArgs {
    int Hcap, nb, nbp, K, Kp, L;
    double shift, fs;
    const double* fw;
    const double* ct;
};

// Frame i of one utterance of T frames: u, f0v, R and nm its own rows, so the neighbourhood m0 .. m1 and the clamp J <= T are the
// utterance's.  The workgroup's work; dynamic LDS: Hcap ints (the harmonics' flags).
__device__ __forceinline__ void phase_coherence_frame(const float* __restrict__ u, const float* __restrict__ f0v, float* __restrict__ R,
                                                      float* __restrict__ nm, const int i, const int T, const CoherenceArgs& A) {
    extern __shared__ int noisy[];
    const int Hcap = A.Hcap, nb = A.nb, nbp = A.nbp, K = A.K, Kp = A.Kp, L = A.L;
    const double shift = A.shift, fs = A.fs;
    const double* __restrict__ fw = A.fw;
    const double* __restrict__ ct = A.ct;
    const int tid = threadIdx.x, nthr = blockDim.x;
    const double f0 = (double)f0v[i];
    int H = 0, J = 2;
    if (f0 > 0.0 && f0 < fs) {
        const double Hd = harmonics_of(f0, fs), Jd = rnd(1.0 / (f0 * shift));
        H = Hd < 0.0 ? 0 : (Hd > (double)(Hcap + 1) ? Hcap + 1 : (int)Hd);
        J = Jd > (double)T ? T : (Jd < 2.0 ? 2 : (int)Jd);
    }
    const int m0 = i - J < 0 ? 0 : i - J, m1 = i + J > T - 1 ? T - 1 : i + J;
    for (int j = tid; j < Hcap; j += nthr) {
        double r = 1.0;
        if (j + 1 <= H - 1) {
            double sx = 0.0, sy = 0.0;
            int n = 0;
            for (int m = m0; m <= m1; ++m) {
                const double fm = (double)f0v[m];
                if (!(fm > 0.0 && fm < fs) || !((double)(j + 1) < harmonics_of(fm, fs))) continue;
                sx += (double)u[((size_t)m * Hcap + j) * 2];
                sy += (double)u[((size_t)m * Hcap + j) * 2 + 1];
                ++n;
            }
            r = n > 0 ? sqrt(sx * sx + sy * sy) / (double)n : 1.0;
        }
        noisy[j] = r < AN_NOISY_BELOW ? 1 : 0;
        R[(size_t)i * Hcap + j] = (float)r;
    }
    __syncthreads();
    for (int b = tid; b < nb; b += nthr) {
        int lo, hi;
        band_bins(ct, nbp, b, K, lo, hi);
        double acc = 0.0;
        if (H >= 2) {
            for (int k = lo; k < hi; ++k) {
                const double hd = floor((double)k * fs / ((double)L * f0));
                const int h = hd < 1.0 ? 1 : (hd > (double)(H - 1) ? H - 1 : (int)hd);
                acc += hat_weight(fw, Kp, nb, k, b) * (double)noisy[h - 1];
            }
        }
        const double s = ct[2 * (size_t)nbp + b];
        nm[(size_t)i * nb + b] = (float)(s > 0.0 ? acc / s : 0.0);
    }
}

// One workgroup per frame.
__global__ __launch_bounds__(AN_THREADS) void phase_coherence_kernel(const float* __restrict__ u, const float* __restrict__ f0v,
                                                                     float* __restrict__ R, float* __restrict__ nm, const int T,
                                                                     const CoherenceArgs A) {
    phase_coherence_frame(u, f0v, R, nm, blockIdx.x, T, A);
}

// One workgroup per frame of the packed batch: a frame sees the rows of its own utterance alone.
__global__ __launch_bounds__(AN_THREADS) void phase_coherence_batch_kernel(const float* __restrict__ u, const float* __restrict__ f0v,
                                                                           float* __restrict__ R, float* __restrict__ nm,
                                                                           const long long* __restrict__ frame_off, const int B,
                                                                           const int T, const CoherenceArgs A) {
    const PackedFrame f = packed_frame(nullptr, 0, frame_off, B, T, blockIdx.x);
    if (!f.ok) return;
    phase_coherence_frame(u + (size_t)f.foff * A.Hcap * 2, f0v + f.foff, R + (size_t)f.foff * A.Hcap, nm + (size_t)f.foff * A.nb, f.i, f.T, A);
}

// One workgroup.  The band index row of the fwbnd table ascends with k, so a band's bins are the run between two binary searches.
__global__ __launch_bounds__(AN_THREADS) void compress_table_kernel(double* __restrict__ ct, const double* __restrict__ fw, const int nb,
                                                                    const int nbp, const int K, const int Kp) {
    __shared__ double d[AN_MAX_NB], e[AN_MAX_NB];
    const int tid = threadIdx.x, nthr = blockDim.x;
    for (int b = tid; b < nbp; b += nthr) {
        if (b >= nb) {
            for (int r = 0; r < CT_ROWS; ++r) ct[(size_t)r * nbp + b] = 0.0;
            continue;
        }
        int bound[2];
#pragma unroll
        for (int q = 0; q < 2; ++q) {                   // the first bin whose lower band is at least b - 1 / b + 1
            const int want = q == 0 ? b - 1 : b + 1;
            int lo = 0, hi = K;
            while (lo < hi) {
                const int mid = (lo + hi) >> 1;
                if (lower_band(fw, nb, mid) >= want) hi = mid; else lo = mid + 1;
            }
            bound[q] = lo;
        }
        double s = 0.0, dd = 0.0, ee = 0.0;
        for (int k = bound[0]; k < bound[1]; ++k) {
            const double w = hat_weight(fw, Kp, nb, k, b);
            s += w;
            dd += w * w;
            if (b + 1 < nb) ee += w * hat_weight(fw, Kp, nb, k, b + 1);
        }
        ct[b] = (double)bound[0];
        ct[(size_t)nbp + b] = (double)bound[1];
        ct[2 * (size_t)nbp + b] = s;
        d[b] = dd;
        e[b] = ee;
    }
    __syncthreads();
    if (tid == 0) {
        double m = d[0];
        for (int b = 0; b < nb; ++b) {
            const double inv = m > 0.0 ? 1.0 / m : 0.0, cp = e[b] * inv;
            ct[3 * (size_t)nbp + b] = e[b];
            ct[4 * (size_t)nbp + b] = inv;
            ct[5 * (size_t)nbp + b] = cp;
            if (b + 1 < nb) m = d[b + 1] - e[b] * cp;
        }
    }
}

// One wave per frame, CT_FRAMES frames per workgroup.  dynamic LDS: CT_FRAMES * nb doubles (the right-hand sides, then y).
__global__ __launch_bounds__(AN_THREADS) void fwbnd_compress_kernel(const float* __restrict__ x, float* __restrict__ out, const int T,
                                                                    const int nb, const int nbp, const int K, const int Kp,
                                                                    const bool lsq, const bool is_log, const double* __restrict__ fw,
                                                                    const double* __restrict__ ct) {
    extern __shared__ double rhs[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long long t = (long long)blockIdx.x * CT_FRAMES + wave;
    const bool live = t < T;
    double* y = rhs + (size_t)wave * nb;
    if (live) {
        const float* row = x + (size_t)t * K;
        for (int b = lane; b < nb; b += 64) {
            int lo, hi;
            band_bins(ct, nbp, b, K, lo, hi);
            double acc = 0.0;
            for (int k = lo; k < hi; ++k) {
                double v = (double)row[k];
                if (lsq && !is_log) {
                    v = fabs(v);
                    v = log(v > AN_FLT_MIN ? v : AN_FLT_MIN);
                }
                acc += hat_weight(fw, Kp, nb, k, b) * v;
            }
            if (lsq) {
                y[b] = acc;
            } else {
                const double s = ct[2 * (size_t)nbp + b];
                out[(size_t)t * nb + b] = (float)(s > 0.0 ? acc / s : 0.0);
            }
        }
    }
    if (!lsq) return;
    __syncthreads();
    if (live && lane == 0) {                            // y'_b = (r_b - e_{b-1} y'_{b-1}) / m_b;  y_b = y'_b - c'_b y_{b+1}
        const double* e = ct + 3 * (size_t)nbp;
        const double* inv = ct + 4 * (size_t)nbp;
        const double* cp = ct + 5 * (size_t)nbp;
        double prev = y[0] * inv[0];
        y[0] = prev;
        for (int b = 1; b < nb; ++b) {
            prev = (y[b] - e[b - 1] * prev) * inv[b];
            y[b] = prev;
        }
        for (int b = nb - 2; b >= 0; --b) {
            prev = y[b] - cp[b] * prev;
            y[b] = prev;
        }
    }
    __syncthreads();
    if (live)
        for (int b = lane; b < nb; b += 64) out[(size_t)t * nb + b] = (float)y[b];
}

static int an_padded_bins(int dftlen) { return (dftlen / 2 + 1 + 3) / 4 * 4; }
static int an_padded_bands(int nb) { return (nb + 3) / 4 * 4; }
static bool an_dftlen_even(int dftlen) { return dftlen >= 8 && dftlen % 2 == 0 && dftlen <= (1 << 20); }

// the two tables of the band axis as an entry point has to find them
static int band_tables(const char* what, int nb, int dftlen, const double* fw, size_t fw_bytes, const double* ct, size_t ct_bytes) {
    PTTS_REQUIRE(fw && ((size_t)fw & 31) == 0 && fw_bytes >= ptts_fwbnd_table_bytes(dftlen),
                 "%s: the table of ptts_fwbnd_table(dftlen=%d) needs %zu aligned bytes, got %zu", what, dftlen,
                 ptts_fwbnd_table_bytes(dftlen), fw_bytes);
    PTTS_REQUIRE(ct && ((size_t)ct & 31) == 0 && ct_bytes >= ptts_fwbnd_compress_table_bytes(nb),
                 "%s: the table of ptts_fwbnd_compress_table(nb=%d) needs %zu aligned bytes, got %zu", what, nb,
                 ptts_fwbnd_compress_table_bytes(nb), ct_bytes);
    return PTTS_OK;
}

}  // namespace ptts

using namespace ptts;

static int frame_harmonics_args(const char* what, int Hcap, double shift, double fs, int dftlen, int& logL, int& lds) {
    PTTS_REQUIRE(Hcap >= 1 && Hcap <= AN_MAX_HCAP, "%s: Hcap=%d outside [1, %d]", what, Hcap, AN_MAX_HCAP);
    logL = frame_log2(dftlen);
    PTTS_REQUIRE(logL > 0, "%s: dftlen=%d is not a power of two in [%d, %d]", what, dftlen, FRAME_MIN_DFTLEN, FRAME_MAX_DFTLEN);
    PTTS_REQUIRE(fs > 0.0 && fs < 1e9, "%s: fs=%g", what, fs);
    PTTS_REQUIRE(shift > 0.0 && shift < 1e3, "%s: shift=%g", what, shift);
    const int M = dftlen / 2;
    lds = (M + M / 4) * (int)sizeof(double2) + (Hcap + 2) * (int)sizeof(double);
    return PTTS_OK;
}

extern "C" int ptts_frame_harmonics(const float* wav, long long N, const float* f0, float* spec, float* u, int T, int Hcap, double shift,
                                    double fs, int dftlen, int log_out, void* stream) {
    PTTS_REQUIRE(T >= 0 && N >= 0, "frame_harmonics: T=%d N=%lld", T, N);
    int logL, lds;
    int rc = frame_harmonics_args("frame_harmonics", Hcap, shift, fs, dftlen, logL, lds);
    if (rc != PTTS_OK) return rc;
    if (T == 0) return PTTS_OK;
    PTTS_REQUIRE(f0 && spec && u && (wav || N == 0), "frame_harmonics: null tensor");
    rc = reserve_lds<frame_harmonics_kernel>("frame_harmonics", lds);
    if (rc != PTTS_OK) return rc;
    hipLaunchKernelGGL(frame_harmonics_kernel, dim3(T), dim3(frame_threads(dftlen / 2, AN_THREADS)), (size_t)lds, (hipStream_t)stream, wav, N,
                       f0, spec, u, Hcap, logL - 1, shift, fs, log_out != 0);
    return check_launch("frame_harmonics");
}

extern "C" int ptts_frame_harmonics_batch(const float* wav, const long long* wav_off, long long wav_total, const long long* frame_off, int B,
                                          int T, const float* f0, float* spec, float* u, int Hcap, double shift, double fs, int dftlen,
                                          int log_out, void* stream) {
    PTTS_REQUIRE(T >= 0 && wav_total >= 0 && B >= 0 && B <= PACKED_MAX_UTTS, "frame_harmonics_batch: T=%d wav_total=%lld B=%d", T, wav_total, B);
    int logL, lds;
    int rc = frame_harmonics_args("frame_harmonics_batch", Hcap, shift, fs, dftlen, logL, lds);
    if (rc != PTTS_OK) return rc;
    if (T == 0 || B == 0) return PTTS_OK;
    PTTS_REQUIRE(f0 && spec && u && wav_off && frame_off && (wav || wav_total == 0), "frame_harmonics_batch: null tensor");
    rc = reserve_lds<frame_harmonics_batch_kernel>("frame_harmonics_batch", lds);
    if (rc != PTTS_OK) return rc;
    hipLaunchKernelGGL(frame_harmonics_batch_kernel, dim3(T), dim3(frame_threads(dftlen / 2, AN_THREADS)), (size_t)lds, (hipStream_t)stream,
                       wav, wav_off, wav_total, frame_off, B, T, f0, spec, u, Hcap, logL - 1, shift, fs, log_out != 0);
    return check_launch("frame_harmonics_batch");
}

// The checks of ptts_phase_coherence and its batched form in front of the T = 0 exit (the tables are looked at behind it)
static int phase_coherence_args(const char* what, int Hcap, int nb, double shift, double fs, int dftlen, const double* fwtable,
                                size_t fwtable_bytes, const double* ctable, size_t ctable_bytes, CoherenceArgs& A) {
    PTTS_REQUIRE(Hcap >= 1 && Hcap <= AN_MAX_HCAP, "%s: Hcap=%d outside [1, %d]", what, Hcap, AN_MAX_HCAP);
    PTTS_REQUIRE(nb >= 2 && nb <= AN_MAX_NB, "%s: nb=%d outside [2, %d]", what, nb, AN_MAX_NB);
    PTTS_REQUIRE(frame_log2(dftlen) > 0, "%s: dftlen=%d is not a power of two in [%d, %d]", what, dftlen, FRAME_MIN_DFTLEN, FRAME_MAX_DFTLEN);
    PTTS_REQUIRE(fs > 0.0 && fs < 1e9, "%s: fs=%g", what, fs);
    PTTS_REQUIRE(shift > 0.0 && shift < 1e3, "%s: shift=%g", what, shift);
    A = CoherenceArgs{Hcap, nb, an_padded_bands(nb), dftlen / 2 + 1, an_padded_bins(dftlen), dftlen, shift, fs, fwtable, ctable};
    return PTTS_OK;
}

extern "C" int ptts_phase_coherence(const float* u, const float* f0, float* R, float* nm, int T, int Hcap, int nb, double shift, double fs,
                                    int dftlen, const double* fwtable, size_t fwtable_bytes, const double* ctable, size_t ctable_bytes,
                                    void* stream) {
    PTTS_REQUIRE(T >= 0, "phase_coherence: T=%d", T);
    CoherenceArgs A;
    int rc = phase_coherence_args("phase_coherence", Hcap, nb, shift, fs, dftlen, fwtable, fwtable_bytes, ctable, ctable_bytes, A);
    if (rc != PTTS_OK) return rc;
    if (T == 0) return PTTS_OK;
    PTTS_REQUIRE(u && f0 && R && nm, "phase_coherence: null tensor");
    rc = band_tables("phase_coherence", nb, dftlen, fwtable, fwtable_bytes, ctable, ctable_bytes);
    if (rc != PTTS_OK) return rc;
    hipLaunchKernelGGL(phase_coherence_kernel, dim3(T), dim3(AN_THREADS), (size_t)Hcap * sizeof(int), (hipStream_t)stream, u, f0, R, nm, T, A);
    return check_launch("phase_coherence");
}

extern "C" int ptts_phase_coherence_batch(const float* u, const float* f0, float* R, float* nm, const long long* frame_off, int B, int T,
                                          int Hcap, int nb, double shift, double fs, int dftlen, const double* fwtable,
                                          size_t fwtable_bytes, const double* ctable, size_t ctable_bytes, void* stream) {
    PTTS_REQUIRE(T >= 0 && B >= 0 && B <= PACKED_MAX_UTTS, "phase_coherence_batch: T=%d B=%d", T, B);
    CoherenceArgs A;
    int rc = phase_coherence_args("phase_coherence_batch", Hcap, nb, shift, fs, dftlen, fwtable, fwtable_bytes, ctable, ctable_bytes, A);
    if (rc != PTTS_OK) return rc;
    if (T == 0 || B == 0) return PTTS_OK;
    PTTS_REQUIRE(u && f0 && R && nm && frame_off, "phase_coherence_batch: null tensor");
    rc = band_tables("phase_coherence_batch", nb, dftlen, fwtable, fwtable_bytes, ctable, ctable_bytes);
    if (rc != PTTS_OK) return rc;
    hipLaunchKernelGGL(phase_coherence_batch_kernel, dim3(T), dim3(AN_THREADS), (size_t)Hcap * sizeof(int), (hipStream_t)stream, u, f0, R, nm,
                       frame_off, B, T, A);
    return check_launch("phase_coherence_batch");
}

extern "C" size_t ptts_fwbnd_compress_table_bytes(int nb) {
    if (nb < 2 || nb > AN_MAX_NB) return 16;
    return align_up((size_t)CT_ROWS * an_padded_bands(nb) * sizeof(double), 256);
}

extern "C" int ptts_fwbnd_compress_table(double* ctable, size_t ctable_bytes, const double* fwtable, size_t fwtable_bytes, int nb,
                                         int dftlen, void* stream) {
    PTTS_REQUIRE(nb >= 2 && nb <= AN_MAX_NB, "fwbnd_compress_table: nb=%d outside [2, %d]", nb, AN_MAX_NB);
    PTTS_REQUIRE(an_dftlen_even(dftlen), "fwbnd_compress_table: dftlen=%d (even, 8 .. %d)", dftlen, 1 << 20);
    const int rc = band_tables("fwbnd_compress_table", nb, dftlen, fwtable, fwtable_bytes, ctable, ctable_bytes);
    if (rc != PTTS_OK) return rc;
    hipLaunchKernelGGL(compress_table_kernel, dim3(1), dim3(AN_THREADS), 0, (hipStream_t)stream, ctable, fwtable, nb, an_padded_bands(nb),
                       dftlen / 2 + 1, an_padded_bins(dftlen));
    return check_launch("fwbnd_compress_table");
}

extern "C" int ptts_fwbnd_compress(const float* x, float* out, int T, int nb, int dftlen, int mode, int is_log, const double* fwtable,
                                   size_t fwtable_bytes, const double* ctable, size_t ctable_bytes, void* stream) {
    PTTS_REQUIRE(T >= 0, "fwbnd_compress: T=%d", T);
    PTTS_REQUIRE(nb >= 2 && nb <= AN_MAX_NB, "fwbnd_compress: nb=%d outside [2, %d]", nb, AN_MAX_NB);
    PTTS_REQUIRE(an_dftlen_even(dftlen), "fwbnd_compress: dftlen=%d (even, 8 .. %d)", dftlen, 1 << 20);
    PTTS_REQUIRE(mode == PTTS_COMPRESS_MEAN || mode == PTTS_COMPRESS_LSQ, "fwbnd_compress: mode=%d", mode);
    if (T == 0) return PTTS_OK;
    PTTS_REQUIRE(x && out, "fwbnd_compress: null tensor");
    const int rc = band_tables("fwbnd_compress", nb, dftlen, fwtable, fwtable_bytes, ctable, ctable_bytes);
    if (rc != PTTS_OK) return rc;
    hipLaunchKernelGGL(fwbnd_compress_kernel, dim3((T + CT_FRAMES - 1) / CT_FRAMES), dim3(AN_THREADS),
                       (size_t)CT_FRAMES * nb * sizeof(double), (hipStream_t)stream, x, out, T, nb, an_padded_bands(nb), dftlen / 2 + 1,
                       an_padded_bins(dftlen), mode == PTTS_COMPRESS_LSQ, is_log != 0, fwtable, ctable);
    return check_launch("fwbnd_compress");
}
