// F0 estimation: the track that analysis.hip takes from its caller (the reference runs an external pitch tracker in front of
// run.py:146-153; the estimator is this build's own, DESIGN.md section 3, after Boersma 1993: the autocorrelation method with a
// path finder).  Notation: L = dftlen, M = L/2, rnd(x) = floor(x + 0.5), N = samples; frame i is centred at c_i = rnd(i shift fs).
//
// window           hw = int(1.5 fs / f0_min), W = 2 hw + 1, w[j] = 0.5 - 0.5 cos(2 pi (j + 1) / (W + 1)) (a Hann window without its
//                  zero ends), lmin = ceil(fs / f0_max), lmax = floor(fs / f0_min), W + lmax + 1 <= L (no circular overlap);
//                  rw[k] = sum_j w[j] w[j+k] / sum_j w[j]^2, k = 0 .. lmax + 1, is the caller's fp64 table
// frame            a[j] = wav[c_i - hw + j] (0 outside [0, N)), the mean of the samples inside taken off the samples inside,
//                  lpeak = max |a|, x[j] = a[j] w[j] (zero up to L), X = rfft(x), P[k] = G(k fs / L) |X[k]|^2 with f_lp = 2.5 f0_max,
//                  G = 1 up to f_lp, cos^2(pi (f - f_lp) / f_lp) up to 1.5 f_lp, 0 above; rho = irfft(P),
//                  r[k] = (rho[k] / rho[0]) / rw[k], k = 0 .. lmax + 1 (all 0 unless rho[0] > 0)
// candidates       slot 0 is unvoiced: strength vt + max(0, 2 - (lpeak / gpeak) / (st / (1 + vt))) (vt + 2 when gpeak = 0).  A lag k in
//                  [lmin, lmax] with r[k] > r[k-1], r[k] >= r[k+1], r[k] > vt / 2 is refined by the parabola through its neighbours:
//                  d = r[k-1] - 2 r[k] + r[k+1], delta = (r[k-1] - r[k+1]) / (2 d) (0 unless d < 0),
//                  peak = r[k] - (r[k-1] - r[k+1]) delta / 4, tau = (k + delta) / fs, F = 1 / tau, kept where f0_min <= F <= f0_max,
//                  strength min(peak, 1) - octave_cost log2(f0_min tau).  The ncand - 1 strongest, strongest first, ties to the
//                  smaller lag.
// path             cost_0[j] = -S[0,j], cost_i[j] = min_p (cost_{i-1}[p] + corr trans(p, j)) - S[i,j] over the valid slots, ties to the
//                  smaller p, corr = 0.01 / shift; trans = 0 between unvoiced slots, voiced_unvoiced_cost between a voiced and an
//                  unvoiced one, octave_jump_cost |log2 F_p - log2 F_j| between voiced ones.  The last frame's smallest cost (ties to
//                  the smaller slot) is followed back.
// refinement       (ptts_f0_refine; after the published StoneMask, the definition is the build's own.)  Frame i with f = f0[i]:
//                  f > 0 false: 0, status 0.  f outside [f0_min, f0_max]: f, status 2, nothing of the waveform is read.
//                  hw = rnd(1.5 fs / f), j = -hw .. hw; c_i - hw < 0 or c_i + hw >= N: f, status 2.  u = j / (2 (hw + 1)),
//                  w_j = 0.42 + 0.5 cos(2 pi u) + 0.08 cos(4 pi u), w'_j = -(pi / (hw + 1)) (0.5 sin(2 pi u) + 0.16 sin(4 pi u));
//                  X(nu) = sum_j wav[c_i + j] w_j e^{-2 pi i nu j / fs}, Xd(nu) the same with w'_j,
//                  IF(nu) = nu - (fs / 2 pi) (Im Xd Re X - Re Xd Im X) / |X|^2.  A pass with H harmonics from g: h = 1 .. H up to
//                  the first with h g >= fs/2, nu = h g, a harmonic whose |X|^2 > 0 is false is skipped, num += |X| IF(nu),
//                  den += |X| h; den > 0 false: f, status 3; else g = num / den.  Two passes, H = 2 from g = f, then H = 6, the
//                  window that of f.  g finite, |g / f - 1| <= 0.2 and f0_min <= g <= f0_max: (float)g, status 1; else f, status 3.
//
// Data is fp32 in memory, arithmetic fp64, every decision is taken in fp64 with the operation order written here (no fused
// contraction), so that a host restatement takes the same ones.  ptts_f0_candidates: one workgroup per frame holds ONE packed
// L-point buffer (the frame, its spectrum, the power spectrum, then r in place), a quarter circle of twiddles and one strength per
// lag: 1.25 M complex fp64 + (lmax + 2) fp64, 80 KiB + 16 KiB at L = 8192.  ptts_f0_viterbi: one wave64 for the utterance, lane
// (j, p) evaluates one transition, the minimum over p is a butterfly inside the group of lanes that share j, costs stay in
// registers; back-pointers are four bits a slot, one or two words a frame, in LDS.  ptts_f0_refine: one workgroup per frame, no
// transform: the spectrum is read at the at most eight frequencies a frame needs by direct sums over the window.  No atomics, no
// polling, nothing between workgroups.
#include <climits>
#include <cmath>
#include "common.h"
#include "frame.h"

namespace ptts {

constexpr int F0_THREADS = 256;
constexpr int F0_MIN_NCAND = 2, F0_MAX_NCAND = 16;
constexpr int F0_MAX_FRAMES = 32768;                    // of ptts_f0_viterbi with one back-pointer word a frame (ncand <= 8): 128 KiB of LDS

__device__ __forceinline__ double f0_block_max(double v, double* red) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nwaves = blockDim.x >> 6;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const double t = __shfl_xor(v, o, 64);
        v = t > v ? t : v;
    }
    __syncthreads();
    if (lane == 0) red[wave] = v;
    __syncthreads();
    double m = red[0];
    for (int w = 1; w < nwaves; ++w) m = red[w] > m ? red[w] : m;
    return m;
}

// (s, k) beats (bs, bk): the larger strength, then the smaller lag
__device__ __forceinline__ bool f0_stronger(double s, int k, double bs, int bk) { return s > bs || (s == bs && k < bk); }

// the strongest (s, k) of the workgroup, in every lane
__device__ __forceinline__ void f0_block_argmax(double& s, int& k, double* red, int* redk) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nwaves = blockDim.x >> 6;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const double ts = __shfl_xor(s, o, 64);
        const int tk = __shfl_xor(k, o, 64);
        if (f0_stronger(ts, tk, s, k)) { s = ts; k = tk; }
    }
    __syncthreads();
    if (lane == 0) { red[wave] = s; redk[wave] = k; }
    __syncthreads();
    s = red[0];
    k = redk[0];
    for (int w = 1; w < nwaves; ++w)
        if (f0_stronger(red[w], redk[w], s, k)) { s = red[w]; k = redk[w]; }
}

// G(k fs / L)
__device__ __forceinline__ double f0_lowpass(int k, int L, double fs, double flp) {
    const double f = (double)k * fs / (double)L;
    if (f <= flp) return 1.0;
    if (f < 1.5 * flp) {
        const double c = cospi((f - flp) / flp);
        return c * c;
    }
    return 0.0;
}

// lag k of r as a candidate: its frequency and strength, or false
__device__ __forceinline__ bool f0_candidate(const double* r, int k, double fs, double f0_min, double f0_max, double vt, double oc,
                                             double& F, double& S) {
    const double a = r[k - 1], b = r[k], c = r[k + 1];
    if (!(b > a && b >= c && b > 0.5 * vt)) return false;
    const double d = a - 2.0 * b + c;
    const double delta = d < 0.0 ? 0.5 * (a - c) / d : 0.0;
    const double peak = b - 0.25 * (a - c) * delta;
    const double tau = ((double)k + delta) / fs;
    F = 1.0 / tau;
    if (!(F >= f0_min && F <= f0_max)) return false;
    S = (peak < 1.0 ? peak : 1.0) - oc * log2(f0_min * tau);
    return true;
}

// The scalars of a ptts_f0_candidates launch that every frame shares
struct F0CandArgs {
    int logM, hw, lmin, lmax, ncand;
    double shift, fs, f0_min, f0_max, vt, st, oc;
};

// Frame i of one utterance: wav [N] its samples, the output rows its own, gpeak its peak.  The workgroup's work; dynamic LDS:
// (M + M/4) double2 + (lmax + 2) doubles + 4 doubles + 4 ints.  The host has checked 1 <= lmin <= lmax and 2 hw + 1 + lmax + 1 <= L.
__device__ __forceinline__ void f0_candidates_frame(const float* __restrict__ wav, const long long N, const double* __restrict__ rw,
                                                    float* __restrict__ freq, float* __restrict__ strength, int* __restrict__ nout,
                                                    int* __restrict__ lag, float* __restrict__ rout, const int i, const double gpeak,
                                                    const F0CandArgs& A) {
    extern __shared__ double2 lds[];
    const int logM = A.logM, hw = A.hw, lmin = A.lmin, lmax = A.lmax, ncand = A.ncand;
    const double shift = A.shift, fs = A.fs, f0_min = A.f0_min, f0_max = A.f0_max, vt = A.vt, st = A.st, oc = A.oc;
    const int M = 1 << logM, L = M << 1, Mq = M >> 2, W = 2 * hw + 1;
    double2* a = lds;
    double2* wq = lds + M;
    double* cs = reinterpret_cast<double*>(lds + M + Mq);       // [lmax + 2]: the strength of a lag that is a candidate, else -inf
    double* red = cs + (lmax + 2);
    int* redk = reinterpret_cast<int*>(red + 4);
    const int tid = threadIdx.x, nthr = blockDim.x;

    fill_twiddles(wq, M);
    // position p of the buffer holds sample s0 + p; [j0, j1) are the positions of the window that lie inside the waveform
    const long long s0 = (long long)rnd((double)i * shift * fs) - hw;
    long long j0 = s0 < 0 ? -s0 : 0, j1 = N - s0;
    j0 = j0 > W ? W : j0;
    j1 = j1 > W ? W : j1;
    j1 = j1 < j0 ? j0 : j1;
    double sum = 0.0;
    for (int n = tid; n < M; n += nthr) {
        double v[2];
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            const int p = 2 * n + q;
            v[q] = 0.0;
            if (p >= j0 && p < j1) {
                v[q] = (double)wav[s0 + p];
                sum += v[q];
            }
        }
        a[n] = make_double2(v[0], v[1]);
    }
    sum = block_sum(sum, red);
    const double mean = j1 > j0 ? sum / (double)(j1 - j0) : 0.0;
    double pk = 0.0;
    for (int n = tid; n < M; n += nthr) {
        const double2 z = a[n];
        double v[2] = {z.x, z.y};
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            const int p = 2 * n + q;
            if (p >= j0 && p < j1) {
                const double x = v[q] - mean;
                pk = fabs(x) > pk ? fabs(x) : pk;
                v[q] = x * (0.5 - 0.5 * cospi(2.0 * (double)(p + 1) / (double)(W + 1)));
            }
        }
        a[n] = make_double2(v[0], v[1]);
    }
    pk = f0_block_max(pk, red);
    fft_forward(a, wq, logM);
    unpack_real(a, logM);

    // P is real and even: the packed spectrum of rho = irfft(P), in the same pass
    const double flp = 2.5 * f0_max;
    for (int k = tid; k <= (M >> 1); k += nthr) {
        if (k == 0) {
            const double2 z = a[0];
            const double p0 = f0_lowpass(0, L, fs, flp) * (z.x * z.x), pm = f0_lowpass(M, L, fs, flp) * (z.y * z.y);
            a[0] = make_double2(0.5 * (p0 + pm), 0.5 * (p0 - pm));
        } else {
            const int km = M - k, rk = bitrev(k, logM), rm = bitrev(km, logM);
            const double2 xk = a[rk], xm = a[rm];
            const double pk2 = f0_lowpass(k, L, fs, flp) * (xk.x * xk.x + xk.y * xk.y);
            const double pm2 = f0_lowpass(km, L, fs, flp) * (xm.x * xm.x + xm.y * xm.y);
            double2 zk, zm;
            pack_pair(make_double2(pk2, 0.0), make_double2(pm2, 0.0), pair_twiddle(k, L), zk, zm);
            a[rk] = zk;
            if (k != (M >> 1)) a[rm] = zm;
        }
    }
    fft_inverse(a, wq, logM);

    // the doubles of the buffer are M rho[k] in natural order; r replaces them in place
    double* r = reinterpret_cast<double*>(a);
    const double rho0 = r[0];
    __syncthreads();
    for (int k = tid; k <= lmax + 1; k += nthr) {
        const double v = rho0 > 0.0 ? (r[k] / rho0) / rw[k] : 0.0;
        r[k] = v;
        if (rout) rout[(size_t)i * (lmax + 2) + k] = (float)v;
    }
    __syncthreads();
    for (int k = tid; k <= lmax + 1; k += nthr) {
        double F, S, s = -INFINITY;
        if (k >= lmin && k <= lmax && f0_candidate(r, k, fs, f0_min, f0_max, vt, oc, F, S)) s = S;
        cs[k] = s;
    }
    __syncthreads();

    float* frow = freq + (size_t)i * ncand;
    float* srow = strength + (size_t)i * ncand;
    int* lrow = lag + (size_t)i * ncand;
    int count = 0;
    for (int slot = 1; slot < ncand; ++slot) {
        double best = -INFINITY;
        int bk = INT_MAX;
        for (int k = lmin + tid; k <= lmax; k += nthr)          // ascending: of equal strengths a lane keeps the smaller lag
            if (cs[k] > best) { best = cs[k]; bk = k; }
        f0_block_argmax(best, bk, red, redk);
        if (bk == INT_MAX) break;                               // the same in every lane
        if (tid == 0) {
            double F = 0.0, S = 0.0;
            f0_candidate(r, bk, fs, f0_min, f0_max, vt, oc, F, S);
            frow[slot] = (float)F;
            srow[slot] = (float)S;
            lrow[slot] = bk;
            cs[bk] = -INFINITY;
        }
        ++count;
        __syncthreads();
    }
    if (tid == 0) {
        double quiet = 2.0;
        if (gpeak > 0.0) {
            quiet = 2.0 - (pk / gpeak) / (st / (1.0 + vt));
            quiet = quiet > 0.0 ? quiet : 0.0;
        }
        frow[0] = 0.f;
        srow[0] = (float)(vt + quiet);
        lrow[0] = 0;
        for (int slot = count + 1; slot < ncand; ++slot) {
            frow[slot] = 0.f;
            srow[slot] = 0.f;
            lrow[slot] = 0;
        }
        nout[i] = count;
    }
}

// One workgroup per frame.
__global__ __launch_bounds__(F0_THREADS) void f0_candidates_kernel(const float* __restrict__ wav, const long long N,
                                                                   const double* __restrict__ rw, float* __restrict__ freq,
                                                                   float* __restrict__ strength, int* __restrict__ nout,
                                                                   int* __restrict__ lag, float* __restrict__ rout, const double gpeak,
                                                                   const F0CandArgs A) {
    f0_candidates_frame(wav, N, rw, freq, strength, nout, lag, rout, blockIdx.x, gpeak, A);
}

// One workgroup per frame of the packed batch: the frame's utterance, then f0_candidates_frame on that utterance's samples and rows
// with its own peak from gpeak [B].
__global__ __launch_bounds__(F0_THREADS) void f0_candidates_batch_kernel(const float* __restrict__ wav, const long long* __restrict__ wav_off,
                                                                         const long long wav_total, const long long* __restrict__ frame_off,
                                                                         const int B, const int T, const double* __restrict__ rw,
                                                                         float* __restrict__ freq, float* __restrict__ strength,
                                                                         int* __restrict__ nout, int* __restrict__ lag,
                                                                         float* __restrict__ rout, const double* __restrict__ gpeak,
                                                                         const F0CandArgs A) {
    const PackedFrame f = packed_frame(wav_off, wav_total, frame_off, B, T, blockIdx.x);
    if (!f.ok) return;
    const double gp = gpeak[f.b];
    f0_candidates_frame(wav + f.woff, f.N, rw, freq + (size_t)f.foff * A.ncand, strength + (size_t)f.foff * A.ncand, nout + f.foff,
                        lag + (size_t)f.foff * A.ncand, rout ? rout + (size_t)f.foff * (A.lmax + 2) : nullptr, f.i,
                        gp >= 0.0 && gp < INFINITY ? gp : 0.0, A);
}

// v of another lane of the row of 16 by a DPP move (no LDS crossbar): CTRL 0xB1 = lane ^ 1, 0x4E = lane ^ 2, 0x141 = the mirror lane of
// the half row (7 - lane), 0x140 = the mirror lane of the row (15 - lane)
template <int CTRL> __device__ __forceinline__ int f0_dpp(int v) { return __builtin_amdgcn_update_dpp(0, v, CTRL, 0xF, 0xF, true); }
template <int CTRL> __device__ __forceinline__ double f0_dpp(double v) {
    return __hiloint2double(f0_dpp<CTRL>(__double2hiint(v)), f0_dpp<CTRL>(__double2loint(v)));
}

// one butterfly step of the (smallest cost, then smallest slot) reduction
template <int CTRL> __device__ __forceinline__ void f0_min_step(double& v, int& arg) {
    const double tv = f0_dpp<CTRL>(v);
    const int ta = f0_dpp<CTRL>(arg);
    if (tv < v || (tv == v && ta < arg)) { v = tv; arg = ta; }
}

// One wave64, no barrier inside the frame loop.  group = the power of two at or above ncand, rows = 64 / group.  Lane l stands at
// (g, p) = (l / group, l % group).  Loads: a chunk of `rows` frames at a time, lane (g, p) holds slot p of the chunk's frame g; the
// next chunk loads while this one is walked, and log2 F is taken once per chunk.  Transitions: in pass t lane (g, p) evaluates the
// step from slot p of the frame before to slot j = t rows + g; the minimum over p is a butterfly of DPP moves inside the group (pairs,
// quads, then the mirror lane of the half row and of the row: once the quads agree, the mirror lane holds the other quad's value),
// the new cost_i[p] comes back to the lanes of column p by one shuffle.  dynamic LDS: T * words unsigned, the back-pointers of frame i
// at [i * words, (i + 1) * words), four bits a slot; the way back leaves the chosen slot of frame i in the first of them.
__device__ __forceinline__ void f0_viterbi_wave(const float* __restrict__ freq, const float* __restrict__ strength,
                                                const int* __restrict__ nv, float* __restrict__ f0, int* __restrict__ path,
                                                const int T, const int nc, const int log_group, const int words,
                                                const double corr, const double ojc, const double vuc) {
    extern __shared__ unsigned bpw[];
    unsigned char* bpb = reinterpret_cast<unsigned char*>(bpw);
    const int lane = threadIdx.x, group = 1 << log_group, log_rows = 6 - log_group, rows = 1 << log_rows;
    const int p = lane & (group - 1), g = lane >> log_group, passes = (nc + rows - 1) >> log_rows;       // at most 4
    const int tp = p >> log_rows, sl = (p & (rows - 1)) << log_group;   // cost_i[p] is made in pass tp by the lanes from sl on

    float fc = 0.f, sc = 0.f, fn = 0.f, sn = 0.f;               // this chunk's and the next one's slot p of frame g
    int ncur = 0, nnext = 0;
    if (g < T) {
        ncur = nv[g];
        if (p < nc) { fc = freq[(size_t)g * nc + p]; sc = strength[(size_t)g * nc + p]; }
    }
    ncur = ncur < 0 ? 0 : (ncur > nc - 1 ? nc - 1 : ncur);
    double lfc = p >= 1 && p <= ncur && fc > 0.f ? log2((double)fc) : 0.0;

    int nprev = __shfl(ncur, 0, 64);
    const double s0 = (double)__shfl(sc, p, 64);
    double costp = p <= nprev ? -s0 : INFINITY;                 // cost_{i-1}[p]
    double lfp = __shfl(lfc, p, 64);                            // log2 F of slot p of frame i - 1
    for (int base = 0; base < T; base += rows) {
        if (base + rows + g < T) {
            const size_t fr = (size_t)(base + rows + g);
            nnext = nv[fr];
            if (p < nc) { fn = freq[fr * nc + p]; sn = strength[fr * nc + p]; }
        }
        for (int f = base == 0 ? 1 : 0; f < rows && base + f < T; ++f) {
            const int i = base + f, src = f << log_group;
            const int ni = __shfl(ncur, src, 64);
            const double lfp_next = __shfl(lfc, src + p, 64);
            double cnew[4] = {INFINITY, INFINITY, INFINITY, INFINITY};
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                if (t < passes) {
                    const int j = (t << log_rows) + g, jj = j < nc ? j : 0;
                    const double lfj = __shfl(lfc, src + jj, 64), sj = (double)__shfl(sc, src + jj, 64);
                    double v = INFINITY;
                    int arg = p;
                    if (j <= ni && p <= nprev) {
                        const double trans = (p == 0 && j == 0) ? 0.0 : ((p == 0 || j == 0) ? vuc : ojc * fabs(lfp - lfj));
                        v = costp + corr * trans;
                    }
                    f0_min_step<0xB1>(v, arg);
                    if (log_group >= 2) f0_min_step<0x4E>(v, arg);
                    if (log_group >= 3) f0_min_step<0x141>(v, arg);
                    if (log_group >= 4) f0_min_step<0x140>(v, arg);
                    cnew[t] = j <= ni ? v - sj : INFINITY;
                    // slots j and j + 1 share a byte: the even one's lane writes both nibbles
                    const unsigned nib = j <= ni ? (unsigned)arg & 15u : 0u;
                    const unsigned odd = __shfl_xor(nib, group, 64);
                    if (p == 0 && !(j & 1) && j < nc) bpb[(size_t)i * words * 4 + (j >> 1)] = (unsigned char)(nib | (odd << 4));
                }
            }
            double cp = INFINITY;
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                if (t < passes) {
                    const double x = __shfl(cnew[t], sl, 64);
                    if (t == tp) cp = x;
                }
            }
            costp = cp;
            lfp = lfp_next;
            nprev = ni;
        }
        fc = fn; sc = sn;
        ncur = nnext < 0 ? 0 : (nnext > nc - 1 ? nc - 1 : nnext);
        lfc = p >= 1 && p <= ncur && fc > 0.f ? log2((double)fc) : 0.0;
    }
    // the cheapest slot of the last frame, ties to the smaller slot: lane p < nc holds cost_{T-1}[p]
    double v = lane < nc ? costp : INFINITY;
    int arg = lane;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const double tv = __shfl_xor(v, o, 64);
        const int ta = __shfl_xor(arg, o, 64);
        if (tv < v || (tv == v && ta < arg)) { v = tv; arg = ta; }
    }
    __syncthreads();
    if (lane == 0) {
        int j = arg < nc ? arg : 0;
        for (int i = T - 1; i >= 1; --i) {
            const unsigned w = bpw[(size_t)i * words + (j >> 3)];
            bpw[(size_t)i * words] = (unsigned)j;
            j = (int)((w >> (4 * (j & 7))) & 15u);
            j = j < nc ? j : 0;
        }
        bpw[0] = (unsigned)j;
    }
    __syncthreads();
    for (int i = lane; i < T; i += 64) {
        const int j = (int)bpw[(size_t)i * words];
        f0[i] = j == 0 ? 0.f : freq[(size_t)i * nc + j];
        if (path) path[i] = j;
    }
}

__global__ __launch_bounds__(64) void f0_viterbi_kernel(const float* __restrict__ freq, const float* __restrict__ strength,
                                                        const int* __restrict__ nv, float* __restrict__ f0, int* __restrict__ path,
                                                        const int T, const int nc, const int log_group, const int words,
                                                        const double corr, const double ojc, const double vuc) {
    f0_viterbi_wave(freq, strength, nv, f0, path, T, nc, log_group, words, corr, ojc, vuc);
}

// One wave per utterance of the packed batch, its back-pointers in its own workgroup's LDS (max_frames * words unsigned, the
// longest utterance's).  An utterance whose rows do not lie inside the packed total, or longer than max_frames, is skipped.
__global__ __launch_bounds__(64) void f0_viterbi_batch_kernel(const float* __restrict__ freq, const float* __restrict__ strength,
                                                              const int* __restrict__ nv, float* __restrict__ f0, int* __restrict__ path,
                                                              const long long* __restrict__ frame_off, const int T,
                                                              const int max_frames, const int nc, const int log_group, const int words,
                                                              const double corr, const double ojc, const double vuc) {
    const long long fo = frame_off[blockIdx.x], fe = frame_off[blockIdx.x + 1];
    if (fo < 0 || fe <= fo || fe > (long long)T || fe - fo > (long long)max_frames) return;
    f0_viterbi_wave(freq + (size_t)fo * nc, strength + (size_t)fo * nc, nv + fo, f0 + fo, path ? path + fo : nullptr, (int)(fe - fo), nc,
                    log_group, words, corr, ojc, vuc);
}

constexpr int F0_REFINE_MAX_WINDOW = 16384;             // samples of the window at f0_min
constexpr int F0_REFINE_H1 = 2, F0_REFINE_H2 = 6;       // harmonics of the two passes

// block_sum of frame.h over NV values at once, in the same fixed order: the wave's butterfly, then the waves in turn.  red: [nwaves * NV]
template <int NV> __device__ __forceinline__ void f0_block_sum_n(double* v, double* red) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nwaves = blockDim.x >> 6;
#pragma unroll
    for (int q = 0; q < NV; ++q) v[q] = wave_sum(v[q]);
    __syncthreads();
    if (lane == 0) {
#pragma unroll
        for (int q = 0; q < NV; ++q) red[wave * NV + q] = v[q];
    }
    __syncthreads();
#pragma unroll
    for (int q = 0; q < NV; ++q) {
        double tot = red[q];
        for (int w = 1; w < nwaves; ++w) tot += red[w * NV + q];
        v[q] = tot;
    }
}

// One pass of the refinement from g over the harmonics h = 1 .. H (those below fs/2): the new value num / den, or false where
// den > 0 is false.  x = wav + c is the window's centre; every lane returns the same.  One sincospi a sample gives the phasor of the
// fundamental, its powers those of the harmonics; the window comes from one more and the double angle.
template <int H> __device__ __forceinline__ bool f0_refine_pass(const float* __restrict__ x, const int hw, const double fs, double& g,
                                                                double* red) {
    int nh = 0;
    while (nh < H && !((double)(nh + 1) * g >= 0.5 * fs)) ++nh;
    double acc[4 * H];                                          // Re X, Im X, Re Xd, Im Xd of every harmonic
#pragma unroll
    for (int q = 0; q < 4 * H; ++q) acc[q] = 0.0;
    const double span = 2.0 * (double)(hw + 1);
    for (int n = threadIdx.x; n <= 2 * hw; n += blockDim.x) {
        const int j = n - hw;
        double s1, c1, sp, cp;
        sincospi(2.0 * ((double)j / span), &s1, &c1);
        const double s2 = 2.0 * s1 * c1, c2 = 2.0 * c1 * c1 - 1.0;
        const double v = (double)x[j];
        const double a = v * (0.42 + 0.5 * c1 + 0.08 * c2);
        const double b = v * (-(M_PI / (double)(hw + 1)) * (0.5 * s1 + 0.16 * s2));
        sincospi(2.0 * g * (double)j / fs, &sp, &cp);
        double zr = cp, zi = -sp;                               // e^{-2 pi i h g j / fs}
#pragma unroll
        for (int h = 0; h < H; ++h) {
            if (h < nh) {
                acc[4 * h + 0] += a * zr;
                acc[4 * h + 1] += a * zi;
                acc[4 * h + 2] += b * zr;
                acc[4 * h + 3] += b * zi;
                const double t = zr * cp + zi * sp;
                zi = zi * cp - zr * sp;
                zr = t;
            }
        }
    }
    f0_block_sum_n<4 * H>(acc, red);
    double num = 0.0, den = 0.0;
#pragma unroll
    for (int h = 0; h < H; ++h) {
        if (h < nh) {
            const double xr = acc[4 * h], xi = acc[4 * h + 1], dr = acc[4 * h + 2], di = acc[4 * h + 3];
            const double p = xr * xr + xi * xi;
            if (p > 0.0) {
                const double nu = (double)(h + 1) * g, m = sqrt(p);
                num += m * (nu - (fs / (2.0 * M_PI)) * (di * xr - dr * xi) / p);
                den += m * (double)(h + 1);
            }
        }
    }
    if (!(den > 0.0)) return false;
    g = num / den;
    return true;
}

// One workgroup per frame: its lanes share the window's samples, one block sum a pass.  Every exit before or between the block sums
// depends on f0[i], the launch's scalars and the block sums alone, the same in every lane.  static LDS: 4 waves * 24 doubles.
// The host has checked 2 rnd(1.5 fs / f0_min) + 1 <= F0_REFINE_MAX_WINDOW, so hw fits an int.
__device__ __forceinline__ void f0_refine_frame(const float* __restrict__ wav, const long long N, const float* __restrict__ f0,
                                                float* __restrict__ out, int* __restrict__ status, const int i, const double shift,
                                                const double fs, const double f0_min, const double f0_max) {
    __shared__ double red[(F0_THREADS / 64) * 4 * F0_REFINE_H2];
    const float fin = f0[i];
    const double f = (double)fin;
    float res = fin;
    int st = 2;
    if (!(f > 0.0)) {
        res = 0.f;
        st = 0;
    } else if (!(f < f0_min || f > f0_max)) {
        const double hwd = rnd(1.5 * fs / f), cd = rnd((double)i * shift * fs);
        if (!(cd - hwd < 0.0 || cd + hwd >= (double)N)) {       // the whole window lies inside the waveform
            const int hw = (int)hwd;
            const float* x = wav + (long long)cd;
            double g = f;
            st = 3;
            if (f0_refine_pass<F0_REFINE_H1>(x, hw, fs, g, red) && f0_refine_pass<F0_REFINE_H2>(x, hw, fs, g, red) &&
                g - g == 0.0 && fabs(g / f - 1.0) <= 0.2 && g >= f0_min && g <= f0_max) {
                res = (float)g;
                st = 1;
            }
        }
    }
    if (threadIdx.x == 0) {
        out[i] = res;
        if (status) status[i] = st;
    }
}

__global__ __launch_bounds__(F0_THREADS) void f0_refine_kernel(const float* __restrict__ wav, const long long N,
                                                               const float* __restrict__ f0, float* __restrict__ out,
                                                               int* __restrict__ status, const double shift, const double fs,
                                                               const double f0_min, const double f0_max) {
    f0_refine_frame(wav, N, f0, out, status, blockIdx.x, shift, fs, f0_min, f0_max);
}

// One workgroup per frame of the packed batch.
__global__ __launch_bounds__(F0_THREADS) void f0_refine_batch_kernel(const float* __restrict__ wav, const long long* __restrict__ wav_off,
                                                                     const long long wav_total, const long long* __restrict__ frame_off,
                                                                     const int B, const int T, const float* __restrict__ f0,
                                                                     float* __restrict__ out, int* __restrict__ status,
                                                                     const double shift, const double fs, const double f0_min,
                                                                     const double f0_max) {
    const PackedFrame f = packed_frame(wav_off, wav_total, frame_off, B, T, blockIdx.x);
    if (!f.ok) return;
    f0_refine_frame(wav + f.woff, f.N, f0 + f.foff, out + f.foff, status ? status + f.foff : nullptr, f.i, shift, fs, f0_min, f0_max);
}

// The checks of ptts_f0_candidates and its batched form that do not depend on the tensors -> the launch's scalars and LDS bytes
static int f0_candidates_args(const char* what, int ncand, double shift, double fs, int dftlen, double f0_min, double f0_max,
                              double voicing_threshold, double silence_threshold, double octave_cost, F0CandArgs& A, int& lds) {
    PTTS_REQUIRE(ncand >= F0_MIN_NCAND && ncand <= F0_MAX_NCAND, "%s: ncand=%d outside [%d, %d]", what, ncand, F0_MIN_NCAND, F0_MAX_NCAND);
    const int logL = frame_log2(dftlen);
    PTTS_REQUIRE(logL > 0, "%s: dftlen=%d is not a power of two in [%d, %d]", what, dftlen, FRAME_MIN_DFTLEN, FRAME_MAX_DFTLEN);
    PTTS_REQUIRE(fs > 0.0 && fs < 1e9, "%s: fs=%g", what, fs);
    PTTS_REQUIRE(shift > 0.0 && shift < 1e3, "%s: shift=%g", what, shift);
    PTTS_REQUIRE(f0_min > 0.0 && f0_min <= f0_max && f0_max <= 0.5 * fs, "%s: f0_min=%g f0_max=%g (positive, ordered, at most fs/2)", what,
                 f0_min, f0_max);
    PTTS_REQUIRE(voicing_threshold > 0.0 && voicing_threshold < 1e3 && silence_threshold > 0.0 && silence_threshold < 1e3 &&
                 octave_cost >= 0.0 && octave_cost < 1e3, "%s: voicing_threshold=%g silence_threshold=%g octave_cost=%g", what,
                 voicing_threshold, silence_threshold, octave_cost);
    const double hwd = 1.5 * fs / f0_min;
    PTTS_REQUIRE(hwd < (double)dftlen, "%s: the window at f0_min=%g does not fit dftlen=%d", what, f0_min, dftlen);
    const int hw = (int)hwd, lmin = (int)ceil(fs / f0_max), lmax = (int)floor(fs / f0_min);
    PTTS_REQUIRE(2 * hw + 1 + lmax + 1 <= dftlen, "%s: the window at f0_min=%g (%d samples) and its longest lag (%d) do not fit dftlen=%d",
                 what, f0_min, 2 * hw + 1, lmax, dftlen);
    PTTS_REQUIRE(lmin >= 1 && lmin <= lmax, "%s: lags %d .. %d", what, lmin, lmax);
    const int M = dftlen / 2;
    lds = (M + M / 4) * (int)sizeof(double2) + (lmax + 2 + 4) * (int)sizeof(double) + 4 * (int)sizeof(int);
    A = F0CandArgs{logL - 1, hw, lmin, lmax, ncand, shift, fs, f0_min, f0_max, voicing_threshold, silence_threshold, octave_cost};
    return PTTS_OK;
}

static int f0_viterbi_args(const char* what, int ncand, double shift, double octave_jump_cost, double voiced_unvoiced_cost) {
    PTTS_REQUIRE(ncand >= F0_MIN_NCAND && ncand <= F0_MAX_NCAND, "%s: ncand=%d outside [%d, %d]", what, ncand, F0_MIN_NCAND, F0_MAX_NCAND);
    PTTS_REQUIRE(shift > 0.0 && shift < 1e3, "%s: shift=%g", what, shift);
    PTTS_REQUIRE(octave_jump_cost >= 0.0 && octave_jump_cost < 1e3 && voiced_unvoiced_cost >= 0.0 && voiced_unvoiced_cost < 1e3,
                 "%s: octave_jump_cost=%g voiced_unvoiced_cost=%g", what, octave_jump_cost, voiced_unvoiced_cost);
    return PTTS_OK;
}

static int f0_refine_args(const char* what, double shift, double fs, double f0_min, double f0_max) {
    PTTS_REQUIRE(fs > 0.0 && fs < 1e9, "%s: fs=%g", what, fs);
    PTTS_REQUIRE(shift > 0.0 && shift < 1e3, "%s: shift=%g", what, shift);
    PTTS_REQUIRE(f0_min > 0.0 && f0_min <= f0_max && f0_max <= 0.5 * fs, "%s: f0_min=%g f0_max=%g (positive, ordered, at most fs/2)", what,
                 f0_min, f0_max);
    const double W = 2.0 * floor(1.5 * fs / f0_min + 0.5) + 1.0;
    PTTS_REQUIRE(W <= (double)F0_REFINE_MAX_WINDOW, "%s: the window at f0_min=%g (%.0f samples) is longer than %d", what, f0_min, W,
                 F0_REFINE_MAX_WINDOW);
    return PTTS_OK;
}

}  // namespace ptts

using namespace ptts;

extern "C" int ptts_f0_candidates(const float* wav, long long N, const double* rw, size_t rw_bytes, float* freq, float* strength, int* n,
                                  int* lag, float* r, int T, int ncand, double shift, double fs, int dftlen, double f0_min, double f0_max,
                                  double gpeak, double voicing_threshold, double silence_threshold, double octave_cost, void* stream) {
    PTTS_REQUIRE(T >= 0 && N >= 0, "f0_candidates: T=%d N=%lld", T, N);
    F0CandArgs A;
    int lds;
    int rc = f0_candidates_args("f0_candidates", ncand, shift, fs, dftlen, f0_min, f0_max, voicing_threshold, silence_threshold,
                                octave_cost, A, lds);
    if (rc != PTTS_OK) return rc;
    PTTS_REQUIRE(gpeak >= 0.0 && gpeak < INFINITY, "f0_candidates: gpeak=%g", gpeak);
    if (T == 0) return PTTS_OK;
    PTTS_REQUIRE(freq && strength && n && lag && (wav || N == 0), "f0_candidates: null tensor");
    PTTS_REQUIRE(rw && ((size_t)rw & 7) == 0 && rw_bytes >= (size_t)(A.lmax + 2) * sizeof(double),
                 "f0_candidates: the window table needs %zu bytes, got %zu", (size_t)(A.lmax + 2) * sizeof(double), rw_bytes);
    rc = reserve_lds<f0_candidates_kernel>("f0_candidates", lds);
    if (rc != PTTS_OK) return rc;
    hipLaunchKernelGGL(f0_candidates_kernel, dim3(T), dim3(frame_threads(dftlen / 2, F0_THREADS)), (size_t)lds, (hipStream_t)stream, wav, N,
                       rw, freq, strength, n, lag, r, gpeak, A);
    return check_launch("f0_candidates");
}

extern "C" int ptts_f0_candidates_batch(const float* wav, const long long* wav_off, long long wav_total, const long long* frame_off, int B,
                                        int T, const double* rw, size_t rw_bytes, float* freq, float* strength, int* n, int* lag,
                                        float* r, int ncand, double shift, double fs, int dftlen, double f0_min, double f0_max,
                                        const double* gpeak, double voicing_threshold, double silence_threshold, double octave_cost,
                                        void* stream) {
    PTTS_REQUIRE(T >= 0 && wav_total >= 0 && B >= 0 && B <= PACKED_MAX_UTTS, "f0_candidates_batch: T=%d wav_total=%lld B=%d", T, wav_total, B);
    F0CandArgs A;
    int lds;
    int rc = f0_candidates_args("f0_candidates_batch", ncand, shift, fs, dftlen, f0_min, f0_max, voicing_threshold, silence_threshold,
                                octave_cost, A, lds);
    if (rc != PTTS_OK) return rc;
    if (T == 0 || B == 0) return PTTS_OK;
    PTTS_REQUIRE(freq && strength && n && lag && wav_off && frame_off && gpeak && (wav || wav_total == 0), "f0_candidates_batch: null tensor");
    PTTS_REQUIRE(rw && ((size_t)rw & 7) == 0 && rw_bytes >= (size_t)(A.lmax + 2) * sizeof(double),
                 "f0_candidates_batch: the window table needs %zu bytes, got %zu", (size_t)(A.lmax + 2) * sizeof(double), rw_bytes);
    rc = reserve_lds<f0_candidates_batch_kernel>("f0_candidates_batch", lds);
    if (rc != PTTS_OK) return rc;
    hipLaunchKernelGGL(f0_candidates_batch_kernel, dim3(T), dim3(frame_threads(dftlen / 2, F0_THREADS)), (size_t)lds, (hipStream_t)stream,
                       wav, wav_off, wav_total, frame_off, B, T, rw, freq, strength, n, lag, r, gpeak, A);
    return check_launch("f0_candidates_batch");
}

extern "C" int ptts_f0_viterbi_max_frames(int ncand) {
    if (ncand < F0_MIN_NCAND || ncand > F0_MAX_NCAND) return 0;
    return ncand <= 8 ? F0_MAX_FRAMES : F0_MAX_FRAMES / 2;
}

extern "C" int ptts_f0_viterbi(const float* freq, const float* strength, const int* n, float* f0, int* path, int T, int ncand, double shift,
                               double octave_jump_cost, double voiced_unvoiced_cost, void* stream) {
    int rc = f0_viterbi_args("f0_viterbi", ncand, shift, octave_jump_cost, voiced_unvoiced_cost);
    if (rc != PTTS_OK) return rc;
    PTTS_REQUIRE(T >= 0 && T <= ptts_f0_viterbi_max_frames(ncand), "f0_viterbi: T=%d frames, at most %d with ncand=%d", T,
                 ptts_f0_viterbi_max_frames(ncand), ncand);
    if (T == 0) return PTTS_OK;
    PTTS_REQUIRE(freq && strength && n && f0, "f0_viterbi: null tensor");
    int log_group = 1;
    while ((1 << log_group) < ncand) ++log_group;
    const int words = ncand <= 8 ? 1 : 2;
    const int lds = T * words * (int)sizeof(unsigned);
    rc = reserve_lds<f0_viterbi_kernel>("f0_viterbi", lds);
    if (rc != PTTS_OK) return rc;
    hipLaunchKernelGGL(f0_viterbi_kernel, dim3(1), dim3(64), (size_t)lds, (hipStream_t)stream, freq, strength, n, f0, path, T, ncand, log_group,
                       words, 0.01 / shift, octave_jump_cost, voiced_unvoiced_cost);
    return check_launch("f0_viterbi");
}

extern "C" int ptts_f0_viterbi_batch(const float* freq, const float* strength, const int* n, float* f0, int* path,
                                     const long long* frame_off, int B, int T, int max_frames, int ncand, double shift,
                                     double octave_jump_cost, double voiced_unvoiced_cost, void* stream) {
    int rc = f0_viterbi_args("f0_viterbi_batch", ncand, shift, octave_jump_cost, voiced_unvoiced_cost);
    if (rc != PTTS_OK) return rc;
    PTTS_REQUIRE(T >= 0 && B >= 0 && B <= PACKED_MAX_UTTS, "f0_viterbi_batch: T=%d B=%d", T, B);
    PTTS_REQUIRE(max_frames >= 0 && max_frames <= ptts_f0_viterbi_max_frames(ncand),
                 "f0_viterbi_batch: max_frames=%d, an utterance has at most %d with ncand=%d", max_frames,
                 ptts_f0_viterbi_max_frames(ncand), ncand);
    if (T == 0 || B == 0 || max_frames == 0) return PTTS_OK;
    PTTS_REQUIRE(freq && strength && n && f0 && frame_off, "f0_viterbi_batch: null tensor");
    int log_group = 1;
    while ((1 << log_group) < ncand) ++log_group;
    const int words = ncand <= 8 ? 1 : 2;
    const int lds = max_frames * words * (int)sizeof(unsigned);
    rc = reserve_lds<f0_viterbi_batch_kernel>("f0_viterbi_batch", lds);
    if (rc != PTTS_OK) return rc;
    hipLaunchKernelGGL(f0_viterbi_batch_kernel, dim3(B), dim3(64), (size_t)lds, (hipStream_t)stream, freq, strength, n, f0, path, frame_off,
                       T, max_frames, ncand, log_group, words, 0.01 / shift, octave_jump_cost, voiced_unvoiced_cost);
    return check_launch("f0_viterbi_batch");
}

extern "C" int ptts_f0_refine(const float* wav, long long N, const float* f0, float* out, int* status, int T, double shift, double fs,
                              double f0_min, double f0_max, void* stream) {
    PTTS_REQUIRE(T >= 0 && N >= 0, "f0_refine: T=%d N=%lld", T, N);
    const int rc = f0_refine_args("f0_refine", shift, fs, f0_min, f0_max);
    if (rc != PTTS_OK) return rc;
    if (T == 0) return PTTS_OK;
    PTTS_REQUIRE(f0 && out && (wav || N == 0), "f0_refine: null tensor");
    hipLaunchKernelGGL(f0_refine_kernel, dim3(T), dim3(F0_THREADS), 0, (hipStream_t)stream, wav, N, f0, out, status, shift, fs, f0_min,
                       f0_max);
    return check_launch("f0_refine");
}

extern "C" int ptts_f0_refine_batch(const float* wav, const long long* wav_off, long long wav_total, const long long* frame_off, int B,
                                    int T, const float* f0, float* out, int* status, double shift, double fs, double f0_min,
                                    double f0_max, void* stream) {
    PTTS_REQUIRE(T >= 0 && wav_total >= 0 && B >= 0 && B <= PACKED_MAX_UTTS, "f0_refine_batch: T=%d wav_total=%lld B=%d", T, wav_total, B);
    const int rc = f0_refine_args("f0_refine_batch", shift, fs, f0_min, f0_max);
    if (rc != PTTS_OK) return rc;
    if (T == 0 || B == 0) return PTTS_OK;
    PTTS_REQUIRE(f0 && out && wav_off && frame_off && (wav || wav_total == 0), "f0_refine_batch: null tensor");
    hipLaunchKernelGGL(f0_refine_batch_kernel, dim3(T), dim3(F0_THREADS), 0, (hipStream_t)stream, wav, wav_off, wav_total, frame_off, B, T,
                       f0, out, status, shift, fs, f0_min, f0_max);
    return check_launch("f0_refine_batch");
}
