// Waveform pre-processing in front of the analysis (the reference's Vocoder.preprocwav, vocoders.py:45-63: pulsemodel's resampler, then
// scipy's filtfilt of a 4th-order Butterworth high-pass).  Both definitions are this build's own, DESIGN.md section 3.  A launch takes a
// packed batch: utterance u is the samples off[u] .. off[u+1] of one fp32 array.
//
// resample         g = gcd(fs_in, fs_out), up = fs_out / g, down = fs_in / g, c = 0.95 min(1, up / down), R = 16 / c, hw = ceil(R);
//                  h[p][j] = c sinc(c tau) I0(9 sqrt(1 - (tau / R)^2)) / I0(9) for |tau| < R, else 0, tau = p / up - j, p = 0 .. up - 1,
//                  j = -hw + 1 .. hw, is the caller's fp64 table [up][2 hw];  M = (N up + down - 1) div down,
//                  y[m] = sum_{j = -hw+1 .. hw} h[p][j] x[q + j], q = (m down) div up, p = (m down) mod up, x = 0 outside [0, N),
//                  summed in increasing j.  One thread per output sample.
// high-pass        K = tan(pi fc / fs); two sections with Q = 1 / (2 cos(pi / 8)), 1 / (2 cos(3 pi / 8)): n = 1 / (1 + K / Q + K^2),
//                  b = (n, -2 n, n), a1 = 2 (K^2 - 1) n, a2 = (1 - K / Q + K^2) n.
//                  e = the signal with P = padlen samples of odd extension at both ends (2 x[0] - x[P - k] in front, 2 x[N-1] - x[N-2-i]
//                  behind), Ne = N + 2 P.  pass(e): section 1, then section 2, each
//                  y[n] = ((b0 x[n] + b1 x[n-1]) + b2 x[n-2]) - a1 y[n-1] - a2 y[n-2]; section 1 starts with x[-1] = x[-2] = e[0], every
//                  other history is 0 (the steady state of a constant input: a section's DC gain is exactly 0).
//                  result = reverse(pass(reverse(pass(e)))) without the P samples at each end.
//
// Data is fp32 in memory, arithmetic fp64, rounded once; no fused contraction.  ptts_highpass_zerophase: one workgroup per utterance
// walks the extended signal in tiles of HP_TILE samples held in LDS as fp64, both sections in place, forward over e and then backward
// over the forward pass's result (fp64, in the caller's workspace); every global access is coalesced.  A section's recursive part is
// a 2-state linear recurrence s' = M s + (v, v).  A lane owns HP_CHUNK consecutive samples (in registers): it runs them from a zero
// state (lane 0: from the state the tile before left) to its end state E, the workgroup scans E_j <- M^(HP_CHUNK 2^d) E_(j - 2^d) + E_j
// over d = 0 .. 7 through LDS (the matrices come from the host, fp64), and the lane runs its chunk again from the end state of the
// lane before it.  No table of homogeneous solutions, no fix-up term.  The scanned state is s = (y[n-1], y[n-1] - y[n-2]), in which
// M = [[1 - c, a2], [-c, a2]] with c = 1 + a1 + a2 = 4 K^2 n: at a low cut-off the poles lie close to 1, the powers of the transition
// matrix of (y[n-1], y[n-2]) grow like [[m + 1, -m], [m, 1 - m]] and cancel 13 bits at m = 8192, those of this one stay near
// [[1, m], [0, 1]] (the blocked form against the sequential loop, fp64, at fc = fs / 4000: 3.0e-9 with the first, 1.8e-11 with this).
// No atomics, no polling, nothing between workgroups; an utterance's result does not depend on what else is in the launch.
#include <cmath>
#include "common.h"
#include "frame.h"      // reserve_lds

namespace ptts {

constexpr int RS_THREADS = 256;
constexpr int RS_MAX_UP = 1024;
constexpr size_t RS_MAX_TABLE_BYTES = (size_t)4 << 20;
constexpr int PREPROC_MAX_UTTS = 65535;
constexpr long long PREPROC_MAX_SAMPLES = 1LL << 40;

constexpr int HP_THREADS = 256;                                 // lanes of the workgroup = chunks of a tile
constexpr int HP_CHUNK = 32;                                    // samples a lane owns
constexpr int HP_TILE = HP_THREADS * HP_CHUNK;
constexpr int HP_ROW = HP_CHUNK + 1;                            // doubles of a lane's row in LDS: stride 66 words, ds_read_b64 of a column is conflict-free
constexpr int HP_LEVELS = 8;                                    // log2(HP_THREADS)
constexpr int HP_MAX_PADLEN = 1 << 20;
constexpr int HP_LDS_BYTES = HP_THREADS * HP_ROW * (int)sizeof(double) + 2 * HP_THREADS * (int)sizeof(double2);

struct HpSection {
    double b0, b1, b2, a1, a2;
    double pw[HP_LEVELS][4];                                    // M^(HP_CHUNK 2^d), row-major, M in the basis (y[n-1], y[n-1] - y[n-2])
};
struct HpCoef { HpSection s[2]; };

// blockIdx.y = utterance, grid-stride over its output samples.  An utterance whose offsets do not lie inside the arrays as the host
// measured them is skipped; no more than y_off[u+1] - y_off[u] samples of it are written.
__global__ __launch_bounds__(RS_THREADS) void resample_kernel(const float* __restrict__ x, const long long* __restrict__ x_off,
                                                              const long long total_in, float* __restrict__ y,
                                                              const long long* __restrict__ y_off, const long long total_out,
                                                              const double* __restrict__ h, const int up, const int down, const int hw) {
    const int u = blockIdx.y;
    const long long a0 = x_off[u], a1 = x_off[u + 1], c0 = y_off[u], c1 = y_off[u + 1];
    if (a0 < 0 || a1 < a0 || a1 > total_in || c0 < 0 || c1 < c0 || c1 > total_out) return;
    const long long N = a1 - a0;
    long long M = (N * up + down - 1) / down;
    M = M > c1 - c0 ? c1 - c0 : M;
    const float* xu = x + a0;
    float* yu = y + c0;
    const int taps = 2 * hw;
    for (long long m = (long long)blockIdx.x * RS_THREADS + threadIdx.x; m < M; m += (long long)gridDim.x * RS_THREADS) {
        const long long md = m * down, q = md / up;
        const double* hp = h + (size_t)(md - q * up) * taps;
        const long long first = q - hw + 1;
        double acc = 0.0;
        for (int t = 0; t < taps; ++t) {
            const long long i = first + t;
            const double xv = i >= 0 && i < N ? (double)xu[i] : 0.0;
            acc += hp[t] * xv;
        }
        yu[m] = (float)acc;
    }
}

// One section over the tile in `buf`, in place.  (cx1, cx2) = the two inputs in front of the tile, cy = (y[-1], y[-1] - y[-2]); they come
// back as the next tile's.  sc: 2 HP_THREADS double2.  Ends with a barrier.
__device__ __forceinline__ void hp_section(double* buf, double2* sc, const HpSection& c, double& cx1, double& cx2, double2& cy) {
    const int tid = threadIdx.x;
    double* row = buf + tid * HP_ROW;
    double xm1 = cx1, xm2 = cx2;
    if (tid) { xm1 = row[-2]; xm2 = row[-3]; }                  // the last two samples of the row before (row[-1] is its padding)
    cx1 = buf[(HP_THREADS - 1) * HP_ROW + HP_CHUNK - 1];
    cx2 = buf[(HP_THREADS - 1) * HP_ROW + HP_CHUNK - 2];
    double v[HP_CHUNK];
#pragma unroll
    for (int i = 0; i < HP_CHUNK; ++i) {
        const double x = row[i];
        v[i] = (c.b0 * x + c.b1 * xm1) + c.b2 * xm2;
        xm2 = xm1;
        xm1 = x;
    }
    double y1 = tid ? 0.0 : cy.x, y2 = tid ? 0.0 : cy.x - cy.y;
#pragma unroll
    for (int i = 0; i < HP_CHUNK; ++i) {
        const double y = (v[i] - c.a1 * y1) - c.a2 * y2;
        y2 = y1;
        y1 = y;
    }
    // inclusive scan of the end states: sc[cur] holds level d's input, level d writes the other half
    double2 E = make_double2(y1, y1 - y2);
    int cur = 0;
    sc[tid] = E;
    __syncthreads();
#pragma unroll
    for (int d = 0; d < HP_LEVELS; ++d) {
        const int o = 1 << d;
        if (tid >= o) {
            const double2 p = sc[cur * HP_THREADS + tid - o];
            E.x = (c.pw[d][0] * p.x + c.pw[d][1] * p.y) + E.x;
            E.y = (c.pw[d][2] * p.x + c.pw[d][3] * p.y) + E.y;
        }
        cur ^= 1;
        sc[cur * HP_THREADS + tid] = E;
        __syncthreads();
    }
    const double2 start = tid ? sc[cur * HP_THREADS + tid - 1] : cy;
    cy = sc[cur * HP_THREADS + HP_THREADS - 1];
    y1 = start.x;
    y2 = start.x - start.y;
#pragma unroll
    for (int i = 0; i < HP_CHUNK; ++i) {
        const double y = (v[i] - c.a1 * y1) - c.a2 * y2;
        row[i] = y;
        y2 = y1;
        y1 = y;
    }
    __syncthreads();
}

__device__ __forceinline__ int hp_slot(int t) { return (t / HP_CHUNK) * HP_ROW + (t % HP_CHUNK); }

// One workgroup per utterance.  dynamic LDS: HP_LDS_BYTES.  ws holds Ne doubles of utterance u from off[u] + 2 P u on.  An utterance
// whose offsets do not lie inside [0, total] or that has no more than P samples is skipped: nothing of it is read or written.
__global__ __launch_bounds__(HP_THREADS) void highpass_kernel(const float* x, float* y, const long long* __restrict__ off,
                                                              double* __restrict__ ws, const long long total, const int P,
                                                              const HpCoef c) {
    extern __shared__ double2 hp_lds[];
    double* buf = reinterpret_cast<double*>(hp_lds);
    double2* sc = reinterpret_cast<double2*>(buf + HP_THREADS * HP_ROW);
    const int u = blockIdx.x, tid = threadIdx.x;
    const long long o0 = off[u], o1 = off[u + 1], N = o1 - o0;
    if (o0 < 0 || o1 > total || N <= P) return;                 // the same in every lane
    const long long Ne = N + 2LL * P;
    const float* xu = x + o0;
    float* yu = y + o0;
    double* w = ws + (o0 + 2LL * P * u);
    const double x0 = (double)xu[0], xl = (double)xu[N - 1];

    double cx1 = 2.0 * x0 - (double)xu[P], cx2 = cx1, dx1 = 0.0, dx2 = 0.0;        // e[0] twice in front of section 1
    double2 cy1 = make_double2(0.0, 0.0), cy2 = cy1;
    for (long long base = 0; base < Ne; base += HP_TILE) {
        for (int t = tid; t < HP_TILE; t += HP_THREADS) {
            const long long k = base + t;
            double e = 0.0;
            if (k < P) e = 2.0 * x0 - (double)xu[P - k];
            else if (k < P + N) e = (double)xu[k - P];
            else if (k < Ne) e = 2.0 * xl - (double)xu[N - 2 - (k - P - N)];
            buf[hp_slot(t)] = e;
        }
        __syncthreads();
        hp_section(buf, sc, c.s[0], cx1, cx2, cy1);
        hp_section(buf, sc, c.s[1], dx1, dx2, cy2);
        for (int t = tid; t < HP_TILE; t += HP_THREADS)
            if (base + t < Ne) w[base + t] = buf[hp_slot(t)];
        __syncthreads();
    }
    // backward: position r of the reversed signal is w[Ne - 1 - r]
    cx1 = cx2 = w[Ne - 1];
    dx1 = dx2 = 0.0;
    cy1 = cy2 = make_double2(0.0, 0.0);
    for (long long base = 0; base < Ne; base += HP_TILE) {
        for (int t = tid; t < HP_TILE; t += HP_THREADS) {
            const long long r = base + t;
            buf[hp_slot(t)] = r < Ne ? w[Ne - 1 - r] : 0.0;
        }
        __syncthreads();
        hp_section(buf, sc, c.s[0], cx1, cx2, cy1);
        hp_section(buf, sc, c.s[1], dx1, dx2, cy2);
        for (int t = tid; t < HP_TILE; t += HP_THREADS) {
            const long long k = Ne - 1 - (base + t);
            if (k >= P && k < P + N) yu[k - P] = (float)buf[hp_slot(t)];
        }
        __syncthreads();
    }
}

static void hp_matmul(const double* a, const double* b, double* out) {
    const double r[4] = {a[0] * b[0] + a[1] * b[2], a[0] * b[1] + a[1] * b[3], a[2] * b[0] + a[3] * b[2], a[2] * b[1] + a[3] * b[3]};
    for (int i = 0; i < 4; ++i) out[i] = r[i];
}

// the two sections at K = tan(pi fc / fs), with the powers of their transition matrices
static void hp_coefficients(double fs, double fc, HpCoef& c) {
    const double pi = 3.14159265358979323846;
    const double K = tan(pi * fc / fs);
    const double Q[2] = {1.0 / (2.0 * cos(pi / 8.0)), 1.0 / (2.0 * cos(3.0 * pi / 8.0))};
    for (int s = 0; s < 2; ++s) {
        HpSection& k = c.s[s];
        const double n = 1.0 / (1.0 + K / Q[s] + K * K);
        k.b0 = n;
        k.b1 = -2.0 * n;
        k.b2 = n;
        k.a1 = 2.0 * (K * K - 1.0) * n;
        k.a2 = (1.0 - K / Q[s] + K * K) * n;
        const double c1 = 4.0 * K * K * n;                                      // 1 + a1 + a2, without the cancellation
        double m[4] = {1.0 - c1, k.a2, -c1, k.a2};
        for (int q = 1; q < HP_CHUNK; q <<= 1) hp_matmul(m, m, m);              // M^HP_CHUNK by squaring
        for (int d = 0; d < HP_LEVELS; ++d) {
            for (int i = 0; i < 4; ++i) k.pw[d][i] = m[i];
            hp_matmul(m, m, m);
        }
    }
}

static bool hp_parameters_ok(double fs, double fc) { return fs > 0.0 && fs < 1e9 && fc >= fs / 4000.0 && fc < 0.5 * fs; }

}  // namespace ptts

using namespace ptts;

extern "C" int ptts_resample(const float* x, const long long* x_off, long long total_in, float* y, const long long* y_off,
                             long long total_out, long long max_out, int n_utts, const double* h, size_t h_bytes, int up, int down, int hw,
                             void* stream) {
    PTTS_REQUIRE(n_utts >= 0 && n_utts <= PREPROC_MAX_UTTS, "resample: n_utts=%d outside [0, %d]", n_utts, PREPROC_MAX_UTTS);
    PTTS_REQUIRE(up >= 1 && up <= RS_MAX_UP && down >= 1 && down <= (1 << 30), "resample: up=%d (1 .. %d) down=%d", up, RS_MAX_UP, down);
    PTTS_REQUIRE(hw >= 1 && (size_t)up * 2 * (size_t)hw * sizeof(double) <= RS_MAX_TABLE_BYTES,
                 "resample: a table of %d x %d taps is larger than %zu bytes", up, 2 * hw, RS_MAX_TABLE_BYTES);
    PTTS_REQUIRE(total_in >= 0 && total_in < PREPROC_MAX_SAMPLES && total_out >= 0 && total_out < PREPROC_MAX_SAMPLES && max_out >= 0 &&
                 max_out <= total_out, "resample: total_in=%lld total_out=%lld max_out=%lld", total_in, total_out, max_out);
    if (n_utts == 0 || max_out == 0) return PTTS_OK;
    PTTS_REQUIRE(x_off && y_off && y && (x || total_in == 0), "resample: null tensor");
    PTTS_REQUIRE(h && ((size_t)h & 7) == 0 && h_bytes >= (size_t)up * 2 * (size_t)hw * sizeof(double),
                 "resample: the table needs %zu bytes, got %zu", (size_t)up * 2 * (size_t)hw * sizeof(double), h_bytes);
    const long long blocks = (max_out + RS_THREADS - 1) / RS_THREADS;
    hipLaunchKernelGGL(resample_kernel, dim3((unsigned)(blocks > 65535 ? 65535 : blocks), (unsigned)n_utts), dim3(RS_THREADS), 0,
                       (hipStream_t)stream, x, x_off, total_in, y, y_off, total_out, h, up, down, hw);
    return check_launch("resample");
}

extern "C" int ptts_highpass_tile(int* chunk, int* tile) {
    PTTS_REQUIRE(chunk && tile, "highpass_tile: null pointer");
    *chunk = HP_CHUNK;
    *tile = HP_TILE;
    return PTTS_OK;
}

extern "C" int ptts_highpass_sections(double fs, double fc, double* sos) {
    PTTS_REQUIRE(hp_parameters_ok(fs, fc), "highpass_sections: fs=%g fc=%g (fs / 4000 <= fc < fs / 2)", fs, fc);
    PTTS_REQUIRE(sos, "highpass_sections: null pointer");
    HpCoef c;
    hp_coefficients(fs, fc, c);
    for (int s = 0; s < 2; ++s) {
        const double row[6] = {c.s[s].b0, c.s[s].b1, c.s[s].b2, 1.0, c.s[s].a1, c.s[s].a2};
        for (int i = 0; i < 6; ++i) sos[6 * s + i] = row[i];
    }
    return PTTS_OK;
}

extern "C" size_t ptts_highpass_workspace_bytes(long long total, int n_utts, int padlen) {
    if (total < 0 || total >= PREPROC_MAX_SAMPLES || n_utts < 0 || n_utts > PREPROC_MAX_UTTS || padlen < 0 || padlen > HP_MAX_PADLEN) return 0;
    return (size_t)(total + 2LL * padlen * n_utts) * sizeof(double);
}

extern "C" int ptts_highpass_zerophase(const float* x, float* y, const long long* off, long long total, int n_utts, double fs, double fc,
                                       int padlen, void* workspace, size_t workspace_bytes, void* stream) {
    PTTS_REQUIRE(n_utts >= 0 && n_utts <= PREPROC_MAX_UTTS, "highpass_zerophase: n_utts=%d outside [0, %d]", n_utts, PREPROC_MAX_UTTS);
    PTTS_REQUIRE(total >= 0 && total < PREPROC_MAX_SAMPLES, "highpass_zerophase: total=%lld", total);
    PTTS_REQUIRE(padlen >= 0 && padlen <= HP_MAX_PADLEN, "highpass_zerophase: padlen=%d outside [0, %d]", padlen, HP_MAX_PADLEN);
    PTTS_REQUIRE(hp_parameters_ok(fs, fc), "highpass_zerophase: fs=%g fc=%g (fs / 4000 <= fc < fs / 2)", fs, fc);
    if (n_utts == 0 || total == 0) return PTTS_OK;
    PTTS_REQUIRE(x && y && off, "highpass_zerophase: null tensor");
    const size_t need = ptts_highpass_workspace_bytes(total, n_utts, padlen);
    PTTS_REQUIRE(workspace && ((size_t)workspace & 7) == 0 && workspace_bytes >= need,
                 "highpass_zerophase: the workspace needs %zu bytes, got %zu", need, workspace_bytes);
    HpCoef c;
    hp_coefficients(fs, fc, c);
    const int rc = reserve_lds<highpass_kernel>("highpass_zerophase", HP_LDS_BYTES);
    if (rc != PTTS_OK) return rc;
    hipLaunchKernelGGL(highpass_kernel, dim3(n_utts), dim3(HP_THREADS), (size_t)HP_LDS_BYTES, (hipStream_t)stream, x, y, off,
                       static_cast<double*>(workspace), total, padlen, c);
    return check_launch("highpass_zerophase");
}
