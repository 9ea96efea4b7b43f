// The pulse table of the two waveform synthesisers (pulsesynth.hip, worldsynth.hip) built on the device, for a batch of utterances
// in one launch per kernel, and the overlap-add over such a batch.  The definition is ops._pulse_table's (ops_offline.py, DESIGN.md
// section 3); the kernels repeat its fp64 operations one by one, so a table is the host's bit for bit.
// Notation: B utterances packed one after the other, utterance b with T_b frames from frame frame_off[b] on and wavlen_b samples
// from sample samp_off[b] on; offs [2][B+1] int64 holds the two offset rows.  The WORLD form is chosen by voiced != NULL.
//
// rate(x)          max(interp(x), 50); in the WORLD form 500 where frame min(max(rnd(x / shift), 0), T-1) is unvoiced;
//                  rnd(x) = floor(x + 0.5)
// interp(x)        numpy.interp(x, shift * arange(T), f0), restated: xp_j = shift * j, j the largest index with xp_j <= x;
//                  f0[T-1] for x >= xp_{T-1}, f0[j] for x == xp_j, otherwise slope * (x - xp_j) + f0[j] with
//                  slope = (f0[j+1] - f0[j]) / (xp_{j+1} - xp_j)
// walk             t_0 = 0, t_{n+1} = t_n + 1.0 / rate(t_n) while t_n < wavlen / fs: a dependent chain, lane 0 of one wave per
//                  utterance walks it while the track lies in LDS (tracks of more than PT_LDS_FRAMES frames are read in place)
// rows             one lane per pulse: start, winlen, lb, rb, fr (i0, i1, v) | delay, f0 (w), written twice: relative to the own
//                  utterance, and offset for the packed buffers the segment kernels read (frames by frame_off[b], samples by
//                  samp_off[b]; winlen = 0 for the pulse of an utterance without samples, which those kernels then skip)
// overlap-add      pulse_overlap_add_kernel's sum for the sample's own utterance: the same pulses in the same order
//
// Every integer decision is taken in fp64 and contraction is off: a fused multiply-add in slope * (x - xp_j) + f0[j] would break
// the equality.  What the host refuses with a ValueError is a status bit here; the lane stops and nothing is written out of bounds.
#include "common.h"

#pragma clang fp contract(off)

namespace ptts {

constexpr int PT_LDS_FRAMES = 8192;             // a longer track is read from global memory
constexpr int PT_MAX_UTTS = 65535;
constexpr double PT_F0_FLOOR = 50.0, PT_UNVOICED_RATE = 500.0;
constexpr int PT_INFO = 4;                      // info [B][4] int32: pulse count, largest winlen, walk status, rows status

struct PtTrack {
    const float* f0;                            // the utterance's [T] values
    const unsigned char* voiced;                // NULL: the PML form
    int T;
    double shift;
};

__device__ __forceinline__ double pt_rnd(double x) { return floor(x + 0.5); }

__device__ __forceinline__ int pt_frame(const PtTrack& tr, double x) {
    const double q = pt_rnd(x / tr.shift), last = (double)(tr.T - 1);
    return q >= last ? tr.T - 1 : (q > 0.0 ? (int)q : 0);
}

__device__ __forceinline__ double pt_interp(const PtTrack& tr, double x) {
    const int last = tr.T - 1;
    const double q = x / tr.shift;
    int j = q >= (double)last ? last : (q > 0.0 ? (int)q : 0);
    while (j > 0 && tr.shift * (double)j > x) --j;
    while (j < last && tr.shift * (double)(j + 1) <= x) ++j;
    if (j >= last) return (double)tr.f0[last];
    const double xj = tr.shift * (double)j, fj = (double)tr.f0[j];
    if (x == xj) return fj;
    const double slope = ((double)tr.f0[j + 1] - fj) / (tr.shift * (double)(j + 1) - xj);
    return slope * (x - xj) + fj;
}

// rate(x); interpolated: the value came from the track (and is held against f0_cap), not the unvoiced constant
__device__ __forceinline__ double pt_rate(const PtTrack& tr, double x, bool& interpolated) {
    interpolated = tr.voiced == nullptr || tr.voiced[pt_frame(tr, x)] != 0;
    if (!interpolated) return PT_UNVOICED_RATE;
    const double r = pt_interp(tr, x);
    return PT_F0_FLOOR > r ? PT_F0_FLOOR : r;
}

// 2 int(max(0.050 fs, 4 fs / rate) / 2) + 1, as a double (rate >= 50 and fs < 1e9: below 2^31)
__device__ __forceinline__ double pt_winlen(double fs, double rate) {
    const double a = 0.050 * fs, b = 4.0 * fs / rate;
    return 2.0 * floor((b > a ? b : a) / 2.0) + 1.0;
}

// the lead of a pulse over its window
__device__ __forceinline__ double pt_pos(bool world, double fs, double winlen) {
    return floor((world ? 2.0 * floor(0.050 * fs / 2.0) + 1.0 : winlen) / 4.0);
}

// One wave per utterance.
__global__ __launch_bounds__(64) void pulse_walk_kernel(const float* __restrict__ f0, const unsigned char* __restrict__ voiced,
                                                        const long long* __restrict__ offs, const int B, const double shift,
                                                        const double fs, const int dftlen, const int cap, const double f0_cap,
                                                        double* __restrict__ t, int* __restrict__ info) {
    __shared__ float sf0[PT_LDS_FRAMES];
    __shared__ unsigned char sv[PT_LDS_FRAMES];
    __shared__ int sbad;
    const int b = blockIdx.x, lane = threadIdx.x;
    const long long foff = offs[b];
    const int T = (int)(offs[b + 1] - foff);
    const long long wavlen = offs[(B + 1) + b + 1] - offs[(B + 1) + b];
    const bool staged = T <= PT_LDS_FRAMES;
    if (lane == 0) sbad = 0;
    __syncthreads();
    bool bad = false;
    for (int i = lane; i < T; i += 64) {
        const float v = f0[foff + i];
        bad = bad || !(v > 0.f) || !isfinite(v);
        if (staged) {
            sf0[i] = v;
            if (voiced) sv[i] = voiced[foff + i];
        }
    }
    if (bad) sbad = 1;
    __syncthreads();
    if (lane != 0) return;

    int* out = info + (size_t)b * PT_INFO;
    double* tb = t + (size_t)b * cap;
    unsigned status = 0;
    int n = 0;
    double maxwin = 0.0;
    if (sbad || T < 1) {
        status = PTTS_PULSE_BAD_F0;
    } else {
        PtTrack tr;
        tr.f0 = staged ? sf0 : f0 + foff;
        tr.voiced = voiced ? (staged ? sv : voiced + foff) : nullptr;
        tr.T = T;
        tr.shift = shift;
        const double end = (double)wavlen / fs;
        double x = 0.0;
        for (;;) {
            if (n >= cap) { status = PTTS_PULSE_TOO_MANY; break; }
            tb[n++] = x;
            bool interpolated;
            const double r = pt_rate(tr, x, interpolated);
            if (interpolated && r > f0_cap) { status = PTTS_PULSE_RATE; break; }
            const double w = pt_winlen(fs, r);
            maxwin = w > maxwin ? w : maxwin;
            if (w > (double)dftlen) { status = PTTS_PULSE_WINDOW; break; }
            if (!(x < end)) break;
            x = x + 1.0 / r;
        }
    }
    out[0] = n;
    out[1] = (int)maxwin;
    out[2] = (int)status;
    out[3] = 0;
}

// One lane per pulse slot: grid (ceil(cap / 256), B).
__global__ __launch_bounds__(256) void pulse_rows_kernel(const float* __restrict__ f0, const unsigned char* __restrict__ voiced,
                                                         const long long* __restrict__ offs, const int B, const double shift,
                                                         const double fs, const int dftlen, const int cap,
                                                         const double* __restrict__ t, int* __restrict__ info,
                                                         int* __restrict__ pulse_off, int* __restrict__ itab_rel,
                                                         int* __restrict__ itab_off, double* __restrict__ dtab) {
    __shared__ int s_before, s_total;
    const int b = blockIdx.y, tid = threadIdx.x;
    if (tid == 0) { s_before = 0; s_total = 0; }
    __syncthreads();
    int before = 0, total = 0;
    for (int i = tid; i < B; i += 256) {
        const int c = info[(size_t)i * PT_INFO];
        total += c;
        if (i < b) before += c;
    }
    if (before) atomicAdd(&s_before, before);
    if (total) atomicAdd(&s_total, total);
    __syncthreads();
    const int p0 = s_before, P = s_total;
    if (blockIdx.x == 0 && tid == 0) {
        pulse_off[b] = p0;
        if (b == B - 1) pulse_off[B] = P;
    }
    const int count = info[(size_t)b * PT_INFO], n = blockIdx.x * 256 + tid;
    if (info[(size_t)b * PT_INFO + 2] != 0 || n >= count) return;       // a refused utterance gets no rows

    const long long foff = offs[b], soff = offs[(B + 1) + b];
    const bool world = voiced != nullptr;
    PtTrack tr;
    tr.f0 = f0 + foff;
    tr.voiced = world ? voiced + foff : nullptr;
    tr.T = (int)(offs[b + 1] - foff);
    tr.shift = shift;
    const double wavlen = (double)(offs[(B + 1) + b + 1] - soff);
    const double* tb = t + (size_t)b * cap;
    const double tn = tb[n];
    bool interpolated;
    const double f0n = pt_rate(tr, tn, interpolated);
    const double winlen = pt_winlen(fs, f0n), pos = pt_pos(world, fs, winlen);
    const double c = pt_rnd(fs * tn), start = c - pos;
    double lb, rb;
    unsigned status = 0;
    if (n > 0) {
        const double tp = tb[n - 1];
        lb = pt_rnd(fs * (tp + tn) / 2.0);
        const double startp = pt_rnd(fs * tp) - pt_pos(world, fs, pt_winlen(fs, pt_rate(tr, tp, interpolated)));
        if (start < startp) status |= PTTS_PULSE_DESCENDING;
    } else {
        lb = pt_rnd(fs * (tn - 0.5 / f0n));
    }
    rb = n < count - 1 ? pt_rnd(fs * (tn + tb[n + 1]) / 2.0) : pt_rnd(fs * (tn + 0.5 / f0n));
    lb = lb < 0.0 ? 0.0 : (lb > wavlen ? wavlen : lb);
    rb = rb < 0.0 ? 0.0 : (rb > wavlen ? wavlen : rb);
    if (rb < lb || (rb > lb && (lb < start || rb - start > (double)dftlen))) status |= PTTS_PULSE_SEGMENT;
    if (!(fabs(start) < 1073741824.0)) status |= PTTS_PULSE_START_RANGE;
    if (status) {
        atomicOr(info + (size_t)b * PT_INFO + 3, (int)status);
        if (status & PTTS_PULSE_START_RANGE) return;                   // nothing an int32 row could hold
    }

    const int fr = pt_frame(tr, tn), col = p0 + n, ifoff = (int)foff, isoff = (int)soff;
    const int istart = (int)start, iwin = (int)winlen, ilb = (int)lb, irb = (int)rb;
    itab_rel[col] = istart;                     itab_off[col] = istart + isoff;
    itab_rel[(size_t)P + col] = iwin;           itab_off[(size_t)P + col] = wavlen > 0.0 ? iwin : 0;
    itab_rel[(size_t)2 * P + col] = ilb;        itab_off[(size_t)2 * P + col] = ilb + isoff;
    itab_rel[(size_t)3 * P + col] = irb;        itab_off[(size_t)3 * P + col] = irb + isoff;
    itab_rel[(size_t)4 * P + col] = fr;         itab_off[(size_t)4 * P + col] = fr + ifoff;
    dtab[col] = pos + (fs * tn - c);
    dtab[(size_t)P + col] = f0n;
    if (world) {
        const double q = tn / shift, last = (double)(tr.T - 1);
        const int i0 = q >= last ? tr.T - 1 : (int)q, i1 = i0 + 1 < tr.T ? i0 + 1 : tr.T - 1, v = tr.voiced[fr] != 0;
        itab_rel[(size_t)5 * P + col] = i0;     itab_off[(size_t)5 * P + col] = i0 + ifoff;
        itab_rel[(size_t)6 * P + col] = i1;     itab_off[(size_t)6 * P + col] = i1 + ifoff;
        itab_rel[(size_t)7 * P + col] = v;      itab_off[(size_t)7 * P + col] = v;
        dtab[(size_t)2 * P + col] = i0 < tr.T - 1 ? q - (double)i0 : 0.0;
    }
}

// One lane per sample of the packed waveform: its utterance by a binary search over samp_off, then pulse_overlap_add_kernel's two
// searches and its sum within that utterance's pulses.
__global__ __launch_bounds__(256) void pulse_overlap_add_batch_kernel(const float* __restrict__ seg, const int* __restrict__ itab,
                                                                      const int* __restrict__ pulse_off,
                                                                      const long long* __restrict__ samp_off, const int B, const int P,
                                                                      const int W, float* __restrict__ wav, const long long wavlen) {
    const long long j = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= wavlen) return;
    int lo = 0, hi = B - 1;                             // the first utterance with samp_off[b + 1] > j
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (samp_off[mid + 1] > j) hi = mid; else lo = mid + 1;
    }
    const int* start = itab;
    const int* winlen = itab + P;
    int p0 = pulse_off[lo], p1 = pulse_off[lo + 1];
    p0 = p0 < 0 ? 0 : p0;
    p1 = p1 > P ? P : p1;
    lo = p0, hi = p1;                                   // first pulse with start > j - W
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if ((long long)start[mid] > j - W) hi = mid; else lo = mid + 1;
    }
    const int first = lo;
    hi = p1;                                            // first pulse with start > j
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

static int walk_args(const char* name, int B, double shift, double fs, int dftlen, int cap) {
    PTTS_REQUIRE(B >= 0 && B <= PT_MAX_UTTS, "%s: B=%d outside [0, %d]", name, B, PT_MAX_UTTS);
    PTTS_REQUIRE(shift > 0.0 && shift < 1e3, "%s: shift=%g", name, shift);
    PTTS_REQUIRE(fs > 0.0 && fs < 1e9, "%s: fs=%g", name, fs);
    PTTS_REQUIRE(dftlen >= 256 && dftlen <= 8192 && !(dftlen & (dftlen - 1)), "%s: dftlen=%d is not a power of two in [256, 8192]",
                 name, dftlen);
    PTTS_REQUIRE(cap >= 1 && (long long)cap * (B > 0 ? B : 1) < (1LL << 31) / 8, "%s: cap=%d for B=%d", name, cap, B);
    return PTTS_OK;
}

}  // namespace ptts

using namespace ptts;

extern "C" int ptts_pulse_walk(const float* f0, const unsigned char* voiced, const long long* offs, int B, double shift, double fs,
                               int dftlen, int cap, double f0_cap, double* t, int* info, void* stream) {
    const int rc = walk_args("pulse_walk", B, shift, fs, dftlen, cap);
    if (rc != PTTS_OK) return rc;
    PTTS_REQUIRE(f0_cap > 0.0 && f0_cap < 1e9, "pulse_walk: f0_cap=%g", f0_cap);
    if (B == 0) return PTTS_OK;
    PTTS_REQUIRE(f0 && offs && t && info, "pulse_walk: null tensor");
    hipLaunchKernelGGL(pulse_walk_kernel, dim3(B), dim3(64), 0, (hipStream_t)stream, f0, voiced, offs, B, shift, fs, dftlen, cap,
                       f0_cap, t, info);
    return check_launch("pulse_walk");
}

extern "C" int ptts_pulse_rows(const float* f0, const unsigned char* voiced, const long long* offs, int B, double shift, double fs,
                               int dftlen, int cap, const double* t, int* info, int* pulse_off, int* itab_rel, int* itab_off,
                               double* dtab, void* stream) {
    const int rc = walk_args("pulse_rows", B, shift, fs, dftlen, cap);
    if (rc != PTTS_OK) return rc;
    if (B == 0) return PTTS_OK;
    PTTS_REQUIRE(f0 && offs && t && info && pulse_off && itab_rel && itab_off && dtab, "pulse_rows: null tensor");
    hipLaunchKernelGGL(pulse_rows_kernel, dim3((cap + 255) / 256, B), dim3(256), 0, (hipStream_t)stream, f0, voiced, offs, B, shift, fs,
                       dftlen, cap, t, info, pulse_off, itab_rel, itab_off, dtab);
    return check_launch("pulse_rows");
}

extern "C" int ptts_pulse_overlap_add_batch(const float* seg, const int* itab, const int* pulse_off, const long long* samp_off, int B,
                                            int P, int W, float* wav, long long wavlen, void* stream) {
    PTTS_REQUIRE(B >= 0 && B <= PT_MAX_UTTS && P >= 0 && W >= 1 && wavlen >= 0, "pulse_overlap_add_batch: B=%d P=%d W=%d wavlen=%lld", B,
                 P, W, wavlen);
    if (wavlen == 0) return PTTS_OK;
    PTTS_REQUIRE(B >= 1 && wav && pulse_off && samp_off && (P == 0 || (seg && itab)), "pulse_overlap_add_batch: null tensor");
    PTTS_REQUIRE((wavlen + 255) / 256 < (1LL << 31), "pulse_overlap_add_batch: wavlen=%lld", wavlen);
    hipLaunchKernelGGL(pulse_overlap_add_batch_kernel, dim3((unsigned)((wavlen + 255) / 256)), dim3(256), 0, (hipStream_t)stream, seg,
                       itab, pulse_off, samp_off, B, P, W, wav, wavlen);
    return check_launch("pulse_overlap_add_batch");
}
