// The two steps of a waveform analysis that the per-utterance path takes on the host, for a batch of utterances packed one after the
// other (frame.h: wav_off / frame_off [B+1] int64), one workgroup per utterance each; with them nothing of an analysis needs the
// host between the waveforms going up and the parameters coming back (the batched forms of the frame kernels are in f0.hip,
// analysis.hip and worldanalysis.hip).
//
// ptts_wave_peak   gpeak_b = max |x - mean(x)| over the utterance's samples, fp64 from the fp32 samples (what ops.f0_estimate
//                  measures with torch in front of ptts_f0_candidates).  A lane sums its samples tid, tid + 1024, .. in ascending
//                  order, block_sum of frame.h adds the lanes in its fixed order: the same input gives the same bytes.  N_b = 0: 0.
// ptts_f0_track    ops.f0_track (ops_offline.py): f0 [T_b] in Hz, <= 0 unvoiced -> the continuous track.
//   interpolation  numpy.interp(i, idx[voiced], f0[voiced]) restated as in pulsetable.hip: with p the last voiced frame <= i and q the
//                  first one > i: f0[first voiced] without p, f0[last voiced] without q, f0[p] for i == p, otherwise
//                  slope * (i - p) + f0[p], slope = (f0[q] - f0[p]) / (q - p), in fp64
//   finish         clip to [f0_min, f0_max], round to fp32; a value that rounded below f0_min goes one ulp up, one that rounded
//                  above f0_max one ulp down; the first Tout_b <= T_b frames are written (the caller's cropping rule), vuv = f0 > 0
//   p and q        a lane owns a run of consecutive frames; the last and first voiced frame of every run, an inclusive block scan
//                  of them over the lanes (max from the left, min from the right), then one walk along the run
//
// What the host path refuses with a ValueError is a status bit in info [B] (PTTS_ANALYSIS_*), OR-ed in by one lane of the
// utterance's workgroup (plain loads and stores: launches on one stream are ordered and an utterance has one workgroup); such an
// utterance gets no rows.  Contraction is off: a fused multiply-add in slope * (i - p) + f0[p] would break the equality with numpy.
#include <climits>
#include <cmath>
#include "common.h"
#include "frame.h"

#pragma clang fp contract(off)

namespace ptts {

constexpr int AB_THREADS = 256;
constexpr int AB_PEAK_THREADS = 1024;           // the peak walks the utterance's samples twice: every lane the workgroup can have

// One workgroup per utterance.
__global__ __launch_bounds__(AB_PEAK_THREADS) void wave_peak_kernel(const float* __restrict__ wav, const long long* __restrict__ wav_off,
                                                               const long long wav_total, double* __restrict__ gpeak,
                                                               int* __restrict__ info) {
    __shared__ double red[AB_PEAK_THREADS / 64];
    const int b = blockIdx.x, tid = threadIdx.x;
    const long long w0 = wav_off[b], w1 = wav_off[b + 1];
    if (w0 < 0 || w1 < w0 || w1 > wav_total) return;    // offsets outside the total: nothing is read or written
    const long long N = w1 - w0;
    const float* x = wav + w0;
    double sum = 0.0, bad = 0.0;
    for (long long j = tid; j < N; j += AB_PEAK_THREADS) {
        const double v = (double)x[j];
        if (!(v - v == 0.0)) bad = 1.0;
        sum += v;
    }
    sum = block_sum(sum, red);
    bad = block_sum(bad, red);
    const double mean = N > 0 ? sum / (double)N : 0.0;
    double pk = 0.0;
    for (long long j = tid; j < N; j += AB_PEAK_THREADS) {
        const double d = fabs((double)x[j] - mean);
        pk = d > pk ? d : pk;
    }
    // the largest of the lanes: the wave's butterfly, then the waves in turn (a maximum does not depend on the order)
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const double t = __shfl_xor(pk, o, 64);
        pk = t > pk ? t : pk;
    }
    __syncthreads();
    if ((tid & 63) == 0) red[tid >> 6] = pk;
    __syncthreads();
    if (tid == 0) {
        for (int w = 1; w < AB_PEAK_THREADS / 64; ++w) pk = red[w] > pk ? red[w] : pk;
        if (bad > 0.0) {
            info[b] = info[b] | PTTS_ANALYSIS_BAD_WAV;
            pk = 0.0;
        }
        gpeak[b] = pk;
    }
}

// One workgroup per utterance.  F: float or double, the type of the track in memory.
template <class F>
__global__ __launch_bounds__(AB_THREADS) void f0_track_kernel(const F* __restrict__ f0, const long long* __restrict__ in_off,
                                                              const long long in_total, const long long* __restrict__ out_off,
                                                              const long long out_total, float* __restrict__ track,
                                                              float* __restrict__ vuv, int* __restrict__ info, const double f0_min,
                                                              const double f0_max) {
    __shared__ int s_last[AB_THREADS], s_first[AB_THREADS];     // the last voiced frame at or before a lane's run / the first at or behind it
    __shared__ int s_bad;
    const int b = blockIdx.x, tid = threadIdx.x;
    const long long i0 = in_off[b], i1 = in_off[b + 1], o0 = out_off[b], o1 = out_off[b + 1];
    if (i0 < 0 || i1 < i0 || i1 > in_total || i1 - i0 > (long long)INT_MAX || o0 < 0 || o1 < o0 || o1 > out_total || o1 - o0 > i1 - i0) return;
    const int T = (int)(i1 - i0), Tout = (int)(o1 - o0);
    const F* x = f0 + i0;
    const int run = (T - 1) / AB_THREADS + 1;                   // T >= 1 below; at T = 0 every run is empty
    const long long lo = (long long)tid * run, hi = lo + run;
    const int r0 = lo < T ? (int)lo : T, r1 = hi < T ? (int)hi : T;
    if (tid == 0) s_bad = 0;
    __syncthreads();
    int last = -1, first = INT_MAX;
    bool bad = false;
    for (int i = r0; i < r1; ++i) {
        const double v = (double)x[i];
        bad = bad || !(v - v == 0.0);
        if (v > 0.0) {
            last = i;
            first = first == INT_MAX ? i : first;
        }
    }
    if (bad) s_bad = 1;
    s_last[tid] = last;
    s_first[tid] = first;
    __syncthreads();
    // inclusive scans over the lanes (Hillis-Steele): s_last the maximum from the left, s_first the minimum from the right
    for (int d = 1; d < AB_THREADS; d <<= 1) {
        const int l = tid >= d ? s_last[tid - d] : -1, f = tid + d < AB_THREADS ? s_first[tid + d] : INT_MAX;
        __syncthreads();
        if (l > s_last[tid]) s_last[tid] = l;
        if (f < s_first[tid]) s_first[tid] = f;
        __syncthreads();
    }
    const int first_voiced = s_first[0], last_voiced = s_last[AB_THREADS - 1];
    if (s_bad || T < 1 || last_voiced < 0) {
        if (tid == 0) info[b] = info[b] | (s_bad || T < 1 ? PTTS_ANALYSIS_BAD_F0 : PTTS_ANALYSIS_NO_VOICED);
        return;
    }
    int p = tid > 0 ? s_last[tid - 1] : -1;                     // the last voiced frame before the run
    const int behind = tid + 1 < AB_THREADS ? s_first[tid + 1] : INT_MAX;      // the first voiced frame behind the run
    int q = -1;                                                 // the first voiced frame > i; -1: to be looked for
    for (int i = r0; i < r1 && i < Tout; ++i) {
        const double v = (double)x[i];
        if (v > 0.0) { p = i; q = -1; }
        if (q < 0) {
            q = behind;
            for (int j = i + 1; j < r1; ++j)
                if ((double)x[j] > 0.0) { q = j; break; }
        }
        double y;
        if (p < 0) y = (double)x[first_voiced];
        else if (q == INT_MAX) y = (double)x[last_voiced];
        else if (p == i) y = v;
        else {
            const double fp = (double)x[p];
            const double slope = ((double)x[q] - fp) / ((double)q - (double)p);
            y = slope * ((double)i - (double)p) + fp;
        }
        y = y < f0_min ? f0_min : (y > f0_max ? f0_max : y);
        float o = (float)y;
        if ((double)o < f0_min) o = nextafterf(o, INFINITY);
        else if ((double)o > f0_max) o = nextafterf(o, -INFINITY);
        track[o0 + i] = o;
        vuv[o0 + i] = v > 0.0 ? 1.f : 0.f;
    }
}

}  // namespace ptts

using namespace ptts;

extern "C" int ptts_wave_peak(const float* wav, const long long* wav_off, long long wav_total, int B, double* gpeak, int* info,
                              void* stream) {
    PTTS_REQUIRE(B >= 0 && B <= PACKED_MAX_UTTS && wav_total >= 0, "wave_peak: B=%d wav_total=%lld", B, wav_total);
    if (B == 0) return PTTS_OK;
    PTTS_REQUIRE(wav_off && gpeak && info && (wav || wav_total == 0), "wave_peak: null tensor");
    hipLaunchKernelGGL(wave_peak_kernel, dim3(B), dim3(AB_PEAK_THREADS), 0, (hipStream_t)stream, wav, wav_off, wav_total, gpeak, info);
    return check_launch("wave_peak");
}

extern "C" int ptts_f0_track(const void* f0, int f0_is_double, const long long* in_off, long long in_total, const long long* out_off,
                             long long out_total, int B, float* track, float* vuv, int* info, double f0_min, double f0_max,
                             void* stream) {
    PTTS_REQUIRE(B >= 0 && B <= PACKED_MAX_UTTS && in_total >= 0 && out_total >= 0 && out_total <= in_total,
                 "f0_track: B=%d in_total=%lld out_total=%lld", B, in_total, out_total);
    PTTS_REQUIRE(f0_min > 0.0 && f0_min <= f0_max && f0_max < 1e9, "f0_track: f0_min=%g f0_max=%g (positive, ordered)", f0_min, f0_max);
    if (B == 0) return PTTS_OK;
    PTTS_REQUIRE(in_off && out_off && info && (f0 || in_total == 0) && ((track && vuv) || out_total == 0), "f0_track: null tensor");
    if (f0_is_double)
        hipLaunchKernelGGL(f0_track_kernel<double>, dim3(B), dim3(AB_THREADS), 0, (hipStream_t)stream, (const double*)f0, in_off, in_total,
                           out_off, out_total, track, vuv, info, f0_min, f0_max);
    else
        hipLaunchKernelGGL(f0_track_kernel<float>, dim3(B), dim3(AB_THREADS), 0, (hipStream_t)stream, (const float*)f0, in_off, in_total,
                           out_off, out_total, track, vuv, info, f0_min, f0_max);
    return check_launch("f0_track");
}
