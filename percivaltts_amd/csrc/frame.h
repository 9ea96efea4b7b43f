// What the kernels of the offline vocoder chain share around the in-LDS transforms of realfft.h (pulsesynth.hip, worldsynth.hip,
// analysis.hip, worldanalysis.hip, f0.hip; preproc.hip takes the LDS reservation alone): the dftlen limits, the workgroup's size, the
// LDS reservation, the quarter circle of twiddles, the zero-phase frame, a bin of an unpacked spectrum, the band axis of
// ptts_fwbnd_table, the fixed-order block sum.  Notation as in realfft.h: L = dftlen, M = L/2 complex points, K = M + 1 bins.
#pragma once
#include "common.h"
#include "realfft.h"

namespace ptts {

constexpr int FRAME_MIN_DFTLEN = 256, FRAME_MAX_DFTLEN = 8192;

// log2(dftlen) for a power of two in [FRAME_MIN_DFTLEN, FRAME_MAX_DFTLEN], else -1
inline int frame_log2(int dftlen) {
    for (int l = 8; l <= 13; ++l)
        if (dftlen == (1 << l)) return l;
    return -1;
}

// threads of a workgroup that holds M complex points: a lane for four of them, a wave at least, `cap` at most
inline int frame_threads(int M, int cap) { return M / 4 < 64 ? 64 : (M / 4 > cap ? cap : M / 4); }

// Reserves `lds` bytes of dynamic LDS for Kernel unless a call before has reserved as much: one counter per kernel, per process.
template <auto Kernel>
int reserve_lds(const char* what, int lds) {
    static int reserved = 0;
    if (lds > reserved) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(Kernel), hipFuncAttributeMaxDynamicSharedMemorySize, lds);
        if (e != hipSuccess) { set_error("%s: cannot reserve %d B of LDS: %s", what, lds, hipGetErrorString(e)); return PTTS_ELAUNCH; }
        reserved = lds;
    }
    return PTTS_OK;
}

__device__ __forceinline__ double rnd(double x) { return floor(x + 0.5); }

// The workgroup's sum in a fixed order: the wave's butterfly, then the waves in turn.  red: [waves]
__device__ __forceinline__ double block_sum(double v, double* red) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nwaves = blockDim.x >> 6;
    const double s = wave_sum(v);
    __syncthreads();
    if (lane == 0) red[wave] = s;
    __syncthreads();
    double tot = red[0];
    for (int w = 1; w < nwaves; ++w) tot += red[w];
    return tot;
}

// A batch of utterances packed one after the other (the *_batch forms of the analysis kernels): utterance b has the samples
// wav_off[b] .. wav_off[b+1] of one waveform buffer and the frame rows frame_off[b] .. frame_off[b+1] of every per-frame tensor,
// both offset rows [B+1] int64 in device memory, ascending from 0.
constexpr int PACKED_MAX_UTTS = 65535;

struct PackedFrame {
    int b, i, T;                // the utterance, the frame's index within it, the utterance's frames
    long long N, woff, foff;    // the utterance's samples, its first sample, its first frame
    bool ok;                    // false: the offsets do not lie inside the totals; nothing of the frame is read or written
};

// Global frame g (0 <= g < T_total) of the packing: a binary search for the first utterance with frame_off[b + 1] > g.
__device__ __forceinline__ PackedFrame packed_frame(const long long* __restrict__ wav_off, long long wav_total,
                                                    const long long* __restrict__ frame_off, int B, int T_total, long long g) {
    int lo = 0, hi = B - 1;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (frame_off[mid + 1] > g) hi = mid; else lo = mid + 1;
    }
    PackedFrame f;
    f.b = lo;
    f.foff = frame_off[lo];
    const long long fe = frame_off[lo + 1];
    f.woff = wav_off ? wav_off[lo] : 0;
    const long long we = wav_off ? wav_off[lo + 1] : 0;
    f.N = we - f.woff;
    f.i = (int)(g - f.foff);
    f.T = (int)(fe - f.foff);
    f.ok = f.foff >= 0 && g >= f.foff && g < fe && fe <= (long long)T_total && f.woff >= 0 && we >= f.woff && we <= wav_total;
    return f;
}

// wq[j] = exp(-2 pi i j / M), 0 <= j < M/4.  Not followed by a barrier: the transforms open with one.
__device__ __forceinline__ void fill_twiddles(double2* wq, int M) {
    for (int j = threadIdx.x; j < (M >> 2); j += blockDim.x) {
        double s, c;
        sincospi(2.0 * (double)j / (double)M, &s, &c);
        wq[j] = make_double2(c, -s);
    }
}

// The windowed frame around sample c, packed, in zero-phase placement: position p of the frame holds wav[c + j] window(j) with
// j = p (p <= hw) or j = p - L (p >= L - hw); 2 hw + 1 <= L keeps them apart, samples outside [0, N) are 0.  No barrier behind it.
template <class Window>
__device__ __forceinline__ void frame_fill(double2* a, const float* __restrict__ wav, long long N, long long c, int hw, int M, Window window) {
    const int L = M << 1;
    for (int n = threadIdx.x; n < M; n += blockDim.x) {
        double v[2];
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            const int p = 2 * n + q;
            v[q] = 0.0;
            if (p <= hw || p >= L - hw) {
                const int j = p <= hw ? p : p - L;
                const long long s = c + j;
                if (s >= 0 && s < N) v[q] = (double)wav[s] * window(j);
            }
        }
        a[n] = make_double2(v[0], v[1]);
    }
}

// bin k (0 .. M) of the unpacked spectrum: X_0 and X_M are real and share slot 0
__device__ __forceinline__ double2 spectrum_bin(const double2* a, int k, int logM) {
    const int M = 1 << logM;
    if (k <= 0) return make_double2(a[0].x, 0.0);
    if (k >= M) return make_double2(a[0].y, 0.0);
    return a[bitrev(k, logM)];
}

// the lower band of bin k as the band row of ptts_fwbnd_table has it (clamped, whatever the table holds)
__device__ __forceinline__ int lower_band(const double* __restrict__ tab, int nb, int k) {
    const int b = (int)tab[k];
    return b < 0 ? 0 : (b > nb - 2 ? nb - 2 : b);
}

// bin k on the band axis: its lower band b and the fraction fr with which it reads band b + 1
__device__ __forceinline__ void band_of(const double* __restrict__ tab, int Kp, int nb, int k, int& b, double& fr) {
    b = lower_band(tab, nb, k);
    fr = tab[(size_t)Kp + k];
}

}  // namespace ptts
