// The in-LDS radix-2 real transform that the kernels of the offline vocoder chain share (frame.h holds what they share around it).
//
// A real transform of length L is a complex transform of length M = L/2 on the packed sequence z[n] = x[2n] + i x[2n+1] plus one
// pass over the bin pairs (k, M - k); the complex transform is radix-2 in LDS, decimation in frequency forwards (natural in,
// bit-reversed out) and decimation in time backwards (bit-reversed in, natural out), so a spectrum lives at bit-reversed addresses
// and no reordering pass exists.  X_0 and X_M of a real sequence are real and share slot 0.  The twiddles are a quarter circle
// wq[j] = exp(-2 pi i j / M), 0 <= j < M/4, that the caller fills.  fp64 throughout; every routine is called by the whole workgroup.
#pragma once
#include "common.h"

namespace ptts {

__device__ __forceinline__ double2 cadd(double2 a, double2 b) { return make_double2(a.x + b.x, a.y + b.y); }
__device__ __forceinline__ double2 csub(double2 a, double2 b) { return make_double2(a.x - b.x, a.y - b.y); }
__device__ __forceinline__ double2 cmul(double2 a, double2 b) { return make_double2(a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x); }
__device__ __forceinline__ double2 cconj(double2 a) { return make_double2(a.x, -a.y); }

// exp(-2 pi i t / M), 0 <= t < M/2, from the quarter circle wq[0 .. M/4)
__device__ __forceinline__ double2 twiddle(const double2* wq, int t, int Mq) {
    if (t < Mq) return wq[t];
    const double2 w = wq[t - Mq];
    return make_double2(w.y, -w.x);
}

// exp(-2 pi i k / L)
__device__ __forceinline__ double2 pair_twiddle(int k, int L) {
    double s, c;
    sincospi(2.0 * (double)k / (double)L, &s, &c);
    return make_double2(c, -s);
}

__device__ __forceinline__ int bitrev(int k, int logM) { return (int)(__brev((unsigned)k) >> (32 - logM)); }

// a[0..M) natural -> its transform at bit-reversed addresses
__device__ void fft_forward(double2* a, const double2* wq, int logM) {
    const int M = 1 << logM, Mq = M >> 2;
    __syncthreads();
    for (int s = logM - 1; s >= 0; --s) {
        const int half = 1 << s;
        for (int b = threadIdx.x; b < (M >> 1); b += blockDim.x) {
            const int j = b & (half - 1), i = ((b >> s) << (s + 1)) | j;
            const double2 u = a[i], v = a[i + half];
            a[i] = cadd(u, v);
            a[i + half] = cmul(csub(u, v), twiddle(wq, j << (logM - 1 - s), Mq));
        }
        __syncthreads();
    }
}

// fft_forward on two buffers at once: the same butterflies, half the barriers
__device__ void fft_forward2(double2* a, double2* b, const double2* wq, int logM) {
    const int M = 1 << logM, Mq = M >> 2;
    __syncthreads();
    for (int s = logM - 1; s >= 0; --s) {
        const int half = 1 << s;
        for (int t = threadIdx.x; t < (M >> 1); t += blockDim.x) {
            const int j = t & (half - 1), i = ((t >> s) << (s + 1)) | j;
            const double2 w = twiddle(wq, j << (logM - 1 - s), Mq);
            const double2 ua = a[i], va = a[i + half], ub = b[i], vb = b[i + half];
            a[i] = cadd(ua, va);
            a[i + half] = cmul(csub(ua, va), w);
            b[i] = cadd(ub, vb);
            b[i + half] = cmul(csub(ub, vb), w);
        }
        __syncthreads();
    }
}

// a spectrum at bit-reversed addresses -> M times its inverse transform, natural order
__device__ void fft_inverse(double2* a, const double2* wq, int logM) {
    const int M = 1 << logM, Mq = M >> 2;
    __syncthreads();
    for (int s = 0; s < logM; ++s) {
        const int half = 1 << s;
        for (int b = threadIdx.x; b < (M >> 1); b += blockDim.x) {
            const int j = b & (half - 1), i = ((b >> s) << (s + 1)) | j;
            const double2 u = a[i], v = cmul(a[i + half], cconj(twiddle(wq, j << (logM - 1 - s), Mq)));
            a[i] = cadd(u, v);
            a[i + half] = csub(u, v);
        }
        __syncthreads();
    }
}

// Bins k and M - k (0 < k <= M/2) of the real sequence whose packed transform gave zk = Z[k], zm = Z[M-k].
__device__ __forceinline__ void unpack_pair(double2 zk, double2 zm, double2 t, double2& xk, double2& xm) {
    const double2 e = make_double2(0.5 * (zk.x + zm.x), 0.5 * (zk.y - zm.y));
    const double2 p = cmul(t, make_double2(0.5 * (zk.x - zm.x), 0.5 * (zk.y + zm.y)));
    xk = make_double2(e.x + p.y, e.y - p.x);
    xm = make_double2(e.x - p.y, -e.y - p.x);
}

// The inverse: Z[k] and Z[M-k] of the packed sequence from bins xk = X[k], xm = X[M-k]; t = exp(-2 pi i k / L).
__device__ __forceinline__ void pack_pair(double2 xk, double2 xm, double2 t, double2& zk, double2& zm) {
    const double2 a = make_double2(0.5 * (xk.x + xm.x), 0.5 * (xk.y - xm.y));
    const double2 q = cmul(cconj(t), make_double2(0.5 * (xk.x - xm.x), 0.5 * (xk.y + xm.y)));
    zk = make_double2(a.x - q.y, a.y + q.x);
    zm = make_double2(a.x + q.y, -a.y + q.x);
}

// In place: the packed transform Z (bit-reversed addresses) -> bins X_k of the real sequence, X_0 and X_M in slot 0.
__device__ void unpack_real(double2* a, int logM) {
    const int M = 1 << logM, L = M << 1;
    for (int k = threadIdx.x; k <= (M >> 1); k += blockDim.x) {
        if (k == 0) {
            const double2 z = a[0];
            a[0] = make_double2(z.x + z.y, z.x - z.y);
        } else if (k == (M >> 1)) {
            const int r = bitrev(k, logM);
            a[r] = cconj(a[r]);
        } else {
            const int rk = bitrev(k, logM), rm = bitrev(M - k, logM);
            double2 xk, xm;
            unpack_pair(a[rk], a[rm], pair_twiddle(k, L), xk, xm);
            a[rk] = xk;
            a[rm] = xm;
        }
    }
    __syncthreads();
}

}  // namespace ptts
