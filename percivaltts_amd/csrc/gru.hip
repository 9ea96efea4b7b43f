// Keras GRU recurrence (reset_after = False; gates z, r, h; activation tanh, recurrent_activation hard_sigmoid, the TF 1.x
// default that pGRU does not override), both directions of a Bidirectional wrapper advanced by the same launches.
// Reference: networktts.py:101-114 (pGRU / pBGRU).
//
// The input projection x.W+b and every weight gradient are big products done outside (ops.gru); what is left here is the
// T-sequential part.  The candidate's recurrent product (r * h_{t-1}).U_h needs the complete r, so a step is TWO launches:
//   forward  A: z, r = hs(xp_zr + h_{t-1}.U_zr), rh = r * h_{t-1}         tiles of 16 samples x 16 of the 2H z|r columns
//            B: hh = tanh(xp_h + rh.U_h), h_t = z h_{t-1} + (1 - z) hh     tiles of 16 samples x 16 units
//   backward A': da_h = dh (1 - z)(1 - hh^2), d(rh) = da_h.U_h^T; dz, dr, da_zr and the elementwise part of dh_{t-1}
//            B': dh_{t-1} += da_zr.U_zr^T  (K = 2H)
// Every product is exact fp32 on v_mfma_f32_16x16x4_f32 against the recurrent kernel packed once per call (the layout of
// lstm_pack_u_fwd_kernel: each lane's B operands of all k-steps contiguous), K split over the 4 waves of a workgroup and the
// partial tiles summed through LDS in a fixed order.  Any H: K is padded to a multiple of 16 with zero weights, and the A
// operands, columns and samples beyond H / 2H / B are predicated off.
// ptts_gru_fwd_ragged / ptts_gru_bwd_ragged: the same launches over a zero-padded batch with a length per row, every row walked
// over its own length (inference, and masked training with gates and r*h stored).
#include "common.h"

namespace ptts {

typedef float f32x4g __attribute__((ext_vector_type(4)));
constexpr int GCH = 16;    // k-steps per register chunk: all loads of a chunk are issued before its first MFMA

__host__ __device__ static inline int round16(int n) { return (n + 15) & ~15; }
__host__ __device__ static inline int tiles16(int n) { return (n + 15) / 16; }

__device__ __forceinline__ float hard_sigmoid(float a) { return fminf(fmaxf(0.2f * a + 0.5f, 0.f), 1.f); }
// Derivative taken from the stored gate value: 0.2 strictly inside (0, 1), 0 where clipped.  At the ties a = +-2.5 (gate
// exactly 0 or 1) TF's clip_by_value passes the gradient and this does not: a set of measure zero.
__device__ __forceinline__ float hard_sigmoid_grad(float g) { return (g > 0.f && g < 1.f) ? 0.2f : 0.f; }

// Upk[d][jt][w][lane][st] = U[d][k][c0 + col]  (trans = 0)   or   U[d][col][c0 + k]  (trans = 1),
//   col = jt*16 + (lane & 15),  k = w*KP/4 + (lane >> 4)*KS + st,  KP = round16(K), KS = KP/16;  0 where k >= K or col >= N.
// U [ndir][H][3H].
__global__ void gru_pack_kernel(const float* __restrict__ U, float* __restrict__ Upk, int H, int ndir, int K, int N, int c0,
                                int trans) {
    const int KS = round16(K) / 16, NT = tiles16(N);
    const long long G3 = 3LL * H;
    const long long total = (long long)ndir * NT * 256 * KS;
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        long long r = i;
        const int st = (int)(r % KS); r /= KS;
        const int lane = (int)(r % 64); r /= 64;
        const int w = (int)(r % 4); r /= 4;
        const int jt = (int)(r % NT);
        const int d = (int)(r / NT);
        const int k = w * 4 * KS + (lane >> 4) * KS + st, col = jt * 16 + (lane & 15);
        float v = 0.f;
        if (k < K && col < N)
            v = trans ? U[((long long)d * H + col) * G3 + c0 + k] : U[((long long)d * H + k) * G3 + c0 + col];
        Upk[i] = v;
    }
}

// One wave's share of a 16 x 16 tile  D[sample r16][col] = sum_k A(k) . Bpk(k, col)  over k = kbase + st, st < KS, where
// loadA(k) is this lane's A operand (sample b0 + (lane & 15)) and bp this lane's packed B operands.  Even and odd k-steps go
// to two accumulators (half the dependent MFMA chain), added at the end: a fixed order, so the result is reproducible.
// The wave's partial tile is left in red[sample * 16 + col].
template <class LoadA>
__device__ __forceinline__ void gru_wave_tile(const float* __restrict__ bp, int KS, int kbase, LoadA loadA, float* red) {
    const int lane = threadIdx.x & 63, r16 = lane & 15, q = lane >> 4;
    f32x4g acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = {0.f, 0.f, 0.f, 0.f};
    for (int s0 = 0; s0 < KS; s0 += GCH) {
        float a[GCH], bv[GCH];
#pragma unroll
        for (int i = 0; i < GCH; ++i) {
            const bool in = s0 + i < KS;
            a[i] = in ? loadA(kbase + s0 + i) : 0.f;
            bv[i] = in ? bp[s0 + i] : 0.f;
        }
#pragma unroll
        for (int i = 0; i < GCH; i += 2) {
            if (s0 + i < KS) acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(a[i], bv[i], acc0, 0, 0, 0);
            if (s0 + i + 1 < KS) acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(a[i + 1], bv[i + 1], acc1, 0, 0, 0);
        }
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) red[(q * 4 + r) * 16 + r16] = acc0[r] + acc1[r];
}

// Ragged inference (RAG): lens [B] holds each row's own length, 1 <= lens[b] <= T (a larger value is read as T).  Row b is active
// while s < lens[b]; the backward direction works on t = lens[b] - 1 - s and reads its previous state at the row's own t + 1.  An inactive row gives a
// zero operand, writes h = 0 at t = s (launch B) and nothing else.  z and rh pass from launch A to launch B through
// zc, rhc [ndir][B][H]; gates and rh are stored only where the caller passes them.  Both launches are bodies templated on RAG
// behind two __global__ entries: with RAG = false the extra pointers are compile-time null and the code is the training kernel's.

// Forward launch A of step s: grid (tiles16(2H), ceil(B/16), ndir), 256 threads.
template <bool RAG>
__device__ __forceinline__ void gru_fwd_zr_body(
    const float* __restrict__ xproj, const float* __restrict__ Upk, const float* __restrict__ h_out, float* __restrict__ gates,
    float* __restrict__ rh, int B, int T, int H, int ndir, int s, const int* __restrict__ lens, float* __restrict__ zc,
    float* __restrict__ rhc) {
    __shared__ float red[4][256];
    // a latency chain that shares its CUs with the wide kernels of other streams: its waves go first at the issue arbiter
    __builtin_amdgcn_s_setprio(3);
    const int d = blockIdx.z;
    int t = d == 1 ? T - 1 - s : s, tp = d == 1 ? t + 1 : t - 1;
    const int jt = blockIdx.x, b0 = blockIdx.y * 16;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r16 = lane & 15, q = lane >> 4;
    const int KS = round16(H) / 16, NT = tiles16(2 * H);
    const long long G3 = 3LL * H, GG = ndir * G3, HH = (long long)ndir * H;
    // epilogue inputs first: sample eb, column c of the z|r block
    const int eb = b0 + (tid >> 4), c = jt * 16 + (tid & 15);
    const int len_e = RAG ? (eb < B ? min(lens[eb], T) : 0) : T;
    const int len_a = RAG ? (b0 + r16 < B ? min(lens[b0 + r16], T) : 0) : T;
    const bool epi = eb < B && c < 2 * H && (!RAG || s < len_e);
    if (RAG && d == 1) { t = len_e - 1 - s; tp = t + 1; }
    float xv = 0.f, hp = 0.f;
    if (epi) {
        xv = xproj[((long long)eb * T + t) * GG + d * G3 + c];
        if (s > 0 && c >= H) hp = h_out[((long long)eb * T + tp) * HH + (long long)d * H + c - H];
    }
    if (s > 0) {
        const int b = b0 + r16;
        const bool bok = RAG ? s < len_a : b < B;
        const int tpa = RAG ? (bok ? (d == 1 ? len_a - s : s - 1) : 0) : tp;
        const float* hrow = h_out + ((long long)(bok ? b : 0) * T + tpa) * HH + (long long)d * H;
        const float* bp = Upk + ((((long long)d * NT + jt) * 4 + wave) * 64 + lane) * KS;
        gru_wave_tile(bp, KS, wave * 4 * KS + q * KS, [&](int k) { return bok && k < H ? hrow[k] : 0.f; }, red[wave]);
        __syncthreads();
    }
    if (!epi) return;
    float a = xv;
    if (s > 0) a += red[0][tid] + red[1][tid] + red[2][tid] + red[3][tid];
    const float g = hard_sigmoid(a);
    const long long row = (long long)eb * T + t;
    if (!RAG || gates) gates[row * GG + d * G3 + c] = g;
    if (RAG) {
        const long long si = ((long long)d * B + eb) * H;
        if (c < H) zc[si + c] = g;
        else rhc[si + c - H] = g * hp;
    }
    if (c >= H && (!RAG || rh)) rh[row * HH + (long long)d * H + c - H] = g * hp;
}

__global__ __launch_bounds__(256) void gru_fwd_zr_kernel(
    const float* __restrict__ xproj, const float* __restrict__ Upk, const float* __restrict__ h_out, float* __restrict__ gates,
    float* __restrict__ rh, int B, int T, int H, int ndir, int s) {
    gru_fwd_zr_body<false>(xproj, Upk, h_out, gates, rh, B, T, H, ndir, s, nullptr, nullptr, nullptr);
}

__global__ __launch_bounds__(256) void gru_fwd_zr_ragged_kernel(
    const float* __restrict__ xproj, const float* __restrict__ Upk, const float* __restrict__ h_out, float* __restrict__ gates,
    float* __restrict__ rh, int B, int T, int H, int ndir, int s, const int* __restrict__ lens, float* __restrict__ zc,
    float* __restrict__ rhc) {
    gru_fwd_zr_body<true>(xproj, Upk, h_out, gates, rh, B, T, H, ndir, s, lens, zc, rhc);
}

// Forward launch B of step s: grid (tiles16(H), ceil(B/16), ndir), 256 threads.
template <bool RAG>
__device__ __forceinline__ void gru_fwd_h_body(
    const float* __restrict__ xproj, const float* __restrict__ Upk, float* __restrict__ h_out, float* __restrict__ gates,
    const float* __restrict__ rh, int B, int T, int H, int ndir, int s, const int* __restrict__ lens,
    const float* __restrict__ zc, const float* __restrict__ rhc) {
    __shared__ float red[4][256];
    __builtin_amdgcn_s_setprio(3);
    const int d = blockIdx.z;
    int t = d == 1 ? T - 1 - s : s, tp = d == 1 ? t + 1 : t - 1;
    const int jt = blockIdx.x, b0 = blockIdx.y * 16;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r16 = lane & 15, q = lane >> 4;
    const int KS = round16(H) / 16, NT = tiles16(H);
    const long long G3 = 3LL * H, GG = ndir * G3, HH = (long long)ndir * H;
    const int eb = b0 + (tid >> 4), j = jt * 16 + (tid & 15);
    const int len_e = RAG ? (eb < B ? min(lens[eb], T) : 0) : T;
    const int len_a = RAG ? (b0 + r16 < B ? min(lens[b0 + r16], T) : 0) : T;
    const bool own = eb < B && j < H;
    const bool epi = own && (!RAG || s < len_e);
    if (RAG && d == 1) { t = len_e - 1 - s; tp = t + 1; }
    const long long row = (long long)eb * T + t;
    float xv = 0.f, z = 0.f, hp = 0.f;
    if (epi) {
        xv = xproj[row * GG + d * G3 + 2 * H + j];
        z = RAG ? zc[((long long)d * B + eb) * H + j] : gates[row * GG + d * G3 + j];
        if (s > 0) hp = h_out[((long long)eb * T + tp) * HH + (long long)d * H + j];
    }
    if (s > 0) {      // at s = 0, rh = r * h_{-1} = 0
        const int b = b0 + r16;
        const bool bok = RAG ? s < len_a : b < B;
        const float* rrow = RAG ? rhc + ((long long)d * B + (bok ? b : 0)) * H
                                : rh + ((long long)(bok ? b : 0) * T + t) * HH + (long long)d * H;
        const float* bp = Upk + ((((long long)d * NT + jt) * 4 + wave) * 64 + lane) * KS;
        gru_wave_tile(bp, KS, wave * 4 * KS + q * KS, [&](int k) { return bok && k < H ? rrow[k] : 0.f; }, red[wave]);
        __syncthreads();
    }
    if (RAG && own && !epi) h_out[((long long)eb * T + s) * HH + (long long)d * H + j] = 0.f;
    if (!epi) return;
    float a = xv;
    if (s > 0) a += red[0][tid] + red[1][tid] + red[2][tid] + red[3][tid];
    const float hh = tanhf(a);
    if (!RAG || gates) gates[row * GG + d * G3 + 2 * H + j] = hh;
    h_out[row * HH + (long long)d * H + j] = z * hp + (1.f - z) * hh;
}

__global__ __launch_bounds__(256) void gru_fwd_h_kernel(
    const float* __restrict__ xproj, const float* __restrict__ Upk, float* __restrict__ h_out, float* __restrict__ gates,
    const float* __restrict__ rh, int B, int T, int H, int ndir, int s) {
    gru_fwd_h_body<false>(xproj, Upk, h_out, gates, rh, B, T, H, ndir, s, nullptr, nullptr, nullptr);
}

__global__ __launch_bounds__(256) void gru_fwd_h_ragged_kernel(
    const float* __restrict__ xproj, const float* __restrict__ Upk, float* __restrict__ h_out, float* __restrict__ gates,
    const float* __restrict__ rh, int B, int T, int H, int ndir, int s, const int* __restrict__ lens,
    const float* __restrict__ zc, const float* __restrict__ rhc) {
    gru_fwd_h_body<true>(xproj, Upk, h_out, gates, rh, B, T, H, ndir, s, lens, zc, rhc);
}

// Backward launch A' of forward step s (launched for s = T-1 .. 0): grid (tiles16(H), ceil(B/16), ndir), 256 threads.
// dh = dh_out[t] + carry (dh_{t} through the recurrence, left by B' of step s+1).  Each workgroup recomputes da_h over its
// K range as the MFMA's A operand; for its own 16 units it writes dgates (z, r, h) and carry2 = dh z + d(rh) r.
// Ragged backward (RAG, masked training): the backward of ptts_gru_fwd_ragged's walk.  Row b is active in forward step s while
// s < len = lens[b] (a larger value is read as T), the backward direction at the row's own t = len - 1 - s, and the row has a
// next step, whose carry it takes, while s < len - 1: its last step starts from the zero gradient the lone utterance ends
// with.  An inactive row gives a zero operand, writes dgates = +0 at t = s (so every (b, t) is written exactly once) and
// touches neither carry; nothing is read of dh_out, h_out or gates at t >= len.  Bodies templated on RAG behind two entries,
// as in the forward.
template <bool RAG>
__device__ __forceinline__ void gru_bwd_h_body(
    const float* __restrict__ dh_out, const float* __restrict__ Upk, const float* __restrict__ h_out,
    const float* __restrict__ gates, float* __restrict__ dgates, const float* __restrict__ carry, float* __restrict__ carry2,
    int B, int T, int H, int ndir, int s, const int* __restrict__ lens) {
    __shared__ float red[4][256];
    __builtin_amdgcn_s_setprio(3);
    const int d = blockIdx.z;
    int t = d == 1 ? T - 1 - s : s, tp = d == 1 ? t + 1 : t - 1;
    const int jt = blockIdx.x, b0 = blockIdx.y * 16;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r16 = lane & 15, q = lane >> 4;
    const int KS = round16(H) / 16, NT = tiles16(H);
    const long long G3 = 3LL * H, GG = ndir * G3, HH = (long long)ndir * H;
    const int eb = b0 + (tid >> 4), j = jt * 16 + (tid & 15);
    const int len_e = RAG ? (eb < B ? min(lens[eb], T) : 0) : T;
    const int len_a = RAG ? (b0 + r16 < B ? min(lens[b0 + r16], T) : 0) : T;
    const bool has_next = s < len_e - 1;          // of the epilogue's row (RAG = false: s < T - 1)
    const bool own = eb < B && j < H;
    const bool epi = own && (!RAG || s < len_e);
    if (RAG && d == 1) { t = len_e - 1 - s; tp = t + 1; }
    const long long row = (long long)eb * T + t;
    float dh = 0.f, z = 0.f, r = 0.f, hh = 0.f, hp = 0.f;
    if (epi) {
        dh = dh_out[row * HH + (long long)d * H + j];
        if (has_next) dh += carry[((long long)d * B + eb) * H + j];
        const float* gp = gates + row * GG + d * G3;
        z = gp[j]; r = gp[H + j]; hh = gp[2 * H + j];
        if (s > 0) hp = h_out[((long long)eb * T + tp) * HH + (long long)d * H + j];
    }
    if (s > 0) {      // at s = 0, d(rh) only meets h_{-1} = 0 and no earlier step takes carry2
        const int b = b0 + r16;
        const bool bok = RAG ? s < len_a : b < B;
        const bool next_a = s < len_a - 1;
        const int ta = RAG ? (bok ? (d == 1 ? len_a - 1 - s : s) : 0) : t;
        const long long bs = bok ? b : 0;
        const float* dhrow = dh_out + (bs * T + ta) * HH + (long long)d * H;
        const float* crow = carry + ((long long)d * B + bs) * H;
        const float* grow = gates + (bs * T + ta) * GG + d * G3;
        const float* bp = Upk + ((((long long)d * NT + jt) * 4 + wave) * 64 + lane) * KS;
        gru_wave_tile(bp, KS, wave * 4 * KS + q * KS, [&](int n) {
            if (!(bok && n < H)) return 0.f;
            float g = dhrow[n];
            if (next_a) g += crow[n];
            const float zn = grow[n], hn = grow[2 * H + n];
            return g * (1.f - zn) * (1.f - hn * hn);
        }, red[wave]);
        __syncthreads();
    }
    if (RAG && own && !epi) {
        float* dg = dgates + ((long long)eb * T + s) * GG + d * G3;
        dg[j] = 0.f; dg[H + j] = 0.f; dg[2 * H + j] = 0.f;
    }
    if (!epi) return;
    const float drh = s > 0 ? red[0][tid] + red[1][tid] + red[2][tid] + red[3][tid] : 0.f;
    const float da_h = dh * (1.f - z) * (1.f - hh * hh);      // the expression of the operand above: the same rounding
    float* dg = dgates + row * GG + d * G3;
    dg[j] = dh * (hp - hh) * hard_sigmoid_grad(z);
    dg[H + j] = drh * hp * hard_sigmoid_grad(r);
    dg[2 * H + j] = da_h;
    carry2[((long long)d * B + eb) * H + j] = dh * z + drh * r;
}

__global__ __launch_bounds__(256) void gru_bwd_h_kernel(
    const float* __restrict__ dh_out, const float* __restrict__ Upk, const float* __restrict__ h_out,
    const float* __restrict__ gates, float* __restrict__ dgates, const float* __restrict__ carry, float* __restrict__ carry2,
    int B, int T, int H, int ndir, int s) {
    gru_bwd_h_body<false>(dh_out, Upk, h_out, gates, dgates, carry, carry2, B, T, H, ndir, s, nullptr);
}

__global__ __launch_bounds__(256) void gru_bwd_h_ragged_kernel(
    const float* __restrict__ dh_out, const float* __restrict__ Upk, const float* __restrict__ h_out,
    const float* __restrict__ gates, float* __restrict__ dgates, const float* __restrict__ carry, float* __restrict__ carry2,
    int B, int T, int H, int ndir, int s, const int* __restrict__ lens) {
    gru_bwd_h_body<true>(dh_out, Upk, h_out, gates, dgates, carry, carry2, B, T, H, ndir, s, lens);
}

// Backward launch B' of forward step s (s >= 1): carry = carry2 + da_zr.U_zr^T; grid (tiles16(H), ceil(B/16), ndir).
template <bool RAG>
__device__ __forceinline__ void gru_bwd_zr_body(
    const float* __restrict__ Upk, const float* __restrict__ dgates, const float* __restrict__ carry2, float* __restrict__ carry,
    int B, int T, int H, int ndir, int s, const int* __restrict__ lens) {
    __shared__ float red[4][256];
    __builtin_amdgcn_s_setprio(3);
    const int d = blockIdx.z;
    const int t0 = d == 1 ? T - 1 - s : s;
    const int jt = blockIdx.x, b0 = blockIdx.y * 16;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r16 = lane & 15, q = lane >> 4;
    const int KS = round16(2 * H) / 16, NT = tiles16(H);
    const long long G3 = 3LL * H, GG = ndir * G3;
    const int eb = b0 + (tid >> 4), j = jt * 16 + (tid & 15);
    const int len_e = RAG ? (eb < B ? min(lens[eb], T) : 0) : T;
    const int len_a = RAG ? (b0 + r16 < B ? min(lens[b0 + r16], T) : 0) : T;
    const bool epi = eb < B && j < H && (!RAG || s < len_e);
    const long long si = ((long long)d * B + eb) * H + j;
    const float base = epi ? carry2[si] : 0.f;
    const int b = b0 + r16;
    const bool bok = RAG ? s < len_a : b < B;
    const int t = RAG ? (bok ? (d == 1 ? len_a - 1 - s : s) : 0) : t0;
    const float* grow = dgates + ((long long)(bok ? b : 0) * T + t) * GG + d * G3;
    const float* bp = Upk + ((((long long)d * NT + jt) * 4 + wave) * 64 + lane) * KS;
    gru_wave_tile(bp, KS, wave * 4 * KS + q * KS, [&](int n) { return bok && n < 2 * H ? grow[n] : 0.f; }, red[wave]);
    __syncthreads();
    if (!epi) return;
    carry[si] = base + (red[0][tid] + red[1][tid] + red[2][tid] + red[3][tid]);
}

__global__ __launch_bounds__(256) void gru_bwd_zr_kernel(
    const float* __restrict__ Upk, const float* __restrict__ dgates, const float* __restrict__ carry2, float* __restrict__ carry,
    int B, int T, int H, int ndir, int s) {
    gru_bwd_zr_body<false>(Upk, dgates, carry2, carry, B, T, H, ndir, s, nullptr);
}

__global__ __launch_bounds__(256) void gru_bwd_zr_ragged_kernel(
    const float* __restrict__ Upk, const float* __restrict__ dgates, const float* __restrict__ carry2, float* __restrict__ carry,
    int B, int T, int H, int ndir, int s, const int* __restrict__ lens) {
    gru_bwd_zr_body<true>(Upk, dgates, carry2, carry, B, T, H, ndir, s, lens);
}

// floats of one packed operand: ndir x tiles16(N) x 256 lanes x KS
static inline size_t packed_floats(int ndir, int K, int N) { return (size_t)ndir * tiles16(N) * 256 * (round16(K) / 16); }

static void launch_pack(const float* U, float* Upk, int H, int ndir, int K, int N, int c0, int trans, hipStream_t st) {
    const size_t total = packed_floats(ndir, K, N);
    const int blocks = (int)(total / 256 + 1 < 1024 ? total / 256 + 1 : 1024);
    hipLaunchKernelGGL(gru_pack_kernel, dim3(blocks), dim3(256), 0, st, U, Upk, H, ndir, K, N, c0, trans);
}

}  // namespace ptts

using namespace ptts;

extern "C" size_t ptts_gru_fwd_workspace_bytes(int B, int T, int H, int ndir) {
    (void)B; (void)T;
    if (H < 1 || ndir < 1) return 16;
    return (packed_floats(ndir, H, 2 * H) + packed_floats(ndir, H, H)) * sizeof(float);
}

extern "C" int ptts_gru_fwd(const float* xproj, const float* U, float* h_out, float* gates, float* rh, void* workspace,
                            size_t workspace_bytes, int B, int T, int H, int ndir, void* stream) {
    PTTS_REQUIRE(xproj && U && h_out && gates && rh, "gru_fwd: null tensor");
    PTTS_REQUIRE(B > 0 && T > 0 && H > 0 && (ndir == 1 || ndir == 2), "gru_fwd: bad dims B=%d T=%d H=%d ndir=%d", B, T, H, ndir);
    const size_t need = ptts_gru_fwd_workspace_bytes(B, T, H, ndir);
    if (!workspace || workspace_bytes < need) {
        set_error("gru_fwd: workspace %zu < %zu", workspace_bytes, need);
        return PTTS_EWORKSPACE;
    }
    hipStream_t st = (hipStream_t)stream;
    float* Uzr = (float*)workspace;                        // U[:, 0:2H]: K = H, N = 2H
    float* Uh = Uzr + packed_floats(ndir, H, 2 * H);       // U[:, 2H:3H]: K = H, N = H
    launch_pack(U, Uzr, H, ndir, H, 2 * H, 0, 0, st);
    launch_pack(U, Uh, H, ndir, H, H, 2 * H, 0, st);
    const dim3 gzr(tiles16(2 * H), tiles16(B), ndir), gh(tiles16(H), tiles16(B), ndir);
    for (int s = 0; s < T; ++s) {
        hipLaunchKernelGGL(gru_fwd_zr_kernel, gzr, dim3(256), 0, st, xproj, (const float*)Uzr, (const float*)h_out, gates, rh,
                           B, T, H, ndir, s);
        hipLaunchKernelGGL(gru_fwd_h_kernel, gh, dim3(256), 0, st, xproj, (const float*)Uh, h_out, gates, (const float*)rh,
                           B, T, H, ndir, s);
    }
    return check_launch("gru_fwd");
}

// Forward for inference over a zero-padded batch with a length per row (see gru_fwd_zr_body); both directions of a
// bidirectional pair, no single reversed direction (as ptts_gru_fwd).  gates and rh may be NULL.  workspace: the two packed
// operands of ptts_gru_fwd_workspace_bytes, then the z and r*h carries, 2*ndir*B*H floats.
extern "C" int ptts_gru_fwd_ragged(const float* xproj, const float* U, float* h_out, float* gates, float* rh,
                                   const int* lens, void* workspace, size_t workspace_bytes, int B, int T, int H, int ndir,
                                   void* stream) {
    PTTS_REQUIRE(xproj && U && h_out && lens, "gru_fwd_ragged: null tensor");
    PTTS_REQUIRE(B > 0 && T > 0 && H > 0 && (ndir == 1 || ndir == 2), "gru_fwd_ragged: bad dims B=%d T=%d H=%d ndir=%d", B, T, H, ndir);
    const size_t need = ptts_gru_fwd_workspace_bytes(B, T, H, ndir) + (size_t)2 * ndir * B * H * sizeof(float);
    if (!workspace || workspace_bytes < need) {
        set_error("gru_fwd_ragged: workspace %zu < %zu", workspace_bytes, need);
        return PTTS_EWORKSPACE;
    }
    hipStream_t st = (hipStream_t)stream;
    float* Uzr = (float*)workspace;
    float* Uh = Uzr + packed_floats(ndir, H, 2 * H);
    float* zc = Uh + packed_floats(ndir, H, H);
    float* rhc = zc + (size_t)ndir * B * H;
    launch_pack(U, Uzr, H, ndir, H, 2 * H, 0, 0, st);
    launch_pack(U, Uh, H, ndir, H, H, 2 * H, 0, st);
    const dim3 gzr(tiles16(2 * H), tiles16(B), ndir), gh(tiles16(H), tiles16(B), ndir);
    for (int s = 0; s < T; ++s) {
        hipLaunchKernelGGL(gru_fwd_zr_ragged_kernel, gzr, dim3(256), 0, st, xproj, (const float*)Uzr, (const float*)h_out,
                           gates, rh, B, T, H, ndir, s, lens, zc, rhc);
        hipLaunchKernelGGL(gru_fwd_h_ragged_kernel, gh, dim3(256), 0, st, xproj, (const float*)Uh, h_out, gates,
                           (const float*)rh, B, T, H, ndir, s, lens, (const float*)zc, (const float*)rhc);
    }
    return check_launch("gru_fwd_ragged");
}

extern "C" size_t ptts_gru_bwd_workspace_bytes(int B, int T, int H, int ndir) {
    (void)T;
    if (B < 1 || H < 1 || ndir < 1) return 16;
    return (packed_floats(ndir, H, H) + packed_floats(ndir, 2 * H, H) + (size_t)2 * ndir * B * H) * sizeof(float);
}

// The launches of ptts_gru_bwd (lens NULL) and of ptts_gru_bwd_ragged.
static int gru_bwd_run(const char* what, const float* dh_out, const float* U, const float* h_out, const float* gates,
                       float* dgates, const int* lens, void* workspace, size_t workspace_bytes, int B, int T, int H, int ndir,
                       void* stream) {
    PTTS_REQUIRE(dh_out && U && h_out && gates && dgates, "%s: null tensor", what);
    PTTS_REQUIRE(B > 0 && T > 0 && H > 0 && (ndir == 1 || ndir == 2), "%s: bad dims B=%d T=%d H=%d ndir=%d", what, B, T, H, ndir);
    const size_t need = ptts_gru_bwd_workspace_bytes(B, T, H, ndir);
    if (!workspace || workspace_bytes < need) {
        set_error("%s: workspace %zu < %zu", what, workspace_bytes, need);
        return PTTS_EWORKSPACE;
    }
    hipStream_t st = (hipStream_t)stream;
    float* UhT = (float*)workspace;                        // U_h^T: K = H (gate units n), N = H (rows j of U)
    float* UzrT = UhT + packed_floats(ndir, H, H);         // U_zr^T: K = 2H, N = H
    float* carry = UzrT + packed_floats(ndir, 2 * H, H);   // [ndir][B][H]: dh_t through the recurrence
    float* carry2 = carry + (size_t)ndir * B * H;          // [ndir][B][H]: its elementwise part
    launch_pack(U, UhT, H, ndir, H, H, 2 * H, 1, st);
    launch_pack(U, UzrT, H, ndir, 2 * H, H, 0, 1, st);
    const dim3 grid(tiles16(H), tiles16(B), ndir);
    for (int s = T - 1; s >= 0; --s) {
        if (lens) {
            hipLaunchKernelGGL(gru_bwd_h_ragged_kernel, grid, dim3(256), 0, st, dh_out, (const float*)UhT, h_out, gates, dgates,
                               (const float*)carry, carry2, B, T, H, ndir, s, lens);
            if (s > 0)
                hipLaunchKernelGGL(gru_bwd_zr_ragged_kernel, grid, dim3(256), 0, st, (const float*)UzrT, (const float*)dgates,
                                   (const float*)carry2, carry, B, T, H, ndir, s, lens);
            continue;
        }
        hipLaunchKernelGGL(gru_bwd_h_kernel, grid, dim3(256), 0, st, dh_out, (const float*)UhT, h_out, gates, dgates,
                           (const float*)carry, carry2, B, T, H, ndir, s);
        if (s > 0)
            hipLaunchKernelGGL(gru_bwd_zr_kernel, grid, dim3(256), 0, st, (const float*)UzrT, (const float*)dgates,
                               (const float*)carry2, carry, B, T, H, ndir, s);
    }
    return check_launch(what);
}

extern "C" int ptts_gru_bwd(const float* dh_out, const float* U, const float* h_out, const float* gates, float* dgates,
                            void* workspace, size_t workspace_bytes, int B, int T, int H, int ndir, void* stream) {
    return gru_bwd_run("gru_bwd", dh_out, U, h_out, gates, dgates, nullptr, workspace, workspace_bytes, B, T, H, ndir, stream);
}

extern "C" int ptts_gru_bwd_ragged(const float* dh_out, const float* U, const float* h_out, const float* gates, float* dgates,
                                   const int* lens, void* workspace, size_t workspace_bytes, int B, int T, int H, int ndir,
                                   void* stream) {
    PTTS_REQUIRE(lens, "gru_bwd_ragged: null lens");
    return gru_bwd_run("gru_bwd_ragged", dh_out, U, h_out, gates, dgates, lens, workspace, workspace_bytes, B, T, H, ndir, stream);
}
