// Keras LSTM recurrence (gates i,f,c,o; tanh / sigmoid), both directions of a Bidirectional
// wrapper advanced by the same launches.  Reference: networktts.py:72-96 (pLSTM/pBLSTM), used by
// the generator's f0 branch (modeltts_common.py:82-84).
//
// The input projection x.W+b and every weight gradient are large GEMMs done by ptts_gemm; what
// is left here is the T-sequential part: one small launch per time step that adds h_{t-1}.U,
// applies the gate non-linearities and advances (c, h).  Three per-step paths, chosen by H alone:
//   packed MFMA : lstm_pk_ok(H), i.e. H % 64 == 0 and (H <= 256 or H % 256 == 0): 64, 128, 192, 256, 512, 768, 1024, ...
//                 (forward only with a workspace of ptts_lstm_fwd_workspace_bytes; without one it takes the MFMA path)
//   MFMA        : every other H % 16 == 0 (16, 32, 48, 80, ..., 320, 384, ...)
//   scalar      : any other H; one lane per (sample, unit), h_{t-1} staged in LDS
// Limits: H <= 4096 forward, H <= 1024 backward (the scalar kernels' LDS rows bound every path).
// ptts_lstm_fwd_ragged runs the same three forward paths, chosen the same way, for inference over a zero-padded batch with a
// length per row (compile-time variants of the step kernels, see lstm_fwd_step_body), and ptts_lstm_bwd_ragged the three backward
// paths for masked training on such a batch (see lstm_bwd_step_body).
#include "common.h"

namespace ptts {

constexpr int LX = 64, LY = 4;   // lanes along units, samples per workgroup

__device__ __forceinline__ float sigmoidf_(float x) { return 1.f / (1.f + __expf(-x)); }

// Ragged inference (RAG): lens [B] holds each row's own length, 1 <= lens[b] <= T.  Row b is active while s < lens[b]; a
// backward direction works on t = lens[b] - 1 - s, so it starts at the row's last real frame with zero state, and reads its
// previous state at the row's own t -/+ 1.  An inactive row gives a zero operand, writes h = 0 at t = s (so every (b, t) is
// written exactly once over the T steps) and leaves the state alone.  The cell state is carried in carry [ndir][B][H], read
// and written by the same lane; gates and c_out are stored only where the caller passes them.  A length above T is read as T,
// one below 1 as an empty row: no value of lens can send an access outside the arrays.  Every step kernel below is a
// compile-time variant of its training kernel: without the ragged arguments the code is the training kernel's, with no extra
// argument and no branch.
// The scalar kernel is a body templated on RAG behind two __global__ entries.  The two MFMA kernels take the ragged arguments as a
// trailing parameter pack instead (empty: the training kernel; <const int* lens, float* carry>: ragged), because inlining a body
// into a kernel turns the __restrict__ parameters into scoped-alias metadata and the packed kernel's <8> and <16> then schedule
// differently: with the pack, every training instantiation compiles to the instructions it had before the ragged variants existed.
__device__ __forceinline__ void rag_args(const int*& lens, float*& carry) { lens = nullptr; carry = nullptr; }
__device__ __forceinline__ void rag_args(const int*& lens, float*& carry, const int* l, float* c) { lens = l; carry = c; }

template <bool RAG>
__device__ __forceinline__ void lstm_fwd_step_body(
    const float* __restrict__ xproj, const float* __restrict__ U, float* __restrict__ h_out,
    float* __restrict__ gates, float* __restrict__ c_out, int B, int T, int H, int ndir, int reverse, int s,
    const int* __restrict__ lens, float* __restrict__ carry) {
    extern __shared__ float hs[];   // [LY][H]
    const int d = blockIdx.z;
    const bool rev = ndir == 2 ? d == 1 : reverse != 0;
    int t = rev ? T - 1 - s : s;
    int tp = rev ? t + 1 : t - 1;
    const int tid = threadIdx.y * LX + threadIdx.x;
    const long long HH = (long long)ndir * H;
    if (s > 0) {
        for (int idx = tid; idx < LY * H; idx += LX * LY) {
            const int by = idx / H, k = idx - by * H;
            const int b = blockIdx.y * LY + by;
            if (RAG) {
                const int len = b < B ? min(lens[b], T) : 0;
                const int tpb = rev ? len - s : s - 1;
                hs[idx] = s < len ? h_out[((long long)b * T + tpb) * HH + (long long)d * H + k] : 0.f;
            } else {
                hs[idx] = b < B ? h_out[((long long)b * T + tp) * HH + (long long)d * H + k] : 0.f;
            }
        }
        __syncthreads();
    }
    const int j = blockIdx.x * LX + threadIdx.x;
    const int b = blockIdx.y * LY + threadIdx.y;
    if (j >= H || b >= B) return;
    if (RAG) {
        const int len = min(lens[b], T);
        if (s >= len) {
            h_out[((long long)b * T + s) * HH + (long long)d * H + j] = 0.f;
            return;
        }
        if (rev) { t = len - 1 - s; tp = t + 1; }
    }
    const long long G4 = 4LL * H;
    const float* xp = xproj + (((long long)b * T + t) * ndir + d) * G4;
    float a0 = xp[j], a1 = xp[H + j], a2 = xp[2 * H + j], a3 = xp[3 * H + j];
    if (s > 0) {
        const float* Ud = U + (long long)d * H * G4 + j;
        const float* hrow = hs + threadIdx.y * H;
#pragma unroll 4
        for (int k = 0; k < H; ++k) {
            const float hk = hrow[k];
            const float* u = Ud + (long long)k * G4;
            a0 = fmaf(hk, u[0], a0);
            a1 = fmaf(hk, u[H], a1);
            a2 = fmaf(hk, u[2 * H], a2);
            a3 = fmaf(hk, u[3 * H], a3);
        }
    }
    const float gi = sigmoidf_(a0), gf = sigmoidf_(a1), gc = tanhf(a2), go = sigmoidf_(a3);
    const long long so = ((long long)b * T + t) * HH + (long long)d * H + j;
    const long long si = ((long long)d * B + b) * H + j;
    const float cp = s > 0 ? (RAG ? carry[si] : c_out[((long long)b * T + tp) * HH + (long long)d * H + j]) : 0.f;
    const float c = gf * cp + gi * gc;
    if (RAG) carry[si] = c;
    if (!RAG || c_out) c_out[so] = c;
    h_out[so] = go * tanhf(c);
    if (!RAG || gates) {
        float* gp = gates + (((long long)b * T + t) * ndir + d) * G4;
        gp[j] = gi; gp[H + j] = gf; gp[2 * H + j] = gc; gp[3 * H + j] = go;
    }
}

__global__ __launch_bounds__(LX * LY) void lstm_fwd_step_kernel(
    const float* __restrict__ xproj, const float* __restrict__ U, float* __restrict__ h_out,
    float* __restrict__ gates, float* __restrict__ c_out, int B, int T, int H, int ndir, int reverse, int s) {
    lstm_fwd_step_body<false>(xproj, U, h_out, gates, c_out, B, T, H, ndir, reverse, s, nullptr, nullptr);
}

__global__ __launch_bounds__(LX * LY) void lstm_fwd_step_ragged_kernel(
    const float* __restrict__ xproj, const float* __restrict__ U, float* __restrict__ h_out,
    float* __restrict__ gates, float* __restrict__ c_out, int B, int T, int H, int ndir, int reverse, int s,
    const int* __restrict__ lens, float* __restrict__ carry) {
    lstm_fwd_step_body<true>(xproj, U, h_out, gates, c_out, B, T, H, ndir, reverse, s, lens, carry);
}

// UT[d][n][k] = U[d][k][n]
__global__ void lstm_transpose_kernel(const float* __restrict__ U, float* __restrict__ UT, int H, int ndir) {
    const long long n4 = 4LL * H;
    const long long total = (long long)ndir * H * n4;
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total;
         i += (long long)gridDim.x * blockDim.x) {
        const int k = (int)(i % H);
        const long long r = i / H;
        const int n = (int)(r % n4);
        const int d = (int)(r / n4);
        UT[i] = U[((long long)d * H + k) * n4 + n];
    }
}

// Ragged backward (masked training): the backward of ptts_lstm_fwd_ragged's walk.  Row b is active in forward step s while
// s < len = lens[b]; a backward direction worked on t = len - 1 - s, so forward step s + 1 of that row lies at t - 1 of the ROW's
// own t, and the row has a next step while s < len - 1: at its last step (s = len - 1, where the launches for larger s found it
// inactive) neither the recurrent term nor the cell-state carry is read, which is the zero state the lone utterance ends with.
// An inactive row gives a zero operand, writes dgates = +0 at t = s (so every (b, t) is written exactly once over the T steps)
// and leaves the carry alone; nothing is read of gates, c_out or dh_out at t >= len.  A length above T is read as T, one
// below 1 as an empty row.  As in the forward, the scalar kernel is a body templated on RAG behind two __global__ entries and
// the MFMA kernels take `lens` as a trailing parameter pack, so the training instantiations keep their code.
__device__ __forceinline__ void rag_lens(const int*& lens) { lens = nullptr; }
__device__ __forceinline__ void rag_lens(const int*& lens, const int* l) { lens = l; }

// backward of forward step s (launched for s = T-1 .. 0)
template <bool RAG>
__device__ __forceinline__ void lstm_bwd_step_body(
    const float* __restrict__ dh_out, const float* __restrict__ UT, const float* __restrict__ gates,
    const float* __restrict__ c_out, float* __restrict__ dgates, float* __restrict__ dc_state, int B, int T,
    int H, int ndir, int reverse, int s, const int* __restrict__ lens) {
    extern __shared__ float das[];   // [LY][4H]: gate-preactivation grads of forward step s+1
    const int d = blockIdx.z;
    const bool rev = ndir == 2 ? d == 1 : reverse != 0;
    int t = rev ? T - 1 - s : s;
    int tp = rev ? t + 1 : t - 1;         // time of forward step s-1
    const int tn = rev ? t - 1 : t + 1;   // time of forward step s+1
    const int tid = threadIdx.y * LX + threadIdx.x;
    const long long G4 = 4LL * H;
    const long long HH = (long long)ndir * H;
    const bool has_next = s < T - 1;
    if (has_next) {
        for (int idx = tid; idx < LY * (int)G4; idx += LX * LY) {
            const int by = idx / (int)G4, n = idx - by * (int)G4;
            const int b = blockIdx.y * LY + by;
            if (RAG) {
                const int len = b < B ? min(lens[b], T) : 0;
                const int tnb = rev ? len - 2 - s : s + 1;
                das[idx] = s < len - 1 ? dgates[(((long long)b * T + tnb) * ndir + d) * G4 + n] : 0.f;
            } else {
                das[idx] = b < B ? dgates[(((long long)b * T + tn) * ndir + d) * G4 + n] : 0.f;
            }
        }
        __syncthreads();
    }
    const int j = blockIdx.x * LX + threadIdx.x;
    const int b = blockIdx.y * LY + threadIdx.y;
    if (j >= H || b >= B) return;
    bool nxt = has_next;                  // of this row
    if (RAG) {
        const int len = min(lens[b], T);
        if (s >= len) {
            float* dg = dgates + (((long long)b * T + s) * ndir + d) * G4;
            dg[j] = 0.f; dg[H + j] = 0.f; dg[2 * H + j] = 0.f; dg[3 * H + j] = 0.f;
            return;
        }
        if (rev) { t = len - 1 - s; tp = t + 1; }
        nxt = s < len - 1;
    }
    float dh = dh_out[((long long)b * T + t) * HH + (long long)d * H + j];
    if (nxt) {
        const float* ut = UT + (long long)d * G4 * H + j;
        const float* drow = das + threadIdx.y * G4;
        float acc = 0.f;
#pragma unroll 4
        for (int n = 0; n < (int)G4; ++n) acc = fmaf(drow[n], ut[(long long)n * H], acc);
        dh += acc;
    }
    const float* gp = gates + (((long long)b * T + t) * ndir + d) * G4;
    const float gi = gp[j], gf = gp[H + j], gc = gp[2 * H + j], go = gp[3 * H + j];
    const long long so = ((long long)b * T + t) * HH + (long long)d * H + j;
    const float c = c_out[so];
    const float cp = s > 0 ? c_out[((long long)b * T + tp) * HH + (long long)d * H + j] : 0.f;
    const float tc = tanhf(c);
    const long long si = ((long long)d * B + b) * H + j;
    float dc = dh * go * (1.f - tc * tc);
    if (nxt) dc += dc_state[si];
    float* dg = dgates + (((long long)b * T + t) * ndir + d) * G4;
    dg[j] = dc * gc * gi * (1.f - gi);
    dg[H + j] = dc * cp * gf * (1.f - gf);
    dg[2 * H + j] = dc * gi * (1.f - gc * gc);
    dg[3 * H + j] = dh * tc * go * (1.f - go);
    dc_state[si] = dc * gf;
}

__global__ __launch_bounds__(LX * LY) void lstm_bwd_step_kernel(
    const float* __restrict__ dh_out, const float* __restrict__ UT, const float* __restrict__ gates,
    const float* __restrict__ c_out, float* __restrict__ dgates, float* __restrict__ dc_state, int B, int T,
    int H, int ndir, int reverse, int s) {
    lstm_bwd_step_body<false>(dh_out, UT, gates, c_out, dgates, dc_state, B, T, H, ndir, reverse, s, nullptr);
}

__global__ __launch_bounds__(LX * LY) void lstm_bwd_step_ragged_kernel(
    const float* __restrict__ dh_out, const float* __restrict__ UT, const float* __restrict__ gates,
    const float* __restrict__ c_out, float* __restrict__ dgates, float* __restrict__ dc_state, int B, int T,
    int H, int ndir, int reverse, int s, const int* __restrict__ lens) {
    lstm_bwd_step_body<true>(dh_out, UT, gates, c_out, dgates, dc_state, B, T, H, ndir, reverse, s, lens);
}


// ------------------------------------------------------------------------------------------------
// MFMA step kernels (H % 16 == 0): v_mfma_f32_16x16x4_f32, K split over the 4 waves of a workgroup,
// partial tiles combined through LDS, then one lane per (sample, unit) applies the gate math.
//   forward : tile = 16 samples x 8 units x 4 gates (two MFMA column blocks: gates {i,f} and {c,o}),
//             grid (H/8, ceil(B/16), ndir) = 256 workgroups at H = 256, B = 64 -> every CU busy.
//   backward: tile = 16 samples x 16 units of dh_rec = da_next . U^T, grid (H/16, ceil(B/16), ndir).
// ------------------------------------------------------------------------------------------------
typedef float f32x4v __attribute__((ext_vector_type(4)));

template <class... R>   // R: empty, or <const int* lens, float* carry> for ragged inference
__global__ __launch_bounds__(256) void lstm_fwd_step_mfma_kernel(
    const float* __restrict__ xproj, const float* __restrict__ U, float* __restrict__ h_out,
    float* __restrict__ gates, float* __restrict__ c_out, int B, int T, int H, int ndir, int reverse, int s, R... rag) {
    constexpr bool RAG = sizeof...(R) != 0;
    const int* lens; float* carry;
    rag_args(lens, carry, rag...);
    __shared__ float red[4][2][256];
    const int d = blockIdx.z;
    const bool rev = ndir == 2 ? d == 1 : reverse != 0;
    int t = rev ? T - 1 - s : s;
    int tp = rev ? t + 1 : t - 1;
    const int j0 = blockIdx.x * 8, b0 = blockIdx.y * 16;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r16 = lane & 15, q = lane >> 4;
    const long long G4 = 4LL * H, HH = (long long)ndir * H;
    if (s > 0) {
        const int ksteps = H / 16;                 // k-steps of 4 per wave
        const int kbase = wave * (H / 4);
        const int b = b0 + r16;
        int len_a = T;                             // RAG, an inactive row: a valid address, a zero operand
        if (RAG) {
            len_a = b < B ? min(lens[b], T) : 0;
            if (rev) tp = s < len_a ? len_a - s : 0;
        }
        const float* hp = h_out + ((long long)(b < B ? b : 0) * T + tp) * HH + (long long)d * H + kbase + q;
        const float* Ud = U + (long long)d * H * G4 + (long long)(kbase + q) * G4 + j0 + (r16 & 7);
        const int gx = (r16 >> 3) * H, gy = (2 + (r16 >> 3)) * H;
        f32x4v acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = {0.f, 0.f, 0.f, 0.f};
        for (int s0 = 0; s0 < ksteps; s0 += 8) {
            float a[8], bx[8], by[8];
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                const int st = s0 + i;
                if (st < ksteps) {
                    a[i] = (RAG ? s < len_a : b < B) ? hp[4 * st] : 0.f;
                    const float* u = Ud + (long long)(4 * st) * G4;
                    bx[i] = u[gx];
                    by[i] = u[gy];
                } else { a[i] = 0.f; bx[i] = 0.f; by[i] = 0.f; }
            }
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(a[i], bx[i], acc0, 0, 0, 0);
                acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(a[i], by[i], acc1, 0, 0, 0);
            }
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            red[wave][0][(q * 4 + r) * 16 + r16] = acc0[r];
            red[wave][1][(q * 4 + r) * 16 + r16] = acc1[r];
        }
        __syncthreads();
    }
    if (tid >= 128) return;
    const int bb = tid >> 3, jj = tid & 7;
    const int b = b0 + bb, j = j0 + jj;
    if (b >= B) return;
    if (RAG) {
        const int len = min(lens[b], T);
        if (s >= len) {
            h_out[((long long)b * T + s) * HH + (long long)d * H + j] = 0.f;
            return;
        }
        if (rev) { t = len - 1 - s; tp = t + 1; }
    }
    const float* xp = xproj + (((long long)b * T + t) * ndir + d) * G4;
    float a4[4];
#pragma unroll
    for (int g = 0; g < 4; ++g) {
        float v = xp[g * H + j];
        if (s > 0) {
            const int idx = bb * 16 + (g & 1) * 8 + jj;
            v += red[0][g >> 1][idx] + red[1][g >> 1][idx] + red[2][g >> 1][idx] + red[3][g >> 1][idx];
        }
        a4[g] = v;
    }
    const float gi = sigmoidf_(a4[0]), gf = sigmoidf_(a4[1]), gc = tanhf(a4[2]), go = sigmoidf_(a4[3]);
    const long long so = ((long long)b * T + t) * HH + (long long)d * H + j;
    const long long si = ((long long)d * B + b) * H + j;
    const float cp = s > 0 ? (RAG ? carry[si] : c_out[((long long)b * T + tp) * HH + (long long)d * H + j]) : 0.f;
    const float c = gf * cp + gi * gc;
    if (RAG) carry[si] = c;
    if (!RAG || c_out) c_out[so] = c;
    h_out[so] = go * tanhf(c);
    if (!RAG || gates) {
        float* gp = gates + (((long long)b * T + t) * ndir + d) * G4;
        gp[j] = gi; gp[H + j] = gf; gp[2 * H + j] = gc; gp[3 * H + j] = go;
    }
}

template <class... R>   // R: empty, or <const int* lens> for the ragged backward
__global__ __launch_bounds__(256) void lstm_bwd_step_mfma_kernel(
    const float* __restrict__ dh_out, const float* __restrict__ UT, const float* __restrict__ gates,
    const float* __restrict__ c_out, float* __restrict__ dgates, float* __restrict__ dc_state, int B, int T,
    int H, int ndir, int reverse, int s, R... rag) {
    constexpr bool RAG = sizeof...(R) != 0;
    const int* lens;
    rag_lens(lens, rag...);
    __shared__ float red[4][256];
    const int d = blockIdx.z;
    const bool rev = ndir == 2 ? d == 1 : reverse != 0;
    int t = rev ? T - 1 - s : s;
    int tp = rev ? t + 1 : t - 1;
    const int tn = rev ? t - 1 : t + 1;
    const int j0 = blockIdx.x * 16, b0 = blockIdx.y * 16;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r16 = lane & 15, q = lane >> 4;
    const long long G4 = 4LL * H, HH = (long long)ndir * H;
    const bool has_next = s < T - 1;
    if (has_next) {
        const int nsteps = H / 4;                  // n-steps of 4 per wave (each wave owns H of the 4H gate columns)
        const int nbase = wave * H;
        const int b = b0 + r16;
        bool a_on = b < B;                          // the tile row has a next step
        int tna = tn;
        if constexpr (RAG) {
            const int len = b < B ? min(lens[b], T) : 0;
            a_on = s < len - 1;
            tna = a_on ? (rev ? len - 2 - s : s + 1) : 0;
        }
        const float* ap = dgates + (((long long)(a_on ? b : 0) * T + tna) * ndir + d) * G4 + nbase + q;
        const float* bp = UT + (long long)d * G4 * H + (long long)(nbase + q) * H + j0 + r16;
        f32x4v acc = {0.f, 0.f, 0.f, 0.f};
        for (int s0 = 0; s0 < nsteps; s0 += 16) {
            float a[16], bv[16];
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                const int st = s0 + i;
                if (st < nsteps) {
                    a[i] = a_on ? ap[4 * st] : 0.f;
                    bv[i] = bp[(long long)(4 * st) * H];
                } else { a[i] = 0.f; bv[i] = 0.f; }
            }
#pragma unroll
            for (int i = 0; i < 16; ++i) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a[i], bv[i], acc, 0, 0, 0);
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) red[wave][(q * 4 + r) * 16 + r16] = acc[r];
        __syncthreads();
    }
    const int bb = tid >> 4, jj = tid & 15;
    const int b = b0 + bb, j = j0 + jj;
    if (b >= B) return;
    bool nxt = has_next;                            // of this row
    if constexpr (RAG) {
        const int len = min(lens[b], T);
        if (s >= len) {
            float* dg = dgates + (((long long)b * T + s) * ndir + d) * (4LL * H);
            dg[j] = 0.f; dg[H + j] = 0.f; dg[2 * H + j] = 0.f; dg[3 * H + j] = 0.f;
            return;
        }
        if (rev) { t = len - 1 - s; tp = t + 1; }
        nxt = s < len - 1;
    }
    float dh = dh_out[((long long)b * T + t) * HH + (long long)d * H + j];
    if (nxt) dh += red[0][tid] + red[1][tid] + red[2][tid] + red[3][tid];
    const float* gp = gates + (((long long)b * T + t) * ndir + d) * G4;
    const float gi = gp[j], gf = gp[H + j], gc = gp[2 * H + j], go = gp[3 * H + j];
    const long long so = ((long long)b * T + t) * HH + (long long)d * H + j;
    const float c = c_out[so];
    const float cp = s > 0 ? c_out[((long long)b * T + tp) * HH + (long long)d * H + j] : 0.f;
    const float tc = tanhf(c);
    const long long si = ((long long)d * B + b) * H + j;
    float dc = dh * go * (1.f - tc * tc);
    if (nxt) dc += dc_state[si];
    float* dg = dgates + (((long long)b * T + t) * ndir + d) * G4;
    dg[j] = dc * gc * gi * (1.f - gi);
    dg[H + j] = dc * cp * gf * (1.f - gf);
    dg[2 * H + j] = dc * gi * (1.f - gc * gc);
    dg[3 * H + j] = dh * tc * go * (1.f - go);
    dc_state[si] = dc * gf;
}


// ------------------------------------------------------------------------------------------------
// Packed-operand MFMA step kernels (H % 64 == 0): the recurrent kernel is re-laid once per call so that every
// lane's MFMA B operands of all k-steps are contiguous (16-byte loads, whole lines per wave), the k index of step
// `st` for lane group q is  k = wave*(K/4) + q*KS + st  so the lane's A operands (h / dgates rows) are contiguous
// too, and every global load of a step (operands AND the gate inputs of the epilogue) is issued before the first
// wait.  The step is latency-bound: this cuts it to one exposed L2 round trip.
// ------------------------------------------------------------------------------------------------
typedef float f32x4a __attribute__((ext_vector_type(4)));

// Upk[d][jt][w][lane][st][2] = { U[d][k][gate(i|f) col], U[d][k][gate(c|o) col] },  k = w*H/4 + q*KS + st
__global__ void lstm_pack_u_fwd_kernel(const float* __restrict__ U, float* __restrict__ Upk, int H, int ndir) {
    const int KS = H / 16, JT = H / 8;
    const long long total = (long long)ndir * JT * 4 * 64 * KS * 2;
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total;
         i += (long long)gridDim.x * blockDim.x) {
        long long r = i;
        const int e = (int)(r % 2); r /= 2;
        const int st = (int)(r % KS); r /= KS;
        const int lane = (int)(r % 64); r /= 64;
        const int w = (int)(r % 4); r /= 4;
        const int jt = (int)(r % JT);
        const int d = (int)(r / JT);
        const int r16 = lane & 15, q = lane >> 4;
        const int k = w * (H / 4) + q * KS + st;
        const int col = ((e == 0 ? 0 : 2) + (r16 >> 3)) * H + jt * 8 + (r16 & 7);
        Upk[i] = U[((long long)d * H + k) * 4 * H + col];
    }
}

// UTpk[d][jt][w][lane][st] = U[d][jt*16 + r16][n],  n = w*H + q*(H/4) + st
__global__ void lstm_pack_u_bwd_kernel(const float* __restrict__ U, float* __restrict__ UTpk, int H, int ndir) {
    const int NS = H / 4, JT = H / 16;
    const long long total = (long long)ndir * JT * 4 * 64 * NS;
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total;
         i += (long long)gridDim.x * blockDim.x) {
        long long r = i;
        const int st = (int)(r % NS); r /= NS;
        const int lane = (int)(r % 64); r /= 64;
        const int w = (int)(r % 4); r /= 4;
        const int jt = (int)(r % JT);
        const int d = (int)(r / JT);
        const int r16 = lane & 15, q = lane >> 4;
        const int n = w * H + q * NS + st;
        UTpk[i] = U[((long long)d * H + jt * 16 + r16) * 4 * H + n];
    }
}

// RAG: a lane needs two lengths, its tile row's (A operand) and its epilogue sample's; both loads go out first.  In a forward
// direction no address depends on them (t = s is inside the padded arrays for every row), so the step keeps its one exposed
// L2 round trip and the lengths only mask; in a backward direction the addresses wait for the lengths: one more L2 hit.
template <int CH, class... R>   // CH: k-steps per register chunk (4, 8 or 16); R: empty, or <const int* lens, float* carry>
__global__ __launch_bounds__(256) void lstm_fwd_step_pk_kernel(
    const float* __restrict__ xproj, const float* __restrict__ Upk, float* __restrict__ h_out,
    float* __restrict__ gates, float* __restrict__ c_out, int B, int T, int H, int ndir, int reverse, int s, R... rag) {
    constexpr bool RAG = sizeof...(R) != 0;
    const int* lens; float* carry;
    rag_args(lens, carry, rag...);
    __shared__ float red[4][2][256];
    // a latency chain that shares its CUs with the wide kernels of the other streams: its waves go first at the issue arbiter
    __builtin_amdgcn_s_setprio(3);
    const int d = blockIdx.z;
    const bool rev = ndir == 2 ? d == 1 : reverse != 0;
    int t = rev ? T - 1 - s : s;
    int tp = rev ? t + 1 : t - 1;
    const int jt = blockIdx.x, j0 = jt * 8, b0 = blockIdx.y * 16;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r16 = lane & 15, q = lane >> 4;
    const long long G4 = 4LL * H, HH = (long long)ndir * H;
    const int KS = H / 16;
    // epilogue inputs first: their latency overlaps everything else
    const int bb = tid >> 3, jj = tid & 7;
    const int eb = b0 + bb, ej = j0 + jj;
    const bool epi = tid < 128 && eb < B;
    int len_e = T, len_a = T;
    if (RAG) {
        len_e = epi ? min(lens[eb], T) : 0;
        len_a = b0 + r16 < B ? min(lens[b0 + r16], T) : 0;
    }
    float xv[4] = {0.f, 0.f, 0.f, 0.f}, cp = 0.f;
    if (RAG && rev) {
        if (s < len_e) {
            t = len_e - 1 - s;
            const float* xp = xproj + (((long long)eb * T + t) * ndir + d) * G4;
#pragma unroll
            for (int g = 0; g < 4; ++g) xv[g] = xp[g * H + ej];
            if (s > 0) cp = carry[((long long)d * B + eb) * H + ej];
        }
    } else if (epi) {
        const float* xp = xproj + (((long long)eb * T + t) * ndir + d) * G4;
#pragma unroll
        for (int g = 0; g < 4; ++g) xv[g] = xp[g * H + ej];
        if (s > 0) cp = RAG ? carry[((long long)d * B + eb) * H + ej] : c_out[((long long)eb * T + tp) * HH + (long long)d * H + ej];
    }
    if (s > 0) {
        const int b = b0 + r16;
        if (RAG && rev) tp = s < len_a ? len_a - s : 0;   // an inactive row: a valid address, a zero operand
        const float* hp = h_out + ((long long)(b < B ? b : 0) * T + tp) * HH + (long long)d * H + wave * (H / 4) + q * KS;
        const float* up = Upk + ((((long long)d * (H / 8) + jt) * 4 + wave) * 64 + lane) * KS * 2;
        f32x4v acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = {0.f, 0.f, 0.f, 0.f};
        for (int s0 = 0; s0 < KS; s0 += CH) {
            f32x4a hv[CH / 4], uv[CH / 2];
#pragma unroll
            for (int i = 0; i < CH / 4; ++i) hv[i] = *reinterpret_cast<const f32x4a*>(hp + s0 + 4 * i);
#pragma unroll
            for (int i = 0; i < CH / 2; ++i) uv[i] = *reinterpret_cast<const f32x4a*>(up + 2 * s0 + 4 * i);
#pragma unroll
            for (int i = 0; i < CH; ++i) {
                const float a = (RAG ? s < len_a : b < B) ? hv[i / 4][i % 4] : 0.f;
                acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(a, uv[i / 2][(i % 2) * 2], acc0, 0, 0, 0);
                acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(a, uv[i / 2][(i % 2) * 2 + 1], acc1, 0, 0, 0);
            }
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            red[wave][0][(q * 4 + r) * 16 + r16] = acc0[r];
            red[wave][1][(q * 4 + r) * 16 + r16] = acc1[r];
        }
        __syncthreads();
    }
    if (!epi) return;
    if (RAG && s >= len_e) {
        h_out[((long long)eb * T + s) * HH + (long long)d * H + ej] = 0.f;
        return;
    }
    float a4[4];
#pragma unroll
    for (int g = 0; g < 4; ++g) {
        float v = xv[g];
        if (s > 0) {
            const int idx = bb * 16 + (g & 1) * 8 + jj;
            v += red[0][g >> 1][idx] + red[1][g >> 1][idx] + red[2][g >> 1][idx] + red[3][g >> 1][idx];
        }
        a4[g] = v;
    }
    const float gi = sigmoidf_(a4[0]), gf = sigmoidf_(a4[1]), gc = tanhf(a4[2]), go = sigmoidf_(a4[3]);
    const long long so = ((long long)eb * T + t) * HH + (long long)d * H + ej;
    const float c = gf * cp + gi * gc;
    if (RAG) carry[((long long)d * B + eb) * H + ej] = c;
    if (!RAG || c_out) c_out[so] = c;
    h_out[so] = go * tanhf(c);
    if (!RAG || gates) {
        float* gp = gates + (((long long)eb * T + t) * ndir + d) * G4;
        gp[ej] = gi; gp[H + ej] = gf; gp[2 * H + ej] = gc; gp[3 * H + ej] = go;
    }
}


template <int NW, class... R>   // R: empty, or <const int* lens> for the ragged backward.  NW: waves per workgroup: 4, or 8 (H = 256: the K = 4H reduction over eight waves -- half the dependent MFMA chain and
                    // half the load rounds per wave of this latency-bound step)
__global__ __launch_bounds__(64 * NW) void lstm_bwd_step_pk_kernel(
    const float* __restrict__ dh_out, const float* __restrict__ UTpk, const float* __restrict__ gates,
    const float* __restrict__ c_out, float* __restrict__ dgates, float* __restrict__ dc_state, int B, int T,
    int H, int ndir, int reverse, int s, R... rag) {
    constexpr bool RAG = sizeof...(R) != 0;
    const int* lens;
    rag_lens(lens, rag...);
    __shared__ float red[NW][256];
    __builtin_amdgcn_s_setprio(3);         // as in the forward step: ahead of the co-resident wide kernels' waves
    const int d = blockIdx.z;
    const bool rev = ndir == 2 ? d == 1 : reverse != 0;
    int t = rev ? T - 1 - s : s;
    int tp = rev ? t + 1 : t - 1;
    const int tn = rev ? t - 1 : t + 1;
    const int jt = blockIdx.x, j0 = jt * 16, b0 = blockIdx.y * 16;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int gate = wave & 3, part = wave >> 2;            // NW == 8: the two halves of a gate's quarter rows
    const int r16 = lane & 15, q = lane >> 4;
    const long long G4 = 4LL * H, HH = (long long)ndir * H;
    const bool has_next = s < T - 1;
    const int NS = H / 4, NSW = NS / (NW / 4);
    // epilogue inputs first
    const int bb = tid >> 4, jj = tid & 15;
    const int eb = b0 + bb, ej = j0 + jj;
    const bool epi = tid < 256 && eb < B;
    bool e_on = epi, nxt = has_next;                 // the epilogue's row is active in this step / has a next step
    if constexpr (RAG) {
        const int len = epi ? min(lens[eb], T) : 0;
        e_on = s < len;
        if (rev) { t = len - 1 - s; tp = t + 1; }
        nxt = s < len - 1;
    }
    float dh = 0.f, gi = 0.f, gf = 0.f, gc = 0.f, go = 0.f, c = 0.f, cp = 0.f, dcs = 0.f;
    const long long si = ((long long)d * B + eb) * H + ej;
    if (e_on) {
        dh = dh_out[((long long)eb * T + t) * HH + (long long)d * H + ej];
        const float* gp = gates + (((long long)eb * T + t) * ndir + d) * G4;
        gi = gp[ej]; gf = gp[H + ej]; gc = gp[2 * H + ej]; go = gp[3 * H + ej];
        c = c_out[((long long)eb * T + t) * HH + (long long)d * H + ej];
        if (s > 0) cp = c_out[((long long)eb * T + tp) * HH + (long long)d * H + ej];
        if (nxt) dcs = dc_state[si];
    }
    if (has_next) {
        const int b = b0 + r16;
        bool a_on = b < B;                           // the tile row has a next step
        int tna = tn;
        if constexpr (RAG) {
            const int len = b < B ? min(lens[b], T) : 0;
            a_on = s < len - 1;
            tna = a_on ? (rev ? len - 2 - s : s + 1) : 0;
        }
        const float* ap = dgates + (((long long)(a_on ? b : 0) * T + tna) * ndir + d) * G4 + gate * H + q * NS + part * NSW;
        const float* bp = UTpk + ((((long long)d * (H / 16) + jt) * 4 + gate) * 64 + lane) * NS + part * NSW;
        f32x4v acc = {0.f, 0.f, 0.f, 0.f};
        for (int s0 = 0; s0 < NSW; s0 += 16) {
            f32x4a av[4], bv[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                if (!RAG || a_on) av[i] = *reinterpret_cast<const f32x4a*>(ap + s0 + 4 * i);      // (RAG: dgates of an unfinished row is not read)
                bv[i] = *reinterpret_cast<const f32x4a*>(bp + s0 + 4 * i);
            }
#pragma unroll
            for (int i = 0; i < 16; ++i)
                acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a_on ? av[i / 4][i % 4] : 0.f, bv[i / 4][i % 4], acc, 0, 0, 0);
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) red[wave][(q * 4 + r) * 16 + r16] = acc[r];
        __syncthreads();
    }
    if (!epi) return;
    if constexpr (RAG) {
        if (!e_on) {
            float* dg = dgates + (((long long)eb * T + s) * ndir + d) * G4;
            dg[ej] = 0.f; dg[H + ej] = 0.f; dg[2 * H + ej] = 0.f; dg[3 * H + ej] = 0.f;
            return;
        }
    }
    if (nxt) {
#pragma unroll
        for (int w = 0; w < NW; ++w) dh += red[w][tid];
    }
    const float tc = tanhf(c);
    float dc = dh * go * (1.f - tc * tc);
    if (nxt) dc += dcs;
    float* dg = dgates + (((long long)eb * T + t) * ndir + d) * G4;
    dg[ej] = dc * gc * gi * (1.f - gi);
    dg[H + ej] = dc * cp * gf * (1.f - gf);
    dg[2 * H + ej] = dc * gi * (1.f - gc * gc);
    dg[3 * H + ej] = dh * tc * go * (1.f - go);
    dc_state[si] = dc * gf;
}

static inline bool lstm_pk_ok(int H) { return H % 64 == 0 && ((H / 16) <= 16 ? true : (H / 16) % 16 == 0); }

}  // namespace ptts

using namespace ptts;

// kept for bench.py, which reports these counters: the recurrence graphs were removed, so they are always zero
extern "C" int ptts_lstm_graph_stats(unsigned long long* hits, unsigned long long* captures, unsigned long long* direct) {
    if (hits) *hits = 0;
    if (captures) *captures = 0;
    if (direct) *direct = 0;
    return PTTS_OK;
}

extern "C" size_t ptts_lstm_fwd_workspace_bytes(int B, int T, int H, int ndir) {
    (void)B; (void)T;
    return lstm_pk_ok(H) ? (size_t)ndir * 4 * H * H * sizeof(float) : 16;
}

extern "C" int ptts_lstm_fwd(const float* xproj, const float* U, float* h_out, float* gates, float* c_out,
                             void* workspace, size_t workspace_bytes, int B, int T, int H, int ndir, int reverse,
                             void* stream) {
    PTTS_REQUIRE(xproj && U && h_out && gates && c_out, "lstm_fwd: null tensor");
    PTTS_REQUIRE(B > 0 && T > 0 && H > 0 && (ndir == 1 || ndir == 2), "lstm_fwd: bad dims");
    PTTS_REQUIRE((size_t)LY * H * sizeof(float) <= 64 * 1024, "lstm_fwd: H=%d too large", H);
    hipStream_t st = (hipStream_t)stream;
    dim3 grid((H + LX - 1) / LX, (B + LY - 1) / LY, ndir), block(LX, LY);
    const size_t lds = (size_t)LY * H * sizeof(float);
    if (lstm_pk_ok(H) && workspace && workspace_bytes >= ptts_lstm_fwd_workspace_bytes(B, T, H, ndir)) {
        float* Upk = (float*)workspace;
        dim3 mgrid(H / 8, (B + 15) / 16, ndir);
        const int KS = H / 16;
        hipLaunchKernelGGL(lstm_pack_u_fwd_kernel, dim3(1024), dim3(256), 0, st, U, Upk, H, ndir);
        for (int s = 0; s < T; ++s) {
            // the chunk must divide KS (a lane owns exactly KS k-steps of Upk and of its h row segment); H % 64 == 0 gives KS % 4 == 0
            if (KS % 16 == 0) hipLaunchKernelGGL(lstm_fwd_step_pk_kernel<16>, mgrid, dim3(256), 0, st, xproj, (const float*)Upk, h_out, gates, c_out, B, T, H, ndir, reverse, s);
            else if (KS % 8 == 0) hipLaunchKernelGGL(lstm_fwd_step_pk_kernel<8>, mgrid, dim3(256), 0, st, xproj, (const float*)Upk, h_out, gates, c_out, B, T, H, ndir, reverse, s);
            else hipLaunchKernelGGL(lstm_fwd_step_pk_kernel<4>, mgrid, dim3(256), 0, st, xproj, (const float*)Upk, h_out, gates, c_out, B, T, H, ndir, reverse, s);
        }
        return check_launch("lstm_fwd_pk");
    }
    if (H % 16 == 0) {
        dim3 mgrid(H / 8, (B + 15) / 16, ndir);
        for (int s = 0; s < T; ++s)
            hipLaunchKernelGGL(lstm_fwd_step_mfma_kernel, mgrid, dim3(256), 0, st, xproj, U, h_out, gates, c_out, B, T,
                               H, ndir, reverse, s);
        return check_launch("lstm_fwd_mfma");
    }
    for (int s = 0; s < T; ++s) {
        hipLaunchKernelGGL(lstm_fwd_step_kernel, grid, block, lds, st, xproj, U, h_out, gates, c_out, B, T, H, ndir,
                           reverse, s);
    }
    return check_launch("lstm_fwd");
}

// bytes of the ragged forward's cell-state carry [ndir][B][H] at the head of its workspace (whole 256-byte lines, so the
// packed operand behind it keeps its 16-byte loads)
static inline size_t lstm_carry_bytes(int B, int H, int ndir) {
    return ((size_t)ndir * B * H * sizeof(float) + 255) & ~(size_t)255;
}

// Forward for inference over a zero-padded batch with a length per row (see lstm_fwd_step_body).  gates and c_out may be
// NULL.  workspace: the cell-state carry, ndir*B*H floats rounded up to 256 bytes, then the packed recurrent operand of
// ptts_lstm_fwd_workspace_bytes; without room for the latter a packed-path H takes the MFMA path, as in ptts_lstm_fwd.
extern "C" int ptts_lstm_fwd_ragged(const float* xproj, const float* U, float* h_out, float* gates, float* c_out,
                                    const int* lens, void* workspace, size_t workspace_bytes, int B, int T, int H,
                                    int ndir, int reverse, void* stream) {
    PTTS_REQUIRE(xproj && U && h_out && lens, "lstm_fwd_ragged: null tensor");
    PTTS_REQUIRE(B > 0 && T > 0 && H > 0 && (ndir == 1 || ndir == 2), "lstm_fwd_ragged: bad dims");
    PTTS_REQUIRE((size_t)LY * H * sizeof(float) <= 64 * 1024, "lstm_fwd_ragged: H=%d too large", H);
    const size_t cb = lstm_carry_bytes(B, H, ndir);
    if (!workspace || workspace_bytes < cb) {
        set_error("lstm_fwd_ragged: workspace %zu < %zu", workspace_bytes, cb);
        return PTTS_EWORKSPACE;
    }
    hipStream_t st = (hipStream_t)stream;
    float* carry = (float*)workspace;
    if (lstm_pk_ok(H) && workspace_bytes >= cb + ptts_lstm_fwd_workspace_bytes(B, T, H, ndir)) {
        float* Upk = (float*)((char*)workspace + cb);
        dim3 mgrid(H / 8, (B + 15) / 16, ndir);
        const int KS = H / 16;
        hipLaunchKernelGGL(lstm_pack_u_fwd_kernel, dim3(1024), dim3(256), 0, st, U, Upk, H, ndir);
        for (int s = 0; s < T; ++s) {
            if (KS % 16 == 0) hipLaunchKernelGGL(lstm_fwd_step_pk_kernel<16>, mgrid, dim3(256), 0, st, xproj, (const float*)Upk, h_out, gates, c_out, B, T, H, ndir, reverse, s, lens, carry);
            else if (KS % 8 == 0) hipLaunchKernelGGL(lstm_fwd_step_pk_kernel<8>, mgrid, dim3(256), 0, st, xproj, (const float*)Upk, h_out, gates, c_out, B, T, H, ndir, reverse, s, lens, carry);
            else hipLaunchKernelGGL(lstm_fwd_step_pk_kernel<4>, mgrid, dim3(256), 0, st, xproj, (const float*)Upk, h_out, gates, c_out, B, T, H, ndir, reverse, s, lens, carry);
        }
        return check_launch("lstm_fwd_ragged_pk");
    }
    if (H % 16 == 0) {
        dim3 mgrid(H / 8, (B + 15) / 16, ndir);
        for (int s = 0; s < T; ++s)
            hipLaunchKernelGGL(lstm_fwd_step_mfma_kernel, mgrid, dim3(256), 0, st, xproj, U, h_out, gates, c_out, B,
                               T, H, ndir, reverse, s, lens, carry);
        return check_launch("lstm_fwd_ragged_mfma");
    }
    dim3 grid((H + LX - 1) / LX, (B + LY - 1) / LY, ndir), block(LX, LY);
    const size_t lds = (size_t)LY * H * sizeof(float);
    for (int s = 0; s < T; ++s)
        hipLaunchKernelGGL(lstm_fwd_step_ragged_kernel, grid, block, lds, st, xproj, U, h_out, gates, c_out, B, T, H, ndir,
                           reverse, s, lens, carry);
    return check_launch("lstm_fwd_ragged");
}

extern "C" size_t ptts_lstm_bwd_workspace_bytes(int B, int T, int H, int ndir) {
    (void)T;
    return ((size_t)2 * ndir * 4 * H * H + (size_t)ndir * B * H) * sizeof(float);
}

// The launches of ptts_lstm_bwd; with rag = <const int* lens> those of ptts_lstm_bwd_ragged (the same paths, chosen the same way).
template <class... R>
static int lstm_bwd_run(const char* what, const float* dh_out, const float* U, const float* gates, const float* c_out,
                        float* dgates, void* workspace, size_t workspace_bytes, int B, int T, int H, int ndir,
                        int reverse, void* stream, R... rag) {
    PTTS_REQUIRE(dh_out && U && gates && c_out && dgates, "%s: null tensor", what);
    PTTS_REQUIRE(B > 0 && T > 0 && H > 0 && (ndir == 1 || ndir == 2), "%s: bad dims", what);
    PTTS_REQUIRE((size_t)LY * 4 * H * sizeof(float) <= 64 * 1024, "%s: H=%d too large", what, H);
    const size_t need = ptts_lstm_bwd_workspace_bytes(B, T, H, ndir);
    if (!workspace || workspace_bytes < need) {
        set_error("%s: workspace %zu < %zu", what, workspace_bytes, need);
        return PTTS_EWORKSPACE;
    }
    hipStream_t st = (hipStream_t)stream;
    float* UT = (float*)workspace;
    float* UTpk = UT + (size_t)ndir * 4 * H * H;
    float* dc_state = UTpk + (size_t)ndir * 4 * H * H;
    if (lstm_pk_ok(H)) {
        dim3 pgrid(H / 16, (B + 15) / 16, ndir);
        const bool w8 = H == 256;
        hipLaunchKernelGGL(lstm_pack_u_bwd_kernel, dim3(1024), dim3(256), 0, st, U, UTpk, H, ndir);
        for (int s = T - 1; s >= 0; --s)
            if (w8)
                hipLaunchKernelGGL((lstm_bwd_step_pk_kernel<8, R...>), pgrid, dim3(512), 0, st, dh_out,
                                   (const float*)UTpk, gates, c_out, dgates, dc_state, B, T, H, ndir, reverse, s, rag...);
            else
                hipLaunchKernelGGL((lstm_bwd_step_pk_kernel<4, R...>), pgrid, dim3(256), 0, st, dh_out,
                                   (const float*)UTpk, gates, c_out, dgates, dc_state, B, T, H, ndir, reverse, s, rag...);
        return check_launch(what);
    }
    const long long tot = (long long)ndir * 4 * H * H;
    int tb = (int)((tot + 255) / 256);
    if (tb > 2048) tb = 2048;
    hipLaunchKernelGGL(lstm_transpose_kernel, dim3(tb), dim3(256), 0, st, U, UT, H, ndir);
    dim3 grid((H + LX - 1) / LX, (B + LY - 1) / LY, ndir), block(LX, LY);
    const size_t lds = (size_t)LY * 4 * H * sizeof(float);
    if (H % 16 == 0) {
        dim3 mgrid(H / 16, (B + 15) / 16, ndir);
        for (int s = T - 1; s >= 0; --s)
            hipLaunchKernelGGL(lstm_bwd_step_mfma_kernel<R...>, mgrid, dim3(256), 0, st, dh_out, (const float*)UT, gates,
                               c_out, dgates, dc_state, B, T, H, ndir, reverse, s, rag...);
        return check_launch(what);
    }
    for (int s = T - 1; s >= 0; --s) {
        if constexpr (sizeof...(R) != 0)
            hipLaunchKernelGGL(lstm_bwd_step_ragged_kernel, grid, block, lds, st, dh_out, (const float*)UT, gates, c_out,
                               dgates, dc_state, B, T, H, ndir, reverse, s, rag...);
        else
            hipLaunchKernelGGL(lstm_bwd_step_kernel, grid, block, lds, st, dh_out, (const float*)UT, gates, c_out,
                               dgates, dc_state, B, T, H, ndir, reverse, s);
    }
    return check_launch(what);
}

extern "C" int ptts_lstm_bwd(const float* dh_out, const float* U, const float* gates, const float* c_out,
                             float* dgates, void* workspace, size_t workspace_bytes, int B, int T, int H, int ndir,
                             int reverse, void* stream) {
    return lstm_bwd_run("lstm_bwd", dh_out, U, gates, c_out, dgates, workspace, workspace_bytes, B, T, H, ndir, reverse, stream);
}

extern "C" int ptts_lstm_bwd_ragged(const float* dh_out, const float* U, const float* gates, const float* c_out,
                                    float* dgates, const int* lens, void* workspace, size_t workspace_bytes, int B, int T,
                                    int H, int ndir, int reverse, void* stream) {
    PTTS_REQUIRE(lens, "lstm_bwd_ragged: null lens");
    return lstm_bwd_run("lstm_bwd_ragged", dh_out, U, gates, c_out, dgates, workspace, workspace_bytes, B, T, H, ndir, reverse,
                        stream, lens);
}
