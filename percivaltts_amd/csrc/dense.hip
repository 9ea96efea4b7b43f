// Dense products C[M,N] = T(A)[M,K] . B[K,N] (+ bias) with M >> N on the bf16 matrix cores of gfx950, in fp32 arithmetic.
//
// Role on the hot path: every Dense layer of critic and generator (reference networktts.py:59-63, networks_critic.py:86-93,
// modeltts_common.py:77-79) -- forward, backward-data (B = W^T, with the LeakyReLU mask of the layer input fused into the
// store) and the masked forward of the gradient penalty's second-order sweep -- and the LSTM input projections
// (networktts.py:85-96).  The fp32-MFMA "tall" kernel of gemm.hip runs these at 71-77 TF, half of a pipe whose peak is 157;
// here the same sums run on v_mfma_f32_16x16x32_bf16 through the three-way bf16 split of BOTH operands (x = x1 + x2 + x3,
// xi = bf16(remainder), exact; the six products of order >= 2^-16 kept, fp32 accumulation: the arithmetic of split.hip and
// conv2d_mfma.hip, admitted as fp32 by the round-1 verdict).
//
// Operands.  The weights are split ONCE per update into three planes in MFMA-fragment order
//     planes[p][nt][ks][lane][8]:  n = 16 nt + (lane & 15),  k = 32 ks + 8 (lane >> 4) + e,   zero beyond N / K,
// so that a wave fetches a fragment with one coalesced 1-KB load straight from L2 into registers (no LDS, no transform).
// The activations stay fp32 in HBM; a workgroup stages TBM rows x 32 k per step, applies the pending transform of the
// producing layer (LeakyReLU, BatchNorm-affine + LeakyReLU, or the gradient-penalty mask), splits, and writes three bf16
// planes to the LDS (rows of 64 B, the four 16-byte quads XOR-swizzled by bit 2 of the row: conflict-free ds_read_b128).
//
// Tiling.  One workgroup (8 waves) owns TBM x 256 outputs -- all columns of a 256-wide block, so A is read once -- with
// TBM = 16 MT chosen to fill the CUs in whole rounds (M = 25 600 -> 112 -> 229 workgroups); wave w owns columns
// [32 w, 32 w + 32) x all MT row tiles.  The MFMA's first operand is the WEIGHT fragment and its second the activations,
// so a lane's accumulator holds four consecutive output columns of one row: 16-byte stores, no epilogue staging.
// Per k-step and wave: 3 MT ds_read_b128, 6 global 16-byte loads, 12 MT MFMAs.
#include "common.h"
#include <cstdlib>
#include <type_traits>

namespace ptts {
namespace dns {

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef unsigned u32x2 __attribute__((ext_vector_type(2)));
typedef unsigned short u16;

constexpr int THREADS = 512;
constexpr int NBLK = 256;          // columns per workgroup
constexpr int BK = 32;

#define DNS_PRODUCTS(X) X(2, 0) X(1, 1) X(0, 2) X(1, 0) X(0, 1) X(0, 0)
// NPL = 3: the six products of the fp32 split; NPL = 1 (ptts_set_bf16_products: BASELINE configs[2]): ONE product of the
// operands' bf16 roundings, fp32 accumulation
#define DNS_PRODUCTS_NPL(NPL, X) do { if (NPL == 3) { X(2, 0) X(1, 1) X(0, 2) X(1, 0) X(0, 1) } X(0, 0) } while (0)

__device__ __forceinline__ unsigned pk_bf16(float a, float b) {
    return __builtin_bit_cast(unsigned, __builtin_convertvector((f32x2){a, b}, bf16x2));
}
// x = h1 + h2 + h3, hi = bf16(remainder), round to nearest even (oracle.np_split3_bf16)
__device__ __forceinline__ void split3_pair(float a, float b, unsigned& p1, unsigned& p2, unsigned& p3) {
    p1 = pk_bf16(a, b);
    const float ra = a - __builtin_bit_cast(float, p1 << 16), rb = b - __builtin_bit_cast(float, p1 & 0xffff0000u);
    p2 = pk_bf16(ra, rb);
    const float sa = ra - __builtin_bit_cast(float, p2 << 16), sb = rb - __builtin_bit_cast(float, p2 & 0xffff0000u);
    p3 = pk_bf16(sa, sb);
}
__device__ __forceinline__ float max_fast(float a, float b) {
    float r;
    asm("v_max_f32 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
    return r;
}

// ------------------------------------------------------------------------------------------------------------
// weight planes.  transposed == 0: B[k][n] = w[k * ldw + n] (w stored [K][N]: the forward product);
//                 transposed == 1: B[k][n] = w[n * ldw + k] (w stored [N][K]: dX = dY . W^T reads W as it lies)
// ------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void split3_dense_weight_kernel(const float* __restrict__ w, long long ldw, int K, int N,
                                                                  int transposed, u16* __restrict__ planes, int NT, int KS) {
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;        // (nt, ks, lane)
    if (idx >= (long long)NT * KS * 64) return;
    const int lane = (int)(idx & 63);
    const long long t = idx >> 6;
    const int ks = (int)(t % KS), nt = (int)(t / KS);
    const int n = nt * 16 + (lane & 15), k0 = ks * 32 + (lane >> 4) * 8;
    float v[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        const int k = k0 + e;
        v[e] = (n < N && k < K) ? (transposed ? w[(long long)n * ldw + k] : w[(long long)k * ldw + n]) : 0.f;
    }
    unsigned q[3][4];
#pragma unroll
    for (int h = 0; h < 4; ++h) split3_pair(v[2 * h], v[2 * h + 1], q[0][h], q[1][h], q[2][h]);
    const size_t ps = (size_t)NT * KS * 512;
#pragma unroll
    for (int p = 0; p < 3; ++p)
        *reinterpret_cast<uint4*>(planes + p * ps + (size_t)idx * 8) = make_uint4(q[p][0], q[p][1], q[p][2], q[p][3]);
}

// the same for up to SPLIT_GROUP weights in one launch (blockIdx.y = weight): after an update every Dense kernel of a network needs its
// planes rebuilt (forward and transposed: 18 launches of 4 us per critic step, each with a launch boundary of its own)
constexpr int SPLIT_GROUP = 32;
struct SplitGroupArgs {
    const float* w[SPLIT_GROUP]; u16* planes[SPLIT_GROUP];
    long long ldw[SPLIT_GROUP];
    int K[SPLIT_GROUP], N[SPLIT_GROUP], transposed[SPLIT_GROUP], NT[SPLIT_GROUP], KS[SPLIT_GROUP];
    int rlo[SPLIT_GROUP], rhi[SPLIT_GROUP];       // rows k outside [rlo, rhi) are zero and never read (windows of a frame sequence)
};
__global__ __launch_bounds__(256) void split3_dense_weight_grouped_kernel(SplitGroupArgs a) {
    const int i = blockIdx.y;
    const int NT = a.NT[i], KS = a.KS[i], K = a.K[i], N = a.N[i], transposed = a.transposed[i];
    const int rlo = a.rlo[i], rhi = a.rhi[i];
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;        // (nt, ks, lane)
    if (idx >= (long long)NT * KS * 64) return;
    const float* __restrict__ w = a.w[i];
    u16* __restrict__ planes = a.planes[i];
    const long long ldw = a.ldw[i];
    const int lane = (int)(idx & 63);
    const long long t = idx >> 6;
    const int ks = (int)(t % KS), nt = (int)(t / KS);
    const int n = nt * 16 + (lane & 15), k0 = ks * 32 + (lane >> 4) * 8;
    float v[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        const int k = k0 + e;
        v[e] = (n < N && k < K && k >= rlo && k < rhi) ? (transposed ? w[(long long)n * ldw + k] : w[(long long)k * ldw + n]) : 0.f;
    }
    unsigned q[3][4];
#pragma unroll
    for (int h = 0; h < 4; ++h) split3_pair(v[2 * h], v[2 * h + 1], q[0][h], q[1][h], q[2][h]);
    const size_t ps = (size_t)NT * KS * 512;
#pragma unroll
    for (int p = 0; p < 3; ++p)
        *reinterpret_cast<uint4*>(planes + p * ps + (size_t)idx * 8) = make_uint4(q[p][0], q[p][1], q[p][2], q[p][3]);
}

// ---- frequency-domain context Conv1D: the kernel's transform, straight into the per-frequency planes ----------------------------
// B_f [2 Kh][N] = [Wr_f ; Wi_f],  W^_f[c][n] = sum_k w[k][c][n] e^{-2 pi i f (pl - k) / P}  (rows c < Cin of each half, the rest zero),
// written as the planes ptts_dense_bf16x6_batched reads for frequency f.  A lane owns one 16-byte fragment piece (8 consecutive rows
// of one column) for FCH frequencies: its 8 x KW taps stay in registers, a frequency costs 8 KW FMAs and one split.  (A GEMM with
// the twiddle matrix + a grouped split pass did the same in 0.35 ms per update: 263 MB of fp32 written, read again and split.)
constexpr int WDFT_FCH = 32;
template <int KW>
__global__ __launch_bounds__(256) void conv1d_wdft_planes_kernel(const float* __restrict__ w, const float* __restrict__ tw,
                                                                u16* __restrict__ planes, long long fstride, int NB, int Cin,
                                                                int N, int Kh, int NT, int KS) {
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;        // (nt, ks, lane)
    if (idx >= (long long)NT * KS * 64) return;
    const int lane = (int)(idx & 63);
    const long long t = idx >> 6;
    const int ks = (int)(t % KS), nt = (int)(t / KS);
    const int n = nt * 16 + (lane & 15), k0 = ks * 32 + (lane >> 4) * 8;
    const int part = k0 >= Kh ? 1 : 0, c0 = k0 - part * Kh;                 // Kh % 8 == 0: the 8 rows lie in one half
    float wr[KW][8];
#pragma unroll
    for (int k = 0; k < KW; ++k)
#pragma unroll
        for (int e = 0; e < 8; ++e)
            wr[k][e] = (n < N && c0 + e < Cin && k0 < 2 * Kh) ? w[((long long)k * Cin + c0 + e) * N + n] : 0.f;
    const size_t ps = (size_t)NT * KS * 512;
    const int f0 = blockIdx.y * WDFT_FCH;
    for (int f = f0; f < min(NB, f0 + WDFT_FCH); ++f) {
        const float* __restrict__ tr = tw + ((long long)f * 2 + part) * KW;
        float v[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int k = 0; k < KW; ++k) {
            const float c = tr[k];
#pragma unroll
            for (int e = 0; e < 8; ++e) v[e] = fmaf(c, wr[k][e], v[e]);
        }
        unsigned q[3][4];
#pragma unroll
        for (int h = 0; h < 4; ++h) split3_pair(v[2 * h], v[2 * h + 1], q[0][h], q[1][h], q[2][h]);
        u16* pf = planes + (long long)f * fstride;
#pragma unroll
        for (int p = 0; p < 3; ++p)
            *reinterpret_cast<uint4*>(pf + p * ps + (size_t)idx * 8) = make_uint4(q[p][0], q[p][1], q[p][2], q[p][3]);
    }
}

// ... and for matrices at REGULAR strides / windows of frame sequences (blockIdx.y = matrix, any number of them in one launch: the
// descriptor form above carries 32 per launch, and the frequency-domain Conv1D splits 256 at a time)
struct SplitStridedArgs {
    const float* w; u16* planes;
    long long stride_w, stride_p, ldw;            // floats, u16 elements, floats
    int K, N, transposed, NT, KS;
    int windows;                                  // 1: matrix z = (b, s) is the window x[b][row_off + s S + k][:] of a frame sequence
    int T, NS, S, row_off, kvalid;
};
__global__ __launch_bounds__(256) void split3_dense_weight_strided_kernel(SplitStridedArgs a) {
    const int z = blockIdx.y;
    const int NT = a.NT, KS = a.KS, K = a.K, N = a.N, transposed = a.transposed;
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;        // (nt, ks, lane)
    if (idx >= (long long)NT * KS * 64) return;
    const float* __restrict__ w;
    int rlo = 0, rhi = K;
    if (a.windows) {
        const int b = z / a.NS, sg = z - b * a.NS;
        const int r0 = a.row_off + sg * a.S;                                // source row of window row 0 (may be negative)
        w = a.w + ((long long)b * a.T + r0) * a.ldw;                        // (only rows inside [rlo, rhi) are dereferenced)
        rlo = r0 < 0 ? -r0 : 0;
        rhi = min(a.kvalid, a.T - r0);
    } else {
        w = a.w + (long long)z * a.stride_w;
    }
    u16* __restrict__ planes = a.planes + (long long)z * a.stride_p;
    const long long ldw = a.ldw;
    const int lane = (int)(idx & 63);
    const long long t = idx >> 6;
    const int ks = (int)(t % KS), nt = (int)(t / KS);
    const int n = nt * 16 + (lane & 15), k0 = ks * 32 + (lane >> 4) * 8;
    float v[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        const int k = k0 + e;
        v[e] = (n < N && k < K && k >= rlo && k < rhi) ? (transposed ? w[(long long)n * ldw + k] : w[(long long)k * ldw + n]) : 0.f;
    }
    unsigned q[3][4];
#pragma unroll
    for (int h = 0; h < 4; ++h) split3_pair(v[2 * h], v[2 * h + 1], q[0][h], q[1][h], q[2][h]);
    const size_t ps = (size_t)NT * KS * 512;
#pragma unroll
    for (int p = 0; p < 3; ++p)
        *reinterpret_cast<uint4*>(planes + p * ps + (size_t)idx * 8) = make_uint4(q[p][0], q[p][1], q[p][2], q[p][3]);
}

// The same planes for row-major matrices B[K][N] (not transposed, no windows) through the LDS: a workgroup takes the 32 k-rows of one
// k-step of one matrix, reads them as whole rows with 16-byte loads (a wave per row: 1 KB runs), and builds the fragments -- a lane's
// 8 consecutive k of ONE column -- out of the LDS.  The direct kernel above reads every value with a 4-byte load of its own (8 per lane,
// 256 B per wave and instruction): 38 us for the 32 MB of per-frequency products that the frequency-domain Conv1D hands to its inverse
// transform as the "weight" operand, 3 % of the loop's kernel time.  N % 4 == 0, ldw % 4 == 0, 16-byte aligned source.
constexpr int SPL_ROW = 256 + 2;         // floats per LDS row: rows 8 apart land 16 banks apart
__global__ __launch_bounds__(256) void split3_dense_weight_strided_lds_kernel(SplitStridedArgs a) {
    __shared__ float tile[32 * SPL_ROW];
    const int z = blockIdx.y, ks = blockIdx.x % a.KS, cb = blockIdx.x / a.KS;          // matrix, k-step, block of 256 columns
    const float* __restrict__ w = a.w + (long long)z * a.stride_w;
    u16* __restrict__ planes = a.planes + (long long)z * a.stride_p;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int n0 = cb * 256;
    // rows k = 32 ks + r: wave w loads rows w, w + 4, ...; lane: four columns
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const int r = wave + 4 * j, k = ks * 32 + r, n = n0 + 4 * lane;
        f32x4 v = {0.f, 0.f, 0.f, 0.f};
        if (k < a.K && n < a.N) v = *reinterpret_cast<const f32x4*>(w + (long long)k * a.ldw + n);
        float* d = tile + r * SPL_ROW + 4 * lane;
        d[0] = v[0]; d[1] = v[1]; d[2] = v[2]; d[3] = v[3];
    }
    __syncthreads();
    const size_t ps = (size_t)a.NT * a.KS * 512;
    const int li = lane & 15, lg = lane >> 4;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int ntl = wave + 4 * j;                                  // column tile inside the block: 0 .. 15
        const int nt = cb * 16 + ntl;
        if (nt >= a.NT) continue;
        float v[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) v[e] = tile[(8 * lg + e) * SPL_ROW + 16 * ntl + li];
        unsigned q[3][4];
#pragma unroll
        for (int h = 0; h < 4; ++h) split3_pair(v[2 * h], v[2 * h + 1], q[0][h], q[1][h], q[2][h]);
        const size_t idx = ((size_t)nt * a.KS + ks) * 64 + lane;
#pragma unroll
        for (int p = 0; p < 3; ++p)
            *reinterpret_cast<uint4*>(planes + p * ps + idx * 8) = make_uint4(q[p][0], q[p][1], q[p][2], q[p][3]);
    }
}

template <int B, int E, class F>
__device__ __forceinline__ void static_for(F&& f) {
    if constexpr (B < E) { f(std::integral_constant<int, B>{}); static_for<B + 1, E>(f); }
}
// ---- The staging of one 32-row slab of both operands (commit below) cut into ISSUE SLICES of at most two 4-cycle vector slots, so that
// the k-loop can put one slice behind each of the issuing wave's own MFMAs: a v_mfma_f32_16x16x32_bf16 holds the SIMD's vector issue for 8
// of its 16 cycles, the other 8 take two VALU / LDS instructions (a conversion counts as two) for nearly nothing -- and vector work of the
// OTHER wave of the SIMD does not run under this wave's MFMAs, which is what the stagger of waves 0-3 / 4-7 relied on.
// A lane's four quads (A rows j = 0, 1; dY rows j = 0, 1) are eight chains of two values, chain c = 2 quad + pair; a chain's operations
// in order: [scale] [shift] zero-select [transform: two operations] [bias sum], then split3_pair's seven (convert, widen, subtract,
// convert, widen, subtract, convert).  The slices run level by level over the chains (eight independent chains side by side), and a
// quad's LDS write of plane p follows the slice that finished the plane's second pair.  The arithmetic and its order per value, and the
// order of the bias sums, are commit's.
enum : int { SL_AFM, SL_AFA, SL_SEL, SL_M1, SL_M2, SL_BS, SL_C1, SL_B1, SL_S1, SL_C2, SL_B2, SL_S2, SL_C3, SL_W };
struct SliceTab { int n; int op[128], who[128], plane[128]; };      // who: the chain, for SL_W the quad
template <int MODE, bool AFFINE, bool BSUM, int NQA, int NQD>
constexpr SliceTab make_slices() {
    SliceTab t{};
    int ops[8][16] = {}, len[8] = {};
    for (int c = 0; c < 2 * (NQA + NQD); ++c) {
        const bool is_a = c < 2 * NQA;
        int n = 0;
        if (is_a && AFFINE) { ops[c][n++] = SL_AFM; ops[c][n++] = SL_AFA; }
        ops[c][n++] = SL_SEL;
        if (is_a && MODE != PTTS_IN_NONE) { ops[c][n++] = SL_M1; ops[c][n++] = SL_M2; }
        if (!is_a && BSUM) ops[c][n++] = SL_BS;
        for (int o = SL_C1; o <= SL_C3; ++o) ops[c][n++] = o;
        len[c] = n;
    }
    int done[8] = {}, written[4] = {};
    for (int l = 0; l < 16; ++l)
        for (int c = 0; c < 2 * (NQA + NQD); ++c) {
            if (l >= len[c]) continue;
            const int o = ops[c][l], q = c >> 1;
            t.op[t.n] = o; t.who[t.n] = c; t.plane[t.n] = 0; ++t.n;
            if (o == SL_C1 || o == SL_C2 || o == SL_C3) ++done[c];
            while (written[q] < (done[2 * q] < done[2 * q + 1] ? done[2 * q] : done[2 * q + 1])) {
                t.op[t.n] = SL_W; t.who[t.n] = q; t.plane[t.n] = written[q]++; ++t.n;
            }
        }
    return t;
}
// NQA quads with the input transform (A), then NQD without (dY); dense_bf16x6_kernel stages NA quads of A alone
template <int MODE, bool AFFINE, bool BSUM, int PLSTRIDE, int NQA = 2, int NQD = 2>
struct StageSlices {
    static constexpr SliceTab TAB = make_slices<MODE, AFFINE, BSUM, NQA, NQD>();
    static constexpr int N = TAB.n;
    f32x2 x[8], y[8], mk[4];         // per chain: its two values, a temporary, the mask source's two values
    unsigned pk[3][8];               // [plane][chain]: a quad's two chains side by side, as its LDS write takes them
    bool ok[4];                      // per quad: its row and its columns are inside
    u16* dst[4];                     // per quad: its 8 bytes of plane 0
    f32x4 sc, sh;
    float alpha;
    // quads: va[0], va[1], vd[0], vd[1] (vm: the mask source of va)
    __device__ __forceinline__ void begin(const f32x4* va, const f32x4* vm, const f32x4* vd) {
#pragma unroll
        for (int c = 0; c < 2 * (NQA + NQD); ++c) {
            const int q = c >> 1, e = 2 * (c & 1);
            const f32x4 v = q < NQA ? va[q < NQA ? q : 0] : vd[q < NQA ? 0 : q - NQA];
            x[c] = (f32x2){v[e], v[e + 1]};
            if (MODE == PTTS_IN_MASKMUL && q < NQA) mk[c & 3] = (f32x2){vm[q < NQA ? q : 0][e], vm[q < NQA ? q : 0][e + 1]};
        }
    }
    template <int I>
    __device__ __forceinline__ void run(f32x4& bsum) {
        if constexpr (I < N) {
            constexpr int op = TAB.op[I], c = TAB.who[I], e = 2 * (c & 1);
            if constexpr (op == SL_AFM) { x[c] = x[c] * (f32x2){sc[e], sc[e + 1]}; }
            else if constexpr (op == SL_AFA) { x[c] = x[c] + (f32x2){sh[e], sh[e + 1]}; }
            else if constexpr (op == SL_SEL) { x[c] = (f32x2){ok[c >> 1] ? x[c][0] : 0.f, ok[c >> 1] ? x[c][1] : 0.f}; }
            else if constexpr (op == SL_M1) {
                if (MODE == PTTS_IN_LRELU) y[c] = (f32x2){alpha * x[c][0], alpha * x[c][1]};
                else y[c] = (f32x2){mk[c & 3][0] > 0.f ? 1.f : alpha, mk[c & 3][1] > 0.f ? 1.f : alpha};
            } else if constexpr (op == SL_M2) {
                if (MODE == PTTS_IN_LRELU) x[c] = (f32x2){max_fast(x[c][0], y[c][0]), max_fast(x[c][1], y[c][1])};
                else x[c] = (f32x2){x[c][0] * y[c][0], x[c][1] * y[c][1]};
            } else if constexpr (op == SL_BS) { bsum[e] += x[c][0]; bsum[e + 1] += x[c][1]; }
            else if constexpr (op == SL_C1 || op == SL_C2 || op == SL_C3) {
                pk[(op - SL_C1) / 3][c] = __builtin_bit_cast(unsigned, __builtin_convertvector(x[c], bf16x2));
            } else if constexpr (op == SL_B1 || op == SL_B2) {
                const unsigned p = pk[(op - SL_B1) / 3][c];
                y[c] = (f32x2){__builtin_bit_cast(float, p << 16), __builtin_bit_cast(float, p & 0xffff0000u)};
            } else if constexpr (op == SL_S1 || op == SL_S2) { x[c] = x[c] - y[c]; }
            else {                                                      // SL_W: c is the quad
                constexpr int p = TAB.plane[I];
                *reinterpret_cast<u32x2*>(dst[c] + p * PLSTRIDE) = (u32x2){pk[p][2 * c], pk[p][2 * c + 1]};
            }
        }
    }
};

// DNS_PRODUCTS' order as tables: product pr multiplies plane prod_pa(pr) of the staged (activation) operand with plane prod_pw(pr) of the other
constexpr int prod_pa(int pr) { constexpr int t[6] = {2, 1, 0, 1, 0, 0}; return t[pr]; }
constexpr int prod_pw(int pr) { constexpr int t[6] = {0, 1, 2, 0, 1, 0}; return t[pr]; }

#ifndef DNS_DEPTH
#define DNS_DEPTH 2        // register stages of the A operand in dense_bf16x6_kernel (1 = the single stage of rounds 2-3; measured 1 / 2 / 3 / 4 / 6:
                           // 25.6 / 25.0 / 25.6 / 26.5 / 29.8 us at 25 600 rows, 82.4 / 75.3 / 80.3 / 83.0 / 86.0 at 76 800: the loads are not what bounds it)
#endif
#ifndef DNS_SKIP_DEAD
#define DNS_SKIP_DEAD 1    // a wave whose columns lie beyond N runs the staging-only loop (0: the MFMAs of the first tile as well, as before)
#endif
struct DenseArgs {
    const float* A; const float* mask_src; const float* in_scale; const float* in_shift;
    const u16* planes; const float* bias; const float* out_mask; float* C;
    int M, N, K, NT, KS;
    long long lda, ldc;
    float alpha, out_alpha;
    int accumulate, has_affine, vec_out;
    const float* res; int res_rows; long long ldr;      // residual added in the store: C[m][n] += res[m % res_rows][n] (NULL: none).  accumulate = res == C
    long long bsA, bsP, bsC;          // batched launch (gridDim.z products of one shape): strides of A and C in floats, of the planes in u16
    double* stats;                    // (ptts_dense_bf16x6_stats) per row tile: the column sums and the column sums of squares of what is stored, [gridDim.x][2 N]
    const float* om_scale; const float* om_shift;     // (ptts_dense_bf16x6_bwd_affine) out_mask holds z of a BatchNorm-affine + LeakyReLU input: see the store
};

// XT: the launch has floor(N / 256) column blocks and the LAST one also owns the 1..16 columns beyond them, as a 17th column tile
// (nt = 16 of the block: the planes are laid out for 256 more columns anyway).  Its MT row tiles are dealt over the waves -- wave w
// multiplies row tile w -- so a wave's k-step grows by one accumulator, three weight-fragment loads, three ds_read_b128 and six
// MFMAs (12 MT + 6: + 6 % at MT = 8) instead of a second column block of full price or a second pass over A by a thin kernel.
template <int MODE, bool AFFINE, int MT, int NPL, bool XT = false>
__global__ __launch_bounds__(THREADS) void dense_bf16x6_kernel(DenseArgs g) {
    if (gridDim.z > 1) {
        g.A += (long long)blockIdx.z * g.bsA;
        g.planes += (long long)blockIdx.z * g.bsP;
        g.C += (long long)blockIdx.z * g.bsC;
    }
    constexpr int TBM = 16 * MT;
    constexpr int NA = (TBM * 8 + THREADS - 1) / THREADS;     // 16-byte quads (4 k) per lane and k-step
    constexpr int ROWS = NA * THREADS / 8;                    // staged rows incl. the pad rows the idle lanes of the last slot write
    constexpr int PL = ROWS * BK;                             // elements of one plane of a stage
    constexpr bool MASK = MODE == PTTS_IN_MASKMUL;
    __shared__ __attribute__((aligned(16))) u16 As[2][NPL * PL];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int li = lane & 15, lg = lane >> 4;
    const int m0 = blockIdx.x * TBM, n0 = blockIdx.y * NBLK;
    const int KS = g.KS;
    const bool wave_live = n0 + 32 * wave < g.N;              // a wave whose columns lie beyond N only stages
    const bool xt_wave = XT && blockIdx.y == gridDim.y - 1 && wave < MT;      // this wave multiplies row tile `wave` of the extra tile

    // ---- this lane's staging slots: quad q = tid + 512 j -> row q >> 3, k-quad q & 7 (the same for every j).  No branches
    // in the k-loop: rows beyond the tile or M read row 0 and are zeroed by a select, and so are the quads beyond K.
    const int kq = tid & 7;
    const float* pa[NA]; const float* pm[NA]; bool oka[NA]; int dst[NA];
#pragma unroll
    for (int j = 0; j < NA; ++j) {
        const int row = (tid + j * THREADS) >> 3;
        oka[j] = row < TBM && m0 + row < g.M;
        const long long base = (long long)(oka[j] ? m0 + row : 0) * g.lda + 4 * kq;
        pa[j] = g.A + base;
        pm[j] = MASK ? g.mask_src + base : nullptr;
        dst[j] = row * BK + ((((kq >> 1) ^ ((row >> 1) & 2))) << 3) + (kq & 1) * 4;
    }
    struct Stage { f32x4 va[NA], vm[MASK ? NA : 1], sc, sh; bool kok; };
    auto load_a = [&](int s, Stage& sg) {
        const int k = s * BK + 4 * kq;
        sg.kok = k < g.K;                                     // K % 4 == 0: a quad is all inside or all outside
        const int ko = sg.kok ? s * BK : -4 * kq;             // (outside: the row's first quad, discarded)
#pragma unroll
        for (int j = 0; j < NA; ++j) {
            sg.va[j] = *reinterpret_cast<const f32x4*>(pa[j] + ko);
            if (MASK) sg.vm[j] = *reinterpret_cast<const f32x4*>(pm[j] + ko);
        }
        if (AFFINE) {
            sg.sc = *reinterpret_cast<const f32x4*>(g.in_scale + (sg.kok ? k : 0));
            sg.sh = *reinterpret_cast<const f32x4*>(g.in_shift + (sg.kok ? k : 0));
        }
    };
    auto commit = [&](const Stage& sg, u16* as) {
        const f32x4 z4 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int j = 0; j < NA; ++j) {
            f32x4 a = sg.va[j];
            if (MODE == PTTS_IN_LRELU) {
                if (AFFINE) a = a * sg.sc + sg.sh;
                if (!(oka[j] && sg.kok)) a = z4;
#pragma unroll
                for (int e = 0; e < 4; ++e) a[e] = max_fast(a[e], g.alpha * a[e]);
            } else if (MASK) {
                if (!(oka[j] && sg.kok)) a = z4;
#pragma unroll
                for (int e = 0; e < 4; ++e) a[e] = a[e] * (sg.vm[j][e] > 0.f ? 1.f : g.alpha);
            } else {
                if (!(oka[j] && sg.kok)) a = z4;
            }
            u16* d = as + dst[j];
            if (NPL == 3) {
                unsigned a1, a2, a3, b1, b2, b3;
                split3_pair(a[0], a[1], a1, a2, a3);
                split3_pair(a[2], a[3], b1, b2, b3);
                *reinterpret_cast<u32x2*>(d) = (u32x2){a1, b1};
                *reinterpret_cast<u32x2*>(d + PL) = (u32x2){a2, b2};
                *reinterpret_cast<u32x2*>(d + 2 * PL) = (u32x2){a3, b3};
            } else {
                *reinterpret_cast<u32x2*>(d) = (u32x2){pk_bf16(a[0], a[1]), pk_bf16(a[2], a[3])};      // the one rounding of bf16 products
            }
        }
    };

    // ---- weight fragments of this wave's two column tiles, straight from global memory
    const size_t ps = (size_t)g.NT * KS * 512;
    const u16* wp[2];
#pragma unroll
    for (int j = 0; j < 2; ++j) wp[j] = g.planes + (((size_t)((n0 >> 4) + 2 * (wave_live ? wave : 0) + j) * KS) * 64 + lane) * 8;
    auto load_w = [&](int s, bf16x8 (&wf)[2][NPL]) {
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int p = 0; p < NPL; ++p) wf[j][p] = *reinterpret_cast<const bf16x8*>(wp[j] + p * ps + (size_t)s * 512);
    };
    // ... and of the extra tile.  No branch in the k-loop: a wave without a share of it loads the block's first tile and drops it.
    const u16* wpx = g.planes + (((size_t)((n0 >> 4) + (xt_wave ? NBLK / 16 : 0)) * KS) * 64 + lane) * 8;
    auto load_wx = [&](int s, bf16x8 (&wf)[NPL]) {
#pragma unroll
        for (int p = 0; p < NPL; ++p) wf[p] = *reinterpret_cast<const bf16x8*>(wpx + p * ps + (size_t)s * 512);
    };

    f32x4 acc[MT][2];
#pragma unroll
    for (int i = 0; i < MT; ++i) { acc[i][0] = f32x4{0.f, 0.f, 0.f, 0.f}; acc[i][1] = f32x4{0.f, 0.f, 0.f, 0.f}; }
    // activation fragment of row tile i: row 16 i + li, quad lg (swizzle = bit 2 of li), plane p: + p PL
    const int boff = li * BK + ((lg ^ ((li >> 1) & 2)) << 3);
    auto mfma_rows = [&](const u16* as, const bf16x8 (&wf)[2][NPL], int i0, int i1) {
#pragma unroll
        for (int i = i0; i < i1; ++i) {
            bf16x8 bf[NPL];
#pragma unroll
            for (int p = 0; p < NPL; ++p) bf[p] = *reinterpret_cast<const bf16x8*>(as + p * PL + boff + i * 16 * BK);
#define DNS_MM(PA, PW)                                                                                    \
            acc[i][0] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf[0][PW < NPL ? PW : 0], bf[PA < NPL ? PA : 0], acc[i][0], 0, 0, 0);    \
            acc[i][1] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf[1][PW < NPL ? PW : 0], bf[PA < NPL ? PA : 0], acc[i][1], 0, 0, 0);
            DNS_PRODUCTS_NPL(NPL, DNS_MM);
#undef DNS_MM
        }
    };

    // extra tile: activation fragments of row tile `wave` (read once more, in the k-step's main block: reusing those of mfma_rows would
    // put a wave-dependent branch into every row tile of it); the six products in the order of the main tiles
    f32x4 accx = {0.f, 0.f, 0.f, 0.f};
    const int xoff = boff + (wave < MT ? wave : MT - 1) * 16 * BK;
    auto read_x = [&](const u16* as, bf16x8 (&bf)[NPL]) {
#pragma unroll
        for (int p = 0; p < NPL; ++p) bf[p] = *reinterpret_cast<const bf16x8*>(as + p * PL + xoff);
    };
    auto mfma_x = [&](const bf16x8 (&wf)[NPL], const bf16x8 (&bf)[NPL]) {
#define DNS_MM(PA, PW) accx = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf[PW < NPL ? PW : 0], bf[PA < NPL ? PA : 0], accx, 0, 0, 0);
        DNS_PRODUCTS_NPL(NPL, DNS_MM);
#undef DNS_MM
    };

    // One basic block per k-step: the staging of step s+1 (transform, split, LDS stores into the other buffer) and the loads
    // of step s+2 sit between the MFMAs of step s.  (A wave whose columns lie beyond N stages its share and meets the same
    // barriers in a loop of its own, run_dead, without weight loads and MFMAs: the SIMD's matrix time is the sum of what its two waves
    // issue, so those MFMAs were paid for by the live wave beside it.)
    // DEPTH register stages of A: the loads of k-step s + DEPTH are issued while step s is multiplied.  The kernel's time is linear in M
    // from 25 600 rows up (tools/dense_ramp_probe.py: 1.0 us per 1000 rows, 130 TF) and hardly moves with DEPTH: what bounds a k-step is
    // the matrix pipe -- TWO waves per SIMD x 84 six-product MFMAs x 16 cycles = 2 700 cycles at the ~1.8 GHz it holds under that load.
    constexpr int DEPTH = DNS_DEPTH;
    constexpr bool OWN_GAPS = NPL == 3;                       // (one plane: 2 MT MFMAs per step, the k-step above)
    Stage sg[DEPTH];
    bf16x8 wc[2][NPL], wn[2][NPL];
    bf16x8 wx[XT ? NPL : 1];                                  // (no second stage: loaded at the head of its k-step, used at its end)
#pragma unroll
    for (int j = 0; j < DEPTH; ++j) load_a(j, sg[j]);
    load_w(0, wc);
    commit(sg[0], As[0]);
    load_a(DEPTH, sg[0]);
    __syncthreads();
    // The two waves of a SIMD leave every barrier together; with the staging at the same place of their instruction streams
    // both would do vector work at the same time and leave the matrix pipe idle.  Waves 0-3 (one per SIMD) stage after two
    // row tiles, waves 4-7 after MT - 2.
    auto step = [&](int s, int cut, Stage& nx) {             // nx: the stage that holds step s + 1 (slot (s + 1) % DEPTH), refilled with step s + 1 + DEPTH
        const u16* as = As[s & 1];
        load_w(s + 1 < KS ? s + 1 : s, wn);
        if constexpr (XT) load_wx(s, wx);
        mfma_rows(as, wc, 0, cut);
        commit(nx, As[(s + 1) & 1]);                          // the other buffer: every wave left it at the last barrier
        load_a(s + 1 + DEPTH, nx);
        bf16x8 bx[XT ? NPL : 1];
        if constexpr (XT) read_x(as, bx);
        mfma_rows(as, wc, cut, MT);
        if constexpr (XT) {
            if (xt_wave) mfma_x(wx, bx);                      // (wave-uniform, in front of the barrier and not around it)
        }
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int p = 0; p < NPL; ++p) wc[j][p] = wn[j][p];
        __syncthreads();
    };
    // Three planes: the same k-step with everything but the MFMAs in this wave's OWN MFMA gaps (StageSlices), the same
    // in every wave.  Row tile i's three fragments are read in the first three gaps of tile i - 1 (two register sets), every other gap
    // takes one slice of the staging of step s + 1; the weight loads of step s + 1 and the A loads of step s + 1 + DEPTH go out in front
    // of the first MFMA, under the latency of tile 0's fragment reads; slices that are left run behind the last MFMA.
    // (wcur / wnext: the weight fragments of this step and the registers the next step's are loaded into -- the caller swaps them, no copy)
    auto step_own = [&](int s, Stage& nx, const bf16x8 (&wcur)[2][NPL], bf16x8 (&wnext)[2][NPL]) __attribute__((always_inline)) {
        if constexpr (NPL == 3) {
            using ST = StageSlices<MODE, AFFINE, false, PL, NA, 0>;
            constexpr int NM = 12 * MT, NR = 3 * (MT - 1);           // MFMAs; fragment reads that stand in gaps
            const u16* as = As[s & 1];
            u16* an = As[(s + 1) & 1];                                // the other buffer: every wave left it at the last barrier
            ST st;
            st.begin(nx.va, nx.vm, nx.va);
#pragma unroll
            for (int j = 0; j < NA; ++j) { st.ok[j] = oka[j] && nx.kok; st.dst[j] = an + dst[j]; }
            st.sc = nx.sc; st.sh = nx.sh; st.alpha = g.alpha;
            f32x4 none = {0.f, 0.f, 0.f, 0.f};
            bf16x8 bf[2][NPL];
            auto read = [&](auto I, auto P) {
                constexpr int i = decltype(I)::value, p = decltype(P)::value;
                bf[i & 1][p] = *reinterpret_cast<const bf16x8*>(as + p * PL + boff + i * 16 * BK);
            };
            static_for<0, 3>([&](auto P) { read(std::integral_constant<int, 0>{}, P); });
            load_w(s + 1 < KS ? s + 1 : s, wnext);
            if constexpr (XT) load_wx(s, wx);
            load_a(s + 1 + DEPTH, nx);
            __builtin_amdgcn_sched_barrier(0);
            static_for<0, NM>([&](auto Q) {
                constexpr int q = decltype(Q)::value, i = q / 12, r = q % 12, pr = r / 2, j = r % 2;
                acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wcur[j][prod_pw(pr)], bf[i & 1][prod_pa(pr)], acc[i][j], 0, 0, 0);
                if constexpr (i + 1 < MT && r < 3) read(std::integral_constant<int, i + 1>{}, std::integral_constant<int, r>{});
                else st.template run<q - (i + 1 < MT ? 3 * i + 3 : NR)>(none);
                __builtin_amdgcn_sched_barrier(0);
            });
            static_for<NM - NR, ST::N>([&](auto I) { st.template run<decltype(I)::value>(none); });
            if constexpr (XT) {
                if (xt_wave) {                                        // (wave-uniform, in front of the barrier and not around it)
                    bf16x8 bx[NPL];
                    read_x(as, bx);
                    mfma_x(wx, bx);
                }
            }
            __syncthreads();
        }
    };
    auto step_dead = [&](int s, Stage& nx) {                  // the staging and the barrier of `step`, nothing else
        commit(nx, As[(s + 1) & 1]);
        load_a(s + 1 + DEPTH, nx);
        __syncthreads();
    };
    auto run = [&](int cut) {
        int s = 0;
        for (; s + DEPTH <= KS; s += DEPTH) {                 // (s % DEPTH == 0: the stage indices are compile-time)
#pragma unroll
            for (int j = 0; j < DEPTH; ++j) step(s + j, cut, sg[(j + 1) % DEPTH]);
        }
#pragma unroll
        for (int j = 0; j < DEPTH; ++j)
            if (s + j < KS) step(s + j, cut, sg[(j + 1) % DEPTH]);
    };
    auto run_own = [&]() {                                   // two steps per trip: wc and wn change places
        static_assert(!OWN_GAPS || DEPTH == 2, "run_own swaps the weight registers over a trip of two steps");
        int s = 0;
        for (; s + 2 <= KS; s += 2) { step_own(s, sg[1], wc, wn); step_own(s + 1, sg[0], wn, wc); }
        if (s < KS) step_own(s, sg[1], wc, wn);
    };
    auto run_dead = [&]() {
        int s = 0;
        for (; s + DEPTH <= KS; s += DEPTH) {
#pragma unroll
            for (int j = 0; j < DEPTH; ++j) step_dead(s + j, sg[(j + 1) % DEPTH]);
        }
#pragma unroll
        for (int j = 0; j < DEPTH; ++j)
            if (s + j < KS) step_dead(s + j, sg[(j + 1) % DEPTH]);
    };
    if (DNS_SKIP_DEAD && !XT && !wave_live) run_dead();       // (XT: every column block is full)
    else if (OWN_GAPS) run_own();
    else if (wave < 4) run(2); else run(MT - 2);
    if constexpr (XT) {
        // ---- store of the extra tile: lane (li, lg) of accx holds row m0 + 16 wave + li, columns n0 + 256 + 4 lg .. + 3
        const int m = m0 + 16 * wave + li, n = n0 + NBLK + 4 * lg;
        if (xt_wave && m < g.M && n < g.N) {
            const long long off = (long long)m * g.ldc + n;
            int mr = m; while (g.res && mr >= g.res_rows) mr -= g.res_rows;
            if (g.vec_out) {                                  // N % 4 == 0: the four columns are inside or outside together
                f32x4 v = accx;
                if (g.bias) v += *reinterpret_cast<const f32x4*>(g.bias + n);
                if (g.out_mask) {
                    const f32x4 mk = *reinterpret_cast<const f32x4*>(g.out_mask + off);
#pragma unroll
                    for (int e = 0; e < 4; ++e) v[e] = v[e] * (mk[e] > 0.f ? 1.f : g.out_alpha);
                }
                if (g.res) v += *reinterpret_cast<const f32x4*>(g.res + (long long)mr * g.ldr + n);
                *reinterpret_cast<f32x4*>(g.C + off) = v;
            } else {
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    if (n + e >= g.N) continue;
                    float v = accx[e] + (g.bias ? g.bias[n + e] : 0.f);
                    if (g.out_mask) v *= g.out_mask[off + e] > 0.f ? 1.f : g.out_alpha;
                    if (g.res) v += g.res[(long long)mr * g.ldr + n + e];
                    g.C[off + e] = v;
                }
            }
        }
    }
    if (!wave_live) return;
    // ---- store: lane (li, lg) of acc[i][j] holds row m0 + 16 i + li, columns n0 + 32 wave + 16 j + 4 lg .. + 3
    const bool interior = m0 + TBM <= g.M;                    // no row guards: the mask / old-value loads go out together
    if (!g.vec_out) {
        // N or ldc no multiple of 4 (the 65-bin spectral head): element-wise stores
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int i = 0; i < MT; ++i) {
                const int m = m0 + 16 * i + li;
                if (m >= g.M) continue;
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const int n = n0 + 32 * wave + 16 * j + 4 * lg + e;
                    if (n >= g.N) continue;
                    const long long off = (long long)m * g.ldc + n;
                    float v = acc[i][j][e] + (g.bias ? g.bias[n] : 0.f);
                    if (g.out_mask) v *= g.out_mask[off] > 0.f ? 1.f : g.out_alpha;
                    if (g.res) { int mr = m; while (mr >= g.res_rows) mr -= g.res_rows; v += g.res[(long long)mr * g.ldr + n]; }
                    g.C[off] = v;
                }
            }
        return;
    }
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int n = n0 + 32 * wave + 16 * j + 4 * lg;
        if (n >= g.N) continue;                               // N % 4 == 0
        f32x4 bv = {0.f, 0.f, 0.f, 0.f};
        if (g.bias) bv = *reinterpret_cast<const f32x4*>(g.bias + n);
        const long long off0 = (long long)(m0 + li) * g.ldc + n;
        // row of the residual: m modulo res_rows (a product shared by k stacked evaluations is added to each of its k row blocks)
        auto res_at = [&](int m) { int mr = m; while (mr >= g.res_rows) mr -= g.res_rows; return g.res + (long long)mr * g.ldr + n; };
        f32x4 ssum = {0.f, 0.f, 0.f, 0.f}, ssq = {0.f, 0.f, 0.f, 0.f};
        // ptts_dense_bf16x6_bwd_affine: the product is da = dy . W^T of a layer whose input was lrelu(sc z + sh), z = out_mask.  What is
        // stored is dz = da lrelu'(sc z + sh) sc; the tile's column sums are those of da lrelu'(.) z (ssum: the affine's dscale) and of
        // da lrelu'(.) (ssq: its dshift) -- ptts_affine_act_bwd's arithmetic, without its pass over da and z
        f32x4 osc = {1.f, 1.f, 1.f, 1.f}, osh = {0.f, 0.f, 0.f, 0.f};
        if (g.om_scale) { osc = *reinterpret_cast<const f32x4*>(g.om_scale + n); osh = *reinterpret_cast<const f32x4*>(g.om_shift + n); }
        auto aff_store = [&](f32x4& v, const f32x4& z) {
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const float gd = v[e] * ((z[e] * osc[e] + osh[e]) > 0.f ? 1.f : g.out_alpha);
                ssum[e] += gd * z[e]; ssq[e] += gd;
                v[e] = gd * osc[e];
            }
        };
        if (interior) {
            f32x4 mk[MT], old[MT];
            if (g.out_mask) {
#pragma unroll
                for (int i = 0; i < MT; ++i) mk[i] = *reinterpret_cast<const f32x4*>(g.out_mask + off0 + (long long)16 * i * g.ldc);
            }
            if (g.res) {
#pragma unroll
                for (int i = 0; i < MT; ++i) old[i] = *reinterpret_cast<const f32x4*>(res_at(m0 + 16 * i + li));
            }
#pragma unroll
            for (int i = 0; i < MT; ++i) {
                f32x4 v = acc[i][j] + bv;
                if (g.om_scale) {
                    aff_store(v, mk[i]);
                } else if (g.out_mask) {
#pragma unroll
                    for (int e = 0; e < 4; ++e) v[e] = v[e] * (mk[i][e] > 0.f ? 1.f : g.out_alpha);
                }
                if (g.res) v += old[i];
                if (g.stats && !g.om_scale) { ssum += v; ssq += v * v; }
                *reinterpret_cast<f32x4*>(g.C + off0 + (long long)16 * i * g.ldc) = v;
            }
        } else {
#pragma unroll
            for (int i = 0; i < MT; ++i) {
                const int m = m0 + 16 * i + li;
                if (m >= g.M) continue;
                const long long off = off0 + (long long)16 * i * g.ldc;
                f32x4 v = acc[i][j] + bv;
                if (g.out_mask) {
                    const f32x4 mk = *reinterpret_cast<const f32x4*>(g.out_mask + off);
                    if (g.om_scale) {
                        aff_store(v, mk);
                    } else {
#pragma unroll
                        for (int e = 0; e < 4; ++e) v[e] = v[e] * (mk[e] > 0.f ? 1.f : g.out_alpha);
                    }
                }
                if (g.res) v += *reinterpret_cast<const f32x4*>(res_at(m));
                if (g.stats && !g.om_scale) { ssum += v; ssq += v * v; }
                *reinterpret_cast<f32x4*>(g.C + off) = v;
            }
        }
        if (g.stats) {
            // the tile's column sums: a lane holds MT of the TBM rows of its four columns; the 16 lanes li of a group hold the others
#pragma unroll
            for (int e = 0; e < 4; ++e)
#pragma unroll
                for (int m = 1; m < 16; m <<= 1) { ssum[e] += __shfl_xor(ssum[e], m, 64); ssq[e] += __shfl_xor(ssq[e], m, 64); }
            if (li == 0) {
                double* row = g.stats + (size_t)blockIdx.x * 2 * g.N;
#pragma unroll
                for (int e = 0; e < 4; ++e) { row[n + e] = (double)ssum[e]; row[g.N + n + e] = (double)ssq[e]; }
            }
        }
    }
}

// The extra-tile form exists for MT <= 7: at MT = 8 and three planes its registers no longer fit (the compiler answers with a kernel
// that keeps its stages in scratch memory).
template <int MODE, bool AFFINE, int MT, int NPL>
static void dense_launch_kernel(bool xt, dim3 grid, hipStream_t st, const DenseArgs& g) {
    if constexpr (MT < 8) {
        if (xt) { hipLaunchKernelGGL((dense_bf16x6_kernel<MODE, AFFINE, MT, NPL, true>), grid, dim3(THREADS), 0, st, g); return; }
    }
    hipLaunchKernelGGL((dense_bf16x6_kernel<MODE, AFFINE, MT, NPL>), grid, dim3(THREADS), 0, st, g);
}

// rows per workgroup (multiple of 16, 64..128) that best fills 256 CUs in whole rounds
static int pick_mt(int M, int col_blocks) {
    static int forced = -1;
    if (forced < 0) { const char* e = getenv("PTTS_DENSE_MT"); forced = e ? atoi(e) : 0; }
    if (forced >= 4 && forced <= 8) return forced;
    int best = 8; double best_eff = -1.0;
    for (int mt = 4; mt <= 8; ++mt) {
        const long long blocks = (long long)((M + 16 * mt - 1) / (16 * mt)) * col_blocks;
        const long long rounds = (blocks + 255) / 256;
        const double eff = (double)M * col_blocks / (double)(rounds * 256 * 16 * mt);
        if (eff > best_eff + 1e-9) { best_eff = eff; best = mt; }
    }
    return best;
}

// ------------------------------------------------------------------------------------------------------------
// Batched products whose members SHARE a small left operand (ptts_dense_bf16x6_batched with strideA == 0, M <= 128, K <= 128: the
// transforms of the frequency-domain context Conv1D, a constant twiddle matrix against one right operand per segment).
// dense_bf16x6_kernel gives each member a workgroup of its own that lives KS <= 4 k-steps: every one of them loads, pads and splits
// the same A, meets a barrier per k-step, and its prologue and store drain are a large share of its life.  Here A is split ONCE per
// workgroup into the LDS -- the planes of all k-steps, in dense_bf16x6_kernel's row layout and swizzle: [k-step][plane][128 rows x 32 k]
// -- and after the one barrier the workgroup's waves walk work items on their own: item = (member z, 32-column slice), wave w of
// workgroup g takes items 8 g + w, + 8 G, ...  A wave loads the weight fragments of an item's two column tiles for all k-steps straight
// from global memory (load_w's 1-KB loads), and refills the registers of k-step s with the NEXT item's as soon as step s is multiplied:
// a whole item of loads (24 KB per wave) is in flight under the MFMAs and the stores.  No barrier, no LDS write and no word between
// workgroups after the prologue.  The k-steps run in order and the six products of an accumulator in DNS_PRODUCTS_NPL's order, so every
// output is dense_bf16x6_kernel's bit for bit (an MFMA's output cell depends on its own row and column alone, so the tiling is free).
// Stores: 16-byte where the quad lies inside N and ldc / strideC / C keep the alignment (vec_out here says ONLY that: N % 4 != 0, the
// 601 channels of the input's transform, stores its last quad of a row element-wise and the others whole), cells guarded by M and N.
// ------------------------------------------------------------------------------------------------------------
constexpr int RES_M = 128, RES_K = 128;
constexpr int RES_KS = RES_K / BK;
constexpr int RES_PL = RES_M * BK;            // elements of one plane of one k-step
template <int NPL> constexpr size_t resident_lds_bytes() { return (size_t)RES_KS * NPL * RES_PL * sizeof(u16); }

// MT = ceil(M / 16) row tiles.  KSC = the number of k-steps when it is RES_KS (the transforms: K = 120, 124), 0 = any (g.KS): with a
// compile-time count the loads of an item are a fixed sequence, and the wait in front of k-step s covers the loads up to s alone -- not
// the later k-steps' and not the stores of the item before.
//
// ROWS: the right operand as fp32 rows (ptts_dense_rows_desc: strided rows, or the windows of a frame sequence) instead of planes.  A
// wave loads an item's fragments as the split pass did -- a lane's 8 consecutive k of one column, eight 4-byte loads per column tile and
// k-step, 64 VGPRs for an item instead of the planes' 96 -- and splits the 16 values of a k-step right in front of that k-step's MFMAs;
// the registers are refilled with the next item's rows behind them, as above.  Through registers and not through the free 64 KB of LDS:
// the waves stay independent of each other (no barrier, no LDS write after the prologue), and the access pattern is the one the split
// pass already had.  A row or column that counts as zero is not read: the lane's offset is clamped to the source's first float, and the
// select that makes the zero waits with the split, so that it does not wait for the load in front of the k-steps before.
// r.mirror = Kh > 0: the store of row m, column n is repeated at row m ^ 1, column Kh + n, negated for odd m (dft_mirror_kernel).
struct RowsArgs {
    const float* B; long long strideB;
    int ldb, windows, T, NS, S, row_off, kvalid, mirror;
};
// what a lane knows of an item's rows: for column tile j its offset of (k = 8 lg, its column) from r.B and the number of rows that are
// read, len (0 for a column beyond N); t0 = 8 lg - (first row that is read).  Row k = 8 lg + c is read when t0 + c < len.
template <bool ROWS> struct RowsItemT { unsigned base[2], len[2], t0; };       // (base in bytes)
template <> struct RowsItemT<false> {};

template <int NPL, int MT = RES_M / 16, int KSC = 0, bool ROWS = false>
__global__ __launch_bounds__(THREADS) void dense_bf16x6_resident_kernel(DenseArgs g, int slices, int items, RowsArgs r) {
    extern __shared__ __attribute__((aligned(16))) u16 lds_r[];
    using RowsItem = RowsItemT<ROWS>;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int li = lane & 15, lg = lane >> 4;
    const int KS = KSC ? KSC : g.KS;
    const size_t ps = (size_t)g.NT * KS * 512;
    const int stride = 8 * (int)gridDim.x;
    int item = 8 * (int)blockIdx.x + wave;
    const bool live = item < items;           // (fewer items than waves: the others only help with the prologue)

    // ---- prologue, first half: this lane's quads of A.  Quad q = tid + 512 j -> row q >> 5, k-quad q & 31 (k-step (q & 31) >> 3); rows
    // >= M and quads >= K read A's first quad and are zeroed by a select
    constexpr int NQ = RES_M * (RES_K / 4) / THREADS;
    f32x4 va[NQ];
#pragma unroll
    for (int j = 0; j < NQ; ++j) {
        const int q = tid + j * THREADS, row = q >> 5, k4 = 4 * (q & 31);
        const bool ok = row < g.M && k4 < g.K;                // K % 4 == 0: a quad is all inside or all outside
        va[j] = *reinterpret_cast<const f32x4*>(g.A + (ok ? (long long)row * g.lda + k4 : 0));
    }

    // ---- weight fragments of an item: column tiles 2 sl, 2 sl + 1 of member z, k-step s
    bf16x8 wf[RES_KS][2][NPL];
    auto load_w = [&](int it, int s) {
        const int z = it / slices, sl = it - z * slices;
        const u16* wp = g.planes + (long long)z * g.bsP + (((size_t)(2 * sl) * KS + s) * 64 + lane) * 8;
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int p = 0; p < NPL; ++p) wf[s][j][p] = *reinterpret_cast<const bf16x8*>(wp + p * ps + (size_t)j * KS * 512);
    };
    // ---- ROWS: the same fragments as fp32, wr[s][j][e] = B_z[32 s + 8 lg + e][32 sl + 16 j + li]
    float wr[ROWS ? RES_KS : 1][2][8];
    auto rows_item = [&](int it) {
        RowsItem q;
        if constexpr (ROWS) {
            const int z = it / slices, sl = it - z * slices;
            long long zoff; int rlo = 0, rhi = r.kvalid;
            if (r.windows) {
                const int b = z / r.NS, sg = z - b * r.NS;
                const int r0 = r.row_off + sg * r.S;              // source row of window row 0 (may be negative)
                zoff = ((long long)b * r.T + r0) * r.ldb;
                rlo = r0 < 0 ? -r0 : 0;
                rhi = min(r.kvalid, r.T - r0);
            } else {
                zoff = (long long)z * r.strideB;
            }
            const unsigned len = (unsigned)max(rhi - rlo, 0);
            q.t0 = (unsigned)(8 * lg - rlo);
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                const int n = 32 * sl + 16 * j + li;
                q.len[j] = n < g.N ? len : 0u;
                q.base[j] = 4u * ((unsigned)zoff + (unsigned)(8 * lg) * (unsigned)r.ldb + (unsigned)n);      // (bytes, modulo 2^32; right wherever it is used)
            }
        }
        return q;
    };
    auto load_r = [&](const RowsItem& q, int s) {
        if constexpr (ROWS) {
            const unsigned ldb4 = 4u * (unsigned)r.ldb;            // a 32-bit byte offset from a uniform base: one address register per load
            unsigned a[2] = {q.base[0] + 32u * s * ldb4, q.base[1] + 32u * s * ldb4};
#pragma unroll
            for (int e = 0; e < 8; ++e)
#pragma unroll
                for (int j = 0; j < 2; ++j) {                     // (the two column tiles of a row lie side by side: one after the other)
                    const unsigned c = 32 * s + e;
                    wr[ROWS ? s : 0][j][e] = *reinterpret_cast<const float*>(reinterpret_cast<const char*>(r.B) + (q.t0 + c < q.len[j] ? a[j] : 0u));
                    a[j] += ldb4;                                 // (row by row: one scalar, not one per row)
                }
        }
    };
    // the first item's fragments go out behind A's quads and in front of the split: no branch here -- a wave without an item loads the
    // last item's and drops them -- so that the split waits for A alone
    RowsItem qcur = rows_item(live ? item : items - 1);
#pragma unroll
    for (int s = 0; s < RES_KS; ++s) {
        if (s < KS) { if constexpr (ROWS) load_r(qcur, s); else load_w(live ? item : items - 1, s); }
        __builtin_amdgcn_sched_barrier(0);                    // k-step by k-step: loads come back in the order they went out
    }

    // ---- prologue, second half: split into the planes of all k-steps in the LDS
    {
#pragma unroll
        for (int j = 0; j < NQ; ++j) {
            const int q = tid + j * THREADS, row = q >> 5, s = (q & 31) >> 3, kq = q & 7;
            u16* d = lds_r + s * NPL * RES_PL + row * BK + ((((kq >> 1) ^ ((row >> 1) & 2))) << 3) + (kq & 1) * 4;
            const f32x4 a = (row < g.M && 4 * (q & 31) < g.K) ? va[j] : f32x4{0.f, 0.f, 0.f, 0.f};
            if (NPL == 3) {
                unsigned a1, a2, a3, b1, b2, b3;
                split3_pair(a[0], a[1], a1, a2, a3);
                split3_pair(a[2], a[3], b1, b2, b3);
                *reinterpret_cast<u32x2*>(d) = (u32x2){a1, b1};
                *reinterpret_cast<u32x2*>(d + RES_PL) = (u32x2){a2, b2};
                *reinterpret_cast<u32x2*>(d + 2 * RES_PL) = (u32x2){a3, b3};
            } else {
                *reinterpret_cast<u32x2*>(d) = (u32x2){pk_bf16(a[0], a[1]), pk_bf16(a[2], a[3])};
            }
        }
    }
    __syncthreads();                                          // the only barrier
    if (!live) return;

    // activation fragment of row tile i: row 16 i + li, quad lg (swizzle = bit 2 of li), k-step s, plane p
    const int boff = li * BK + ((lg ^ ((li >> 1) & 2)) << 3);
    // One item.  The bias goes into registers in front of the k-steps: loads come back in order, and behind the next item's fragments
    // it would hold the store until all of them are in.
    auto run_item = [&](const int it, const bool has_next, const int next, const RowsItem& qc, const RowsItem& qn) __attribute__((always_inline)) {
        const int z = it / slices, sl = it - z * slices;
        f32x4 bv[2] = {f32x4{0.f, 0.f, 0.f, 0.f}, f32x4{0.f, 0.f, 0.f, 0.f}};
        if (g.bias) {                                         // (four plain loads per tile, columns beyond N clamped and never stored: no branch per lane)
#pragma unroll
            for (int j = 0; j < 2; ++j)
#pragma unroll
                for (int e = 0; e < 4; ++e) bv[j][e] = g.bias[min(32 * sl + 16 * j + 4 * lg + e, g.N - 1)];
        }
        f32x4 acc[MT][2];
#pragma unroll
        for (int i = 0; i < MT; ++i) { acc[i][0] = f32x4{0.f, 0.f, 0.f, 0.f}; acc[i][1] = f32x4{0.f, 0.f, 0.f, 0.f}; }
#pragma unroll
        for (int s = 0; s < RES_KS; ++s) {
            if (s < KS) {
                const u16* as = lds_r + s * NPL * RES_PL + boff;
                bf16x8 ws[2][NPL];                            // ROWS: this k-step's planes, made here (split3_dense_weight_strided_kernel's)
                if constexpr (ROWS) {
#pragma unroll
                    for (int j = 0; j < 2; ++j) {
                        unsigned q[3][4];
#pragma unroll
                        for (int h = 0; h < 4; ++h) {
                            const unsigned c = 32 * s + 2 * h;
                            const float v0 = qc.t0 + c < qc.len[j] ? wr[ROWS ? s : 0][j][2 * h] : 0.f;
                            const float v1 = qc.t0 + c + 1 < qc.len[j] ? wr[ROWS ? s : 0][j][2 * h + 1] : 0.f;
                            if (NPL == 3) split3_pair(v0, v1, q[0][h], q[1][h], q[2][h]);
                            else q[0][h] = pk_bf16(v0, v1);
                        }
#pragma unroll
                        for (int p = 0; p < NPL; ++p) ws[j][p] = __builtin_bit_cast(bf16x8, make_uint4(q[p][0], q[p][1], q[p][2], q[p][3]));
                    }
                }
#pragma unroll
                for (int i = 0; i < MT; ++i) {
                    bf16x8 bf[NPL];
#pragma unroll
                    for (int p = 0; p < NPL; ++p) bf[p] = *reinterpret_cast<const bf16x8*>(as + p * RES_PL + i * 16 * BK);
#define DNS_WF(J, PW) (ROWS ? ws[J][PW < NPL ? PW : 0] : wf[s][J][PW < NPL ? PW : 0])
#define DNS_MM(PA, PW)                                                                                    \
                    acc[i][0] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(DNS_WF(0, PW), bf[PA < NPL ? PA : 0], acc[i][0], 0, 0, 0);    \
                    acc[i][1] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(DNS_WF(1, PW), bf[PA < NPL ? PA : 0], acc[i][1], 0, 0, 0);
                    DNS_PRODUCTS_NPL(NPL, DNS_MM);
#undef DNS_MM
#undef DNS_WF
                }
                if (has_next) { if constexpr (ROWS) load_r(qn, s); else load_w(next, s); }      // this k-step's registers are free: the next item's loads go out
                // (a compile-time KS makes the k-steps one basic block; moved up across this line, the later steps' LDS reads cost registers
                // the fragments in flight need)
                if (KSC) __builtin_amdgcn_sched_barrier(0);
            }
        }
        // ---- store: lane (li, lg) of acc[i][j] holds row 16 i + li, columns 32 sl + 16 j + 4 lg .. + 3 of member z
        float* __restrict__ Cz = g.C + (long long)z * g.bsC;
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int n = 32 * sl + 16 * j + 4 * lg;
            if (n >= g.N) continue;
            if (g.vec_out && n + 3 < g.N) {
#pragma unroll
                for (int i = 0; i < MT; ++i) {
                    const int m = 16 * i + li;
                    if (m < g.M) {
                        const f32x4 v = acc[i][j] + bv[j];
                        *reinterpret_cast<f32x4*>(Cz + (long long)m * g.ldc + n) = v;
                        if (ROWS && r.mirror > 0) *reinterpret_cast<f32x4*>(Cz + (long long)(m ^ 1) * g.ldc + r.mirror + n) = (li & 1) ? -v : v;
                    }
                }
            } else {
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    if (n + e >= g.N) continue;
#pragma unroll
                    for (int i = 0; i < MT; ++i) {
                        const int m = 16 * i + li;
                        if (m < g.M) {
                            const float v = acc[i][j][e] + bv[j][e];
                            Cz[(long long)m * g.ldc + n + e] = v;
                            if (ROWS && r.mirror > 0) Cz[(long long)(m ^ 1) * g.ldc + r.mirror + n + e] = (li & 1) ? -v : v;
                        }
                    }
                }
            }
        }
    };
    // The first item apart from the loop: only loads are in flight in front of it, they come back in order, and the wait in front of
    // k-step s is for the fragments up to s.  In the loop the stores of the item before are in flight too; loads and stores do not
    // come back in one order, so there the first wait of an item is for everything.
    int next = item + stride;
    RowsItem qnext = qcur;
    if (ROWS && next < items) qnext = rows_item(next);
    run_item(item, next < items, next, qcur, qnext);
    while (next < items) {
        item = next;
        next = item + stride;
        qcur = qnext;
        if (ROWS && next < items) qnext = rows_item(next);
        run_item(item, next < items, next, qcur, qnext);
    }
}


// ------------------------------------------------------------------------------------------------------------
// Weight gradient  dW[Kin][N] += T(A)[M][Kin]^T . dY[M][N],  db[N] += sum_m dY[m][:]   (reduction over the M frames).
// Both operands are activations: each 32-row slab of A (with the pending transform of the layer input) and of dY is split
// on its way into the LDS as row-major planes [32 m][128 columns] and read TRANSPOSED by ds_read_b64_tr_b16, so that a
// lane gets 8 consecutive m of its column (the MFMA's k index) -- the construction of conv2d_mfma.hip's weight gradient.
// A row is eight 32-byte segments (one 16-column MFMA tile each); segment t of row r lies at position
// (t + r + 4 (r >> 3)) & 7: the four rows a 16-lane group reads, and the two groups of a half-wave, hit disjoint banks.
// Output tile 128 x 128 per workgroup (8 waves: 2 x 4 MFMA tiles each), the frames of a tile shared out over
// 256 / tiles workgroups; every workgroup stores its partial tile (and 128 bias sums, from the staged dY values of the first
// tile row) as a row of the caller's workspace, and dense_wgrad_reduce_kernel -- one grouped launch for a batch of products -- adds
// the rows in a fixed order into the gradient buffers (a first version flushed with fp32 atomics from every workgroup).
// ------------------------------------------------------------------------------------------------------------
typedef short s16x4 __attribute__((ext_vector_type(4)));
typedef s16x4 __attribute__((address_space(3)))* lds_s16x4_ptr;
__device__ __forceinline__ bf16x4 tr_read(const u16* p) {
    return __builtin_bit_cast(bf16x4, __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4_ptr)(p)));
}
__device__ __forceinline__ bf16x8 cat8(bf16x4 a, bf16x4 b) { return __builtin_shufflevector(a, b, 0, 1, 2, 3, 4, 5, 6, 7); }

// The k-step of the two transposed-reduction kernels with three planes: 48 MFMAs (tile row, product, dY-column tile), 18 transposed
// fragment reads and the StageSlices of the next slab.  Fragment ids: 3 i + p = A fragment of tile row i, plane p; 6 + 3 j + p = dY (B)
// fragment of column tile j, plane p.  Seven fragments are read in front of the first MFMA (with the global loads of the slab after the
// next behind them, under the LDS latency), the other eleven one per gap, each four or more MFMAs ahead of its first use; from gap 11 on a
// gap takes one slice; what is left of the slices runs behind the last MFMA, in front of the barrier.
constexpr int TN_HEAD_FRAGS = 7, TN_READ_GAPS = 11, TN_MFMAS = 48;
constexpr int tn_read_order(int r) {
    constexpr int ro[18] = {2, 6, 9, 12, 15, 1, 7,   10, 13, 16, 0, 8, 11, 14, 17, 5, 4, 3};
    return ro[r];
}

struct WgradArgs {
    const float* A; const float* dY; const float* mask_src; const float* in_scale; const float* in_shift;
    float* partials;                         // [tile][split][part]: the workgroups' partial tiles (+ 128 bias sums, + the remainder tile)
    int Kin, N, M;
    long long lda, ldb;
    float alpha;
    int tiles_n, steps_total, split;         // 128-column tiles along N; 32-row steps of M; workgroups per tile
    int tiles_k, part;                       // 128-row tiles along Kin (wgrad_tiles_k); floats of a partial row (wgrad_part)
};

constexpr int WT = 128;                       // tile edge (columns of A x columns of dY)
constexpr int WROW = WT;                      // elements per staged row of a plane
constexpr int WPL = 32 * WROW;                // elements of one plane of one operand
constexpr int WPART = WT * WT + WT;           // floats of a workgroup's partial row: the tile and the bias sums
// Remainder tile: 1..16 rows of dW beyond a multiple of 128 (the critic's 260-wide layer) are no tile row of their own -- 4 live rows
// of 128 at the price of a whole tile, and half as many frames' worth of workgroups for every tile -- but a 16-row tile more for the
// workgroups of the LAST full tile row: rows 128 tiles_k .. + 15 against their 128 dY columns, eight MFMA tiles, one per wave.
constexpr int WXR = 16;                       // rows of the remainder tile
constexpr int WXPL = 32 * WXR + 4 * 64;       // elements of a plane of its staged A columns: 32 rows of 16, 64 more per 8 rows (banks)
constexpr int WPARTX = WXR * WT;              // floats it adds to every partial row of the product
__host__ __device__ inline bool wgrad_has_rem(int Kin) { return Kin > WT && Kin % WT >= 1 && Kin % WT <= WXR; }
__host__ __device__ inline int wgrad_tiles_k(int Kin) { return wgrad_has_rem(Kin) ? Kin / WT : (Kin + WT - 1) / WT; }
__host__ __device__ inline int wgrad_part(int Kin) { return WPART + (wgrad_has_rem(Kin) ? WPARTX : 0); }

// (cur: the buffer that is multiplied; ao / bo: the lane's fragment offsets; st: the slices of the next slab, already begun;
// load_next: the global loads of the slab after the next)
template <class ST, class LoadF>
__device__ __forceinline__ void tn_step_own(const u16* cur, const int (&ao)[2][2], const int (&bo)[4][2], f32x4 (&acc)[2][4], ST& st,
                                            f32x4& bsum, LoadF&& load_next) {
    bf16x8 af[2][3], bf[4][3];
    auto read = [&](auto R) {
        constexpr int id = tn_read_order(decltype(R)::value);
        if constexpr (id < 6) {
            constexpr int i = id / 3, p = id % 3;
            af[i][p] = cat8(tr_read(cur + p * WPL + ao[i][0]), tr_read(cur + p * WPL + ao[i][1]));
        } else {
            constexpr int j = (id - 6) / 3, p = (id - 6) % 3;
            bf[j][p] = cat8(tr_read(cur + p * WPL + bo[j][0]), tr_read(cur + p * WPL + bo[j][1]));
        }
    };
    static_for<0, TN_HEAD_FRAGS>(read);
    load_next();
    __builtin_amdgcn_sched_barrier(0);
    static_for<0, TN_MFMAS>([&](auto Q) {
        constexpr int q = decltype(Q)::value, i = q / 24, pr = (q % 24) / 4, j = q % 4;
        acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[i][prod_pa(pr)], bf[j][prod_pw(pr)], acc[i][j], 0, 0, 0);
        if constexpr (q < TN_READ_GAPS) read(std::integral_constant<int, TN_HEAD_FRAGS + q>{});
        else st.template run<q - TN_READ_GAPS>(bsum);
        __builtin_amdgcn_sched_barrier(0);
    });
    static_for<TN_MFMAS - TN_READ_GAPS, ST::N>([&](auto I) { st.template run<decltype(I)::value>(bsum); });
}

template <int MODE, bool AFFINE, int NPL, bool XR = false>
__global__ __launch_bounds__(THREADS) void dense_wgrad_bf16x6_kernel(WgradArgs g) {
    constexpr bool MASK = MODE == PTTS_IN_MASKMUL;
    extern __shared__ __attribute__((aligned(16))) u16 lds_w[];          // [buffer][A planes 0..2 | dY planes 0..2]: 96 KB; XR: + [buffer][3 WXPL]
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int li = lane & 15, lg = lane >> 4;
    const int tile = blockIdx.y, tk = tile / g.tiles_n, tn = tile - tk * g.tiles_n;
    const int k0 = tk * WT, n0 = tn * WT;
    const bool xr_wg = XR && tk == g.tiles_k - 1;                        // this workgroup also owns the remainder tile
    // this workgroup's share of the 32-row steps
    const int per = (g.steps_total + g.split - 1) / g.split;
    const int s_begin = blockIdx.x * per, s_end = min(g.steps_total, s_begin + per);
    const int nsteps = max(0, s_end - s_begin);           // (a share without steps still writes its row of zeros)

    // ---- staging slots: float4 q = tid + 512 j (j = 0, 1) -> row q >> 5, columns 4 (q & 31) ..; the same columns for both j
    const int c4 = tid & 31;
    const bool a_ok = k0 + 4 * c4 < g.Kin, d_ok = n0 + 4 * c4 < g.N;     // Kin, N multiples of 4
    const float* pa = g.A + (a_ok ? k0 + 4 * c4 : 0);
    const float* pm = MASK ? g.mask_src + (a_ok ? k0 + 4 * c4 : 0) : nullptr;
    const float* pd = g.dY + (d_ok ? n0 + 4 * c4 : 0);
    int dst[2];
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int row = (tid + j * THREADS) >> 5;
        dst[j] = row * WROW + ((((c4 >> 2) + row + 4 * (row >> 3)) & 7) << 4) + (c4 & 3) * 4;
    }
    f32x4 sc = {1.f, 1.f, 1.f, 1.f}, sh = {0.f, 0.f, 0.f, 0.f};
    if (AFFINE && a_ok) { sc = *reinterpret_cast<const f32x4*>(g.in_scale + k0 + 4 * c4); sh = *reinterpret_cast<const f32x4*>(g.in_shift + k0 + 4 * c4); }
    // remainder tile: the 16 columns of A behind the last full tile, 32 rows x 4 quads = the lanes of waves 0 and 1, one quad each
    const bool xr_stage = xr_wg && wave < 2;
    const int xrow = tid >> 2, xkq = g.tiles_k * WT + 4 * (tid & 3);
    const bool x_ok = xr_stage && xkq < g.Kin;
    const float* pax = g.A + (x_ok ? xkq : 0);
    const float* pmx = MASK ? g.mask_src + (x_ok ? xkq : 0) : nullptr;
    auto xrow_off = [](int row) { return row * WXR + 64 * (row >> 3); };
    const int xdst = xrow_off(xrow & 31) + 4 * (tid & 3);
    f32x4 scx = {1.f, 1.f, 1.f, 1.f}, shx = {0.f, 0.f, 0.f, 0.f};
    if (AFFINE && x_ok) { scx = *reinterpret_cast<const f32x4*>(g.in_scale + xkq); shx = *reinterpret_cast<const f32x4*>(g.in_shift + xkq); }
    struct Stage { f32x4 va[2], vm[MASK ? 2 : 1], vd[2]; bool ok[2]; f32x4 vx, vmx; bool okx; };
    auto load = [&](int s, Stage& sg) {
        if (XR && xr_stage) {                                            // (wave-uniform)
            const int m = (s_begin + s) * 32 + xrow;
            sg.okx = s < nsteps && m < g.M && x_ok;
            const long long r = sg.okx ? m : 0;
            sg.vx = *reinterpret_cast<const f32x4*>(pax + r * g.lda);
            if (MASK) sg.vmx = *reinterpret_cast<const f32x4*>(pmx + r * g.lda);
        }
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int m = (s_begin + s) * 32 + ((tid + j * THREADS) >> 5);
            sg.ok[j] = s < nsteps && m < g.M;
            const long long r = sg.ok[j] ? m : 0;
            sg.va[j] = *reinterpret_cast<const f32x4*>(pa + r * g.lda);
            if (MASK) sg.vm[j] = *reinterpret_cast<const f32x4*>(pm + r * g.lda);
            sg.vd[j] = *reinterpret_cast<const f32x4*>(pd + r * g.ldb);
        }
    };
    f32x4 bsum = {0.f, 0.f, 0.f, 0.f};
    auto commit = [&](const Stage& sg, u16* ls, u16* lsx) {
        const f32x4 z4 = {0.f, 0.f, 0.f, 0.f};
        if (XR && xr_stage) {                                            // the transform and the split of the main tile's columns
            f32x4 a = sg.vx;
            if (MODE == PTTS_IN_LRELU) {
                if (AFFINE) a = a * scx + shx;
                if (!sg.okx) a = z4;
#pragma unroll
                for (int e = 0; e < 4; ++e) a[e] = max_fast(a[e], g.alpha * a[e]);
            } else if (MASK) {
                if (!sg.okx) a = z4;
#pragma unroll
                for (int e = 0; e < 4; ++e) a[e] = a[e] * (sg.vmx[e] > 0.f ? 1.f : g.alpha);
            } else {
                if (!sg.okx) a = z4;
            }
            u16* q = lsx + xdst;
            if (NPL == 3) {
                unsigned a1, a2, a3, b1, b2, b3;
                split3_pair(a[0], a[1], a1, a2, a3);
                split3_pair(a[2], a[3], b1, b2, b3);
                *reinterpret_cast<u32x2*>(q) = (u32x2){a1, b1};
                *reinterpret_cast<u32x2*>(q + WXPL) = (u32x2){a2, b2};
                *reinterpret_cast<u32x2*>(q + 2 * WXPL) = (u32x2){a3, b3};
            } else {
                *reinterpret_cast<u32x2*>(q) = (u32x2){pk_bf16(a[0], a[1]), pk_bf16(a[2], a[3])};
            }
        }
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            f32x4 a = sg.va[j], d = sg.vd[j];
            if (MODE == PTTS_IN_LRELU) {
                if (AFFINE) a = a * sc + sh;
                if (!(sg.ok[j] && a_ok)) a = z4;
#pragma unroll
                for (int e = 0; e < 4; ++e) a[e] = max_fast(a[e], g.alpha * a[e]);
            } else if (MASK) {
                if (!(sg.ok[j] && a_ok)) a = z4;
#pragma unroll
                for (int e = 0; e < 4; ++e) a[e] = a[e] * (sg.vm[j][e] > 0.f ? 1.f : g.alpha);
            } else {
                if (!(sg.ok[j] && a_ok)) a = z4;
            }
            if (!(sg.ok[j] && d_ok)) d = z4;
            bsum += d;
            u16* q = ls + dst[j];
            if (NPL == 3) {
                unsigned a1, a2, a3, b1, b2, b3;
                split3_pair(a[0], a[1], a1, a2, a3);
                split3_pair(a[2], a[3], b1, b2, b3);
                *reinterpret_cast<u32x2*>(q) = (u32x2){a1, b1};
                *reinterpret_cast<u32x2*>(q + WPL) = (u32x2){a2, b2};
                *reinterpret_cast<u32x2*>(q + 2 * WPL) = (u32x2){a3, b3};
                split3_pair(d[0], d[1], a1, a2, a3);
                split3_pair(d[2], d[3], b1, b2, b3);
                q += 3 * WPL;
                *reinterpret_cast<u32x2*>(q) = (u32x2){a1, b1};
                *reinterpret_cast<u32x2*>(q + WPL) = (u32x2){a2, b2};
                *reinterpret_cast<u32x2*>(q + 2 * WPL) = (u32x2){a3, b3};
            } else {
                *reinterpret_cast<u32x2*>(q) = (u32x2){pk_bf16(a[0], a[1]), pk_bf16(a[2], a[3])};
                *reinterpret_cast<u32x2*>(q + 3 * WPL) = (u32x2){pk_bf16(d[0], d[1]), pk_bf16(d[2], d[3])};
            }
        }
    };

    // ---- MFMA tiles of this wave: A-column tiles 2 (wave & 3) + {0, 1}, dY-column tiles 4 (wave >> 2) + {0..3}
    // transposed-read address of lane (li, lg) in tile t: row 8 lg + (li >> 2) (+ 4 for the second half), columns 4 (li & 3)
    auto tr_off = [&](int t, int half) {
        const int row = 8 * lg + (li >> 2) + 4 * half;
        return row * WROW + (((t + row + 4 * (row >> 3)) & 7) << 4) + (li & 3) * 4;
    };
    int ao[2][2], bo[4][2];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
#pragma unroll
        for (int i = 0; i < 2; ++i) ao[i][h] = tr_off(2 * (wave & 3) + i, h);
#pragma unroll
        for (int i = 0; i < 4; ++i) bo[i][h] = 3 * WPL + tr_off(4 * (wave >> 2) + i, h);
    }
    f32x4 acc[2][4];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
    // remainder tile of this wave: its 16 rows x dY-column tile `wave` (one of the four above, read once more: no wave-dependent
    // index into the fragment registers); the same six products in the same order
    f32x4 accx = {0.f, 0.f, 0.f, 0.f};
    int axo[2], bxo[2];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        axo[h] = xrow_off(8 * lg + (li >> 2) + 4 * h) + (li & 3) * 4;
        bxo[h] = 3 * WPL + tr_off(wave, h);
    }
    auto mfma_rem = [&](const u16* ls, const u16* lsx) {
        bf16x8 af[NPL], bf[NPL];
#pragma unroll
        for (int p = 0; p < NPL; ++p) {
            af[p] = cat8(tr_read(lsx + p * WXPL + axo[0]), tr_read(lsx + p * WXPL + axo[1]));
            bf[p] = cat8(tr_read(ls + p * WPL + bxo[0]), tr_read(ls + p * WPL + bxo[1]));
        }
#define DNS_MM(PA, PW) accx = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[PA < NPL ? PA : 0], bf[PW < NPL ? PW : 0], accx, 0, 0, 0);
        DNS_PRODUCTS_NPL(NPL, DNS_MM);
#undef DNS_MM
    };
    // one k-step of MFMAs on buffer BUF (a compile-time index: every LDS address is a lane base + an immediate); the dY
    // fragments are read once and serve both A-column tiles; `stage` (the next step's transform / split / LDS stores and the
    // loads of the step after) runs between the two tile rows in waves 0-3 and in front of them in waves 4-7
    auto mfma_tile_row = [&](const u16* ls, int i, const bf16x8 (&bf)[4][NPL]) {
        bf16x8 af[NPL];
#pragma unroll
        for (int p = 0; p < NPL; ++p) af[p] = cat8(tr_read(ls + p * WPL + ao[i][0]), tr_read(ls + p * WPL + ao[i][1]));
#define DNS_MM(PA, PW)                                                                                       \
        _Pragma("unroll") for (int j = 0; j < 4; ++j)                                                        \
            acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[PA < NPL ? PA : 0], bf[j][PW < NPL ? PW : 0], acc[i][j], 0, 0, 0);
        DNS_PRODUCTS_NPL(NPL, DNS_MM);
#undef DNS_MM
    };
    auto read_bf = [&](const u16* ls, bf16x8 (&bf)[4][NPL]) {
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int p = 0; p < NPL; ++p) bf[j][p] = cat8(tr_read(ls + p * WPL + bo[j][0]), tr_read(ls + p * WPL + bo[j][1]));
    };

    u16* const buf0 = lds_w;
    u16* const buf1 = lds_w + 6 * WPL;
    u16* const xbuf0 = lds_w + 12 * WPL;
    u16* const xbuf1 = xbuf0 + 3 * WXPL;
    Stage sg;
    load(0, sg);
    commit(sg, buf0, xbuf0);
    load(1, sg);
    __syncthreads();
    auto step = [&](int s, const u16* cur, u16* nxt, const u16* curx, u16* nxtx, bool stage_first) {
        bf16x8 bf[4][NPL];
        if (stage_first) { commit(sg, nxt, nxtx); load(s + 2, sg); }       // (rows of a step beyond the share are staged as zeros)
        read_bf(cur, bf);
        mfma_tile_row(cur, 0, bf);
        if (!stage_first) { commit(sg, nxt, nxtx); load(s + 2, sg); }
        mfma_tile_row(cur, 1, bf);
        if (XR && xr_wg) mfma_rem(cur, curx);                        // (workgroup-uniform, in front of the barrier)
        __syncthreads();
    };
    // the staging of step s + 1 in this wave's own MFMA gaps (StageSlices), the same in every wave.  Not with one plane (8 MFMAs), not
    // with the remainder tile (256 registers already) and not with the affine input, whose trace row did not shrink:
    // those keep the k-step above.
    constexpr bool OWN_GAPS = NPL == 3 && !XR && !AFFINE;
    auto step_own = [&](int s, const u16* cur, u16* nxt) {
        if constexpr (OWN_GAPS) {
            using ST = StageSlices<MODE, AFFINE, true, WPL>;
            ST st;
            st.begin(sg.va, sg.vm, sg.vd);
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                st.ok[j] = sg.ok[j] && a_ok; st.ok[2 + j] = sg.ok[j] && d_ok;
                st.dst[j] = nxt + dst[j]; st.dst[2 + j] = nxt + dst[j] + 3 * WPL;
            }
            st.sc = sc; st.sh = sh; st.alpha = g.alpha;
            tn_step_own(cur, ao, bo, acc, st, bsum, [&]() { load(s + 2, sg); });   // (rows of a step beyond the share are staged as zeros)
            __syncthreads();
        }
    };
    // Two steps per trip: the buffers are compile-time.  The forms that keep `step`: the two waves of a SIMD leave every barrier together,
    // so waves 0-3 run half of their MFMAs before the staging of the next step and waves 4-7 stage first -- one wave's vector work
    // under the other's matrix work.
    if (OWN_GAPS) {
        int s = 0;
        for (; s + 1 < nsteps; s += 2) { step_own(s, buf0, buf1); step_own(s + 1, buf1, buf0); }
        if (s < nsteps) step_own(s, buf0, buf1);
    } else if (wave < 4) {
        int s = 0;
        for (; s + 1 < nsteps; s += 2) { step(s, buf0, buf1, xbuf0, xbuf1, false); step(s + 1, buf1, buf0, xbuf1, xbuf0, false); }
        if (s < nsteps) step(s, buf0, buf1, xbuf0, xbuf1, false);
    } else {
        int s = 0;
        for (; s + 1 < nsteps; s += 2) { step(s, buf0, buf1, xbuf0, xbuf1, true); step(s + 1, buf1, buf0, xbuf1, xbuf0, true); }
        if (s < nsteps) step(s, buf0, buf1, xbuf0, xbuf1, true);
    }

    // ---- the workgroup's partial tile, row (tile, split index) of the partials: [128 k][128 n] | 128 column sums of dY | with a
    // remainder in the product, [16 k][128 n] of it (written by the last tile row's workgroups, never read of the others).
    // lane (li, lg) of acc[i][j] holds rows k = 32 (wave & 3) + 16 i + 4 lg + r, column 64 (wave >> 2) + 16 j + li
    float* out = g.partials + ((size_t)tile * g.split + blockIdx.x) * g.part;
    if (XR && xr_wg) {
        // lane (li, lg) of accx holds rows 128 tiles_k + 4 lg + r, column 16 wave + li of the tile
#pragma unroll
        for (int r = 0; r < 4; ++r) out[WPART + (4 * lg + r) * WT + 16 * wave + li] = accx[r];
    }
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int n = 64 * (wave >> 2) + 16 * j + li;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int k = 32 * (wave & 3) + 16 * i + 4 * lg + r;
                out[k * WT + n] = acc[i][j][r];
            }
        }
    {
        // 16 lanes (tid >> 5) share the column group c4: sum through the LDS (the planes are dead)
        float* red = reinterpret_cast<float*>(lds_w);
        __syncthreads();
        *reinterpret_cast<f32x4*>(red + tid * 4) = bsum;
        __syncthreads();
        if (tid < WT) {
            float v = 0.f;
#pragma unroll
            for (int q = 0; q < 16; ++q) v += red[(q * 32 + (tid >> 2)) * 4 + (tid & 3)];
            out[WT * WT + tid] = v;
        }
    }
}


// partial rows -> gradient buffers, several products per launch.  Thread = one element of a tile, summed over the split
// workgroups in a fixed order; added into C / the bias gradient with one fp32 atomic per element (products of one backward
// pass share gradient buffers: first- and second-order sweeps of a layer).
constexpr int DR_MAX = 16;
struct DwReduceArgs {
    int n;
    int blk_begin[DR_MAX + 1];
    const float* partials[DR_MAX]; float* C[DR_MAX]; float* colsum[DR_MAX];
    int split[DR_MAX], tiles_n[DR_MAX], Kin[DR_MAX], N[DR_MAX];
    long long ldc[DR_MAX];
};
// blocks per tile: a block per 256 floats of a partial row (the tile, the bias sums, with a remainder in the product its 16 rows)
__host__ __device__ inline int dr_bpt(int Kin) { return (wgrad_part(Kin) + 255) / 256; }
__global__ __launch_bounds__(256) void dense_wgrad_reduce_kernel(DwReduceArgs a) {
    int gi = 0;
    while ((int)blockIdx.x >= a.blk_begin[gi + 1]) ++gi;
    const int b = blockIdx.x - a.blk_begin[gi];
    const int PART = wgrad_part(a.Kin[gi]), BPT = dr_bpt(a.Kin[gi]);
    const int tile = b / BPT, e = (b - tile * BPT) * 256 + threadIdx.x;
    if (e >= PART) return;
    const int tk = tile / a.tiles_n[gi], tn = tile - tk * a.tiles_n[gi];
    const int tiles_k = wgrad_tiles_k(a.Kin[gi]);
    if (e >= WPART && tk != tiles_k - 1) return;             // the remainder tile belongs to the last tile row
    const int S = a.split[gi];
    const float* p = a.partials[gi] + (size_t)tile * S * PART + e;
    // eight rows in flight per thread (a fixed order still: the same sums in every run): the plain loop waited for every load in turn
    float v0 = 0.f, v1 = 0.f, v2 = 0.f, v3 = 0.f, v4 = 0.f, v5 = 0.f, v6 = 0.f, v7 = 0.f;
    int s = 0;
    for (; s + 8 <= S; s += 8) {
        const float* q = p + (size_t)s * PART;
        const float t0 = q[0], t1 = q[(size_t)PART], t2 = q[(size_t)2 * PART], t3 = q[(size_t)3 * PART];
        const float t4 = q[(size_t)4 * PART], t5 = q[(size_t)5 * PART], t6 = q[(size_t)6 * PART], t7 = q[(size_t)7 * PART];
        v0 += t0; v1 += t1; v2 += t2; v3 += t3; v4 += t4; v5 += t5; v6 += t6; v7 += t7;
    }
    for (; s < S; ++s) v0 += p[(size_t)s * PART];
    const float v = ((v0 + v1) + (v2 + v3)) + ((v4 + v5) + (v6 + v7));
    if (e < WT * WT) {
        const int k = tk * WT + (e >> 7), n = tn * WT + (e & (WT - 1));
        if (k < a.Kin[gi] && n < a.N[gi]) atomicAdd(a.C[gi] + (long long)k * a.ldc[gi] + n, v);
    } else if (e < WPART) {
        const int n = tn * WT + (e - WT * WT);
        if (tk == 0 && a.colsum[gi] && n < a.N[gi]) atomicAdd(a.colsum[gi] + n, v);
    } else {
        const int k = tiles_k * WT + ((e - WPART) >> 7), n = tn * WT + ((e - WPART) & (WT - 1));
        if (k < a.Kin[gi] && n < a.N[gi]) atomicAdd(a.C[gi] + (long long)k * a.ldc[gi] + n, v);
    }
}


// ------------------------------------------------------------------------------------------------------------
// Batched transposed-reduction product  C_z[Kin][N] = A_z[M][Kin]^T . B_z[M][N]  (gridDim.z members z): the construction of
// dense_wgrad_bf16x6_kernel above -- 32-row slabs of both fp32 operands split on their way into the LDS (the same row layout, the same
// transposed reads, the same six products, two buffers, the same two k-step forms: step_own with three planes) -- for products whose reduction
// is short and whose batch is long (the frequency-domain context Conv1D: M = 2 B NS rows per frequency, S rows per segment): one
// workgroup owns a whole 128 x 128 tile, so there is no split over M, no partial rows and no reduce launch; the tile goes straight
// into C, every cell guarded by the true Kin and N.  No input transforms, no bias sums, no remainder tile.
// blockIdx.x = tile (column tiles innermost), blockIdx.z = member: the tiles of a member are dispatched together.  (Regrouping the
// workgroups so that a member's tiles share one XCD's L2 was measured on the correlation: 164.5 against 168 us, not kept.)
// ------------------------------------------------------------------------------------------------------------
struct TnArgs {
    const float* A; const float* B; float* C;
    long long strideA, strideB, strideC;     // floats between batch members (strideA = 0: a shared left operand)
    long long lda, ldb, ldc;
    int Kin, N, M;
    int tiles_n;                             // 128-column tiles along N
};

template <int NPL>
__global__ __launch_bounds__(THREADS) void dense_tn_bf16x6_kernel(TnArgs g) {
    extern __shared__ __attribute__((aligned(16))) u16 lds_t[];          // [buffer][A planes 0..2 | B planes 0..2]: 96 KB
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int li = lane & 15, lg = lane >> 4;
    const int member = blockIdx.z, tile = blockIdx.x, tk = tile / g.tiles_n, tn = tile - tk * g.tiles_n;
    const int k0 = tk * WT, n0 = tn * WT;
    const int nsteps = (g.M + 31) / 32;

    // ---- staging slots as in dense_wgrad_bf16x6_kernel: float4 q = tid + 512 j (j = 0, 1) -> row q >> 5, columns 4 (q & 31) ..
    // (a quad that straddles Kin or N is loaded whole -- lda, ldb cover the rounded-up width -- and its cells beyond are never stored)
    const int c4 = tid & 31;
    const bool a_ok = k0 + 4 * c4 < g.Kin, b_ok = n0 + 4 * c4 < g.N;
    const float* pa = g.A + (long long)member * g.strideA + (a_ok ? k0 + 4 * c4 : 0);
    const float* pb = g.B + (long long)member * g.strideB + (b_ok ? n0 + 4 * c4 : 0);
    int dst[2];
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int row = (tid + j * THREADS) >> 5;
        dst[j] = row * WROW + ((((c4 >> 2) + row + 4 * (row >> 3)) & 7) << 4) + (c4 & 3) * 4;
    }
    struct Stage { f32x4 va[2], vb[2]; bool ok[2]; };
    auto load = [&](int s, Stage& sg) {
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int m = s * 32 + ((tid + j * THREADS) >> 5);
            sg.ok[j] = m < g.M;                                          // (also false for the steps behind the last)
            const long long r = sg.ok[j] ? m : 0;
            sg.va[j] = *reinterpret_cast<const f32x4*>(pa + r * g.lda);
            sg.vb[j] = *reinterpret_cast<const f32x4*>(pb + r * g.ldb);
        }
    };
    auto commit = [&](const Stage& sg, u16* ls) {
        const f32x4 z4 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            f32x4 a = sg.va[j], d = sg.vb[j];
            if (!(sg.ok[j] && a_ok)) a = z4;
            if (!(sg.ok[j] && b_ok)) d = z4;
            u16* q = ls + dst[j];
            if (NPL == 3) {
                unsigned a1, a2, a3, b1, b2, b3;
                split3_pair(a[0], a[1], a1, a2, a3);
                split3_pair(a[2], a[3], b1, b2, b3);
                *reinterpret_cast<u32x2*>(q) = (u32x2){a1, b1};
                *reinterpret_cast<u32x2*>(q + WPL) = (u32x2){a2, b2};
                *reinterpret_cast<u32x2*>(q + 2 * WPL) = (u32x2){a3, b3};
                split3_pair(d[0], d[1], a1, a2, a3);
                split3_pair(d[2], d[3], b1, b2, b3);
                q += 3 * WPL;
                *reinterpret_cast<u32x2*>(q) = (u32x2){a1, b1};
                *reinterpret_cast<u32x2*>(q + WPL) = (u32x2){a2, b2};
                *reinterpret_cast<u32x2*>(q + 2 * WPL) = (u32x2){a3, b3};
            } else {
                *reinterpret_cast<u32x2*>(q) = (u32x2){pk_bf16(a[0], a[1]), pk_bf16(a[2], a[3])};
                *reinterpret_cast<u32x2*>(q + 3 * WPL) = (u32x2){pk_bf16(d[0], d[1]), pk_bf16(d[2], d[3])};
            }
        }
    };

    // ---- MFMA tiles of this wave: A-column tiles 2 (wave & 3) + {0, 1}, B-column tiles 4 (wave >> 2) + {0..3}
    auto tr_off = [&](int t, int half) {
        const int row = 8 * lg + (li >> 2) + 4 * half;
        return row * WROW + (((t + row + 4 * (row >> 3)) & 7) << 4) + (li & 3) * 4;
    };
    int ao[2][2], bo[4][2];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
#pragma unroll
        for (int i = 0; i < 2; ++i) ao[i][h] = tr_off(2 * (wave & 3) + i, h);
#pragma unroll
        for (int i = 0; i < 4; ++i) bo[i][h] = 3 * WPL + tr_off(4 * (wave >> 2) + i, h);
    }
    f32x4 acc[2][4];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
    auto mfma_tile_row = [&](const u16* ls, int i, const bf16x8 (&bf)[4][NPL]) {
        bf16x8 af[NPL];
#pragma unroll
        for (int p = 0; p < NPL; ++p) af[p] = cat8(tr_read(ls + p * WPL + ao[i][0]), tr_read(ls + p * WPL + ao[i][1]));
#define DNS_MM(PA, PW)                                                                                       \
        _Pragma("unroll") for (int j = 0; j < 4; ++j)                                                        \
            acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[PA < NPL ? PA : 0], bf[j][PW < NPL ? PW : 0], acc[i][j], 0, 0, 0);
        DNS_PRODUCTS_NPL(NPL, DNS_MM);
#undef DNS_MM
    };
    auto read_bf = [&](const u16* ls, bf16x8 (&bf)[4][NPL]) {
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int p = 0; p < NPL; ++p) bf[j][p] = cat8(tr_read(ls + p * WPL + bo[j][0]), tr_read(ls + p * WPL + bo[j][1]));
    };

    u16* const buf0 = lds_t;
    u16* const buf1 = lds_t + 6 * WPL;
    Stage sg;
    load(0, sg);
    commit(sg, buf0);
    load(1, sg);
    __syncthreads();
    auto step = [&](int s, const u16* cur, u16* nxt, bool stage_first) {
        bf16x8 bf[4][NPL];
        if (stage_first) { commit(sg, nxt); load(s + 2, sg); }
        read_bf(cur, bf);
        mfma_tile_row(cur, 0, bf);
        if (!stage_first) { commit(sg, nxt); load(s + 2, sg); }
        mfma_tile_row(cur, 1, bf);
        __syncthreads();
    };
    // three planes: dense_wgrad_bf16x6_kernel's step_own
    auto step_own = [&](int s, const u16* cur, u16* nxt) {
        if constexpr (NPL == 3) {
            using ST = StageSlices<PTTS_IN_NONE, false, false, WPL>;
            ST st;
            st.begin(sg.va, nullptr, sg.vb);
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                st.ok[j] = sg.ok[j] && a_ok; st.ok[2 + j] = sg.ok[j] && b_ok;
                st.dst[j] = nxt + dst[j]; st.dst[2 + j] = nxt + dst[j] + 3 * WPL;
            }
            f32x4 none = {0.f, 0.f, 0.f, 0.f};
            tn_step_own(cur, ao, bo, acc, st, none, [&]() { load(s + 2, sg); });
            __syncthreads();
        }
    };
    if (NPL == 3) {
        int s = 0;
        for (; s + 1 < nsteps; s += 2) { step_own(s, buf0, buf1); step_own(s + 1, buf1, buf0); }
        if (s < nsteps) step_own(s, buf0, buf1);
    } else if (wave < 4) {
        int s = 0;
        for (; s + 1 < nsteps; s += 2) { step(s, buf0, buf1, false); step(s + 1, buf1, buf0, false); }
        if (s < nsteps) step(s, buf0, buf1, false);
    } else {
        int s = 0;
        for (; s + 1 < nsteps; s += 2) { step(s, buf0, buf1, true); step(s + 1, buf1, buf0, true); }
        if (s < nsteps) step(s, buf0, buf1, true);
    }

    // ---- the tile, straight from the accumulators: lane (li, lg) of acc[i][j] holds rows k = 32 (wave & 3) + 16 i + 4 lg + r, column
    // 64 (wave >> 2) + 16 j + li, so one store instruction writes 64-byte segments of four rows; the four j of a row are issued back to
    // back and complete 256 contiguous bytes of it
    float* out = g.C + (long long)member * g.strideC;
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int k = k0 + 32 * (wave & 3) + 16 * i + 4 * lg + r;
            if (k >= g.Kin) continue;
            float* row = out + (long long)k * g.ldc;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int n = n0 + 64 * (wave >> 2) + 16 * j + li;
                if (n < g.N) row[n] = acc[i][j][r];
            }
        }
}

}  // namespace dns
}  // namespace ptts

using namespace ptts;
using namespace ptts::dns;

// bytes of the three planes of a [K][N] operand (N rounded up to 256 columns, K to 32)
extern "C" size_t ptts_dense_planes_bytes(int N, int K) {
    if (N <= 0 || K <= 0) return 0;
    const size_t NT = (size_t)((N + NBLK - 1) / NBLK) * (NBLK / 16), KS = (size_t)(K + BK - 1) / BK;
    return 3 * NT * KS * 512 * sizeof(u16);
}

// planes of B[K][N]: transposed == 0 reads w as [K][N] (row stride ldw), transposed == 1 as [N][K]
extern "C" int ptts_split3_dense_weight(const float* w, long long ldw, int K, int N, int transposed, void* planes, void* stream) {
    PTTS_REQUIRE(w && planes, "split3_dense_weight: null pointer");
    PTTS_REQUIRE(K > 0 && N > 0 && ldw >= (transposed ? K : N), "split3_dense_weight: bad dims K=%d N=%d ldw=%lld", K, N, ldw);
    const int NT = (N + NBLK - 1) / NBLK * (NBLK / 16), KS = (K + BK - 1) / BK;
    const long long total = (long long)NT * KS * 64;
    hipLaunchKernelGGL(split3_dense_weight_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                       w, ldw, K, N, transposed, (u16*)planes, NT, KS);
    return check_launch("split3_dense_weight");
}

extern "C" int ptts_split3_dense_weight_grouped(const ptts_dense_split_desc* descs, int n, void* stream) {
    PTTS_REQUIRE(descs && n > 0, "split3_dense_weight_grouped: nothing to split");
    for (int base = 0; base < n; base += SPLIT_GROUP) {
        SplitGroupArgs a;
        const int m = n - base < SPLIT_GROUP ? n - base : SPLIT_GROUP;
        long long most = 0;
        for (int i = 0; i < m; ++i) {
            const ptts_dense_split_desc& d = descs[base + i];
            PTTS_REQUIRE(d.w && d.planes, "split3_dense_weight_grouped: null pointer (weight %d)", base + i);
            PTTS_REQUIRE(d.K > 0 && d.N > 0 && d.ldw >= (d.transposed ? d.K : d.N), "split3_dense_weight_grouped: bad dims K=%d N=%d ldw=%lld (weight %d)", d.K, d.N, d.ldw, base + i);
            a.w[i] = d.w; a.planes[i] = (u16*)d.planes; a.ldw[i] = d.ldw; a.K[i] = d.K; a.N[i] = d.N; a.transposed[i] = d.transposed;
            a.rlo[i] = 0; a.rhi[i] = d.K;
            a.NT[i] = (d.N + NBLK - 1) / NBLK * (NBLK / 16); a.KS[i] = (d.K + BK - 1) / BK;
            const long long total = (long long)a.NT[i] * a.KS[i] * 64;
            if (total > most) most = total;
        }
        hipLaunchKernelGGL(split3_dense_weight_grouped_kernel, dim3((unsigned)((most + 255) / 256), (unsigned)m), dim3(256), 0, (hipStream_t)stream, a);
    }
    return check_launch("split3_dense_weight_grouped");
}

// n weights of one shape at regular strides (w + i * stride_w floats -> planes + i * stride_planes_bytes): the operands of the
// batched products, without a descriptor array on the host side
extern "C" int ptts_split3_dense_weight_strided(const float* w, long long stride_w, void* planes, long long stride_planes_bytes, int n,
                                                long long ldw, int K, int N, int transposed, void* stream) {
    PTTS_REQUIRE(w && planes && n > 0 && n <= 65535, "split3_dense_weight_strided: nothing to split (or more than 65535 matrices)");
    PTTS_REQUIRE(K > 0 && N > 0 && ldw >= (transposed ? K : N), "split3_dense_weight_strided: bad dims K=%d N=%d ldw=%lld", K, N, ldw);
    PTTS_REQUIRE(stride_planes_bytes % 16 == 0, "split3_dense_weight_strided: the planes' stride must keep 16-byte alignment");
    SplitStridedArgs a;
    a.w = w; a.planes = (u16*)planes; a.stride_w = stride_w; a.stride_p = stride_planes_bytes / 2; a.ldw = ldw;
    a.K = K; a.N = N; a.transposed = transposed;
    a.NT = (N + NBLK - 1) / NBLK * (NBLK / 16); a.KS = (K + BK - 1) / BK;
    a.windows = 0; a.T = a.NS = a.S = a.row_off = a.kvalid = 0;
    const long long total = (long long)a.NT * a.KS * 64;
    static int lds_form = -1;
    if (lds_form < 0) { const char* e = getenv("PTTS_SPLIT_LDS"); lds_form = e ? atoi(e) : 1; }
    if (lds_form && !transposed && N % 4 == 0 && ldw % 4 == 0 && stride_w % 4 == 0 && ((uintptr_t)w & 15) == 0) {
        const unsigned cbn = (unsigned)((N + 255) / 256);
        hipLaunchKernelGGL(split3_dense_weight_strided_lds_kernel, dim3((unsigned)a.KS * cbn, (unsigned)n), dim3(256), 0, (hipStream_t)stream, a);
        return check_launch("split3_dense_weight_strided");
    }
    hipLaunchKernelGGL(split3_dense_weight_strided_kernel, dim3((unsigned)((total + 255) / 256), (unsigned)n), dim3(256), 0, (hipStream_t)stream, a);
    return check_launch("split3_dense_weight_strided");
}

// Planes of WINDOWS of frame sequences x [B][T][C]: matrix z = b NS + s is the P rows x[b][row_off + s S + k][:], k < P, zero for rows
// outside [0, T) and for k >= kvalid (the segments of an overlap-save convolution: a window of S + KW - 1 input frames per S output
// frames; a block of S gradient frames zero-padded to P).  planes + z stride_planes_bytes, ptts_dense_planes_bytes(C, P) each.
extern "C" int ptts_split3_frame_windows(const float* x, int B, int T, int C, int NS, int S, int row_off, int P, int kvalid,
                                         void* planes, long long stride_planes_bytes, void* stream) {
    PTTS_REQUIRE(x && planes && B > 0 && T > 0 && C > 0 && NS > 0 && S > 0 && P > 0 && kvalid > 0 && kvalid <= P, "split3_frame_windows: bad arguments");
    PTTS_REQUIRE((long long)B * NS <= 65535 && stride_planes_bytes % 16 == 0, "split3_frame_windows: more than 65535 windows, or a planes stride off 16-byte alignment");
    SplitStridedArgs a;
    a.w = x; a.planes = (u16*)planes; a.stride_w = 0; a.stride_p = stride_planes_bytes / 2; a.ldw = C;
    a.K = P; a.N = C; a.transposed = 0;
    a.NT = (C + NBLK - 1) / NBLK * (NBLK / 16); a.KS = (P + BK - 1) / BK;
    a.windows = 1; a.T = T; a.NS = NS; a.S = S; a.row_off = row_off; a.kvalid = kvalid;
    const long long total = (long long)a.NT * a.KS * 64;
    hipLaunchKernelGGL(split3_dense_weight_strided_kernel, dim3((unsigned)((total + 255) / 256), (unsigned)(B * NS)), dim3(256), 0, (hipStream_t)stream, a);
    return check_launch("split3_frame_windows");
}

// 1 when ptts_dense_bf16x6 takes the shape
extern "C" int ptts_dense_bf16x6_supported(int M, int N, int K, long long lda, long long ldc) {
    (void)ldc;                                    // any N / ldc: rows that are no multiple of 4 floats are stored element-wise
    return (M > 0 && N > 0 && K > 0 && K % 4 == 0 && lda % 4 == 0 && K <= 65536 &&
            (long long)((N + NBLK - 1) / NBLK) <= 65535) ? 1 : 0;
}

// C[M,N] (+)= T(A)[M,K] . B (+ bias), then C *= (out_mask > 0 ? 1 : alpha) -- the contract of ptts_gemm with transA = 0 and
// B given as the planes of ptts_split3_dense_weight.  in_mode / in_scale / in_shift / mask_src / alpha as in ptts_gemm.
// extra_tile: 1..16 columns beyond a multiple of 256 run as a 17th column tile of the last column block (dense_bf16x6_kernel<.., XT>).
// Only the plain entry point asks for it; the others keep their whole column blocks.
static int dense_launch(const float* A, const void* planes, const float* bias, float* C, int M, int N, int K,
                        long long lda, long long ldc, int in_mode, const float* in_scale, const float* in_shift,
                        const float* mask_src, float alpha, const float* res, int res_rows, long long ldr,
                        const float* out_mask, double* stats, int stats_capacity_rows, int* stats_rows_out, void* stream,
                        bool extra_tile = false);
extern "C" int ptts_dense_bf16x6(const float* A, const void* planes, const float* bias, float* C, int M, int N, int K,
                                 long long lda, long long ldc, int in_mode, const float* in_scale, const float* in_shift,
                                 const float* mask_src, float alpha, int accumulate, const float* out_mask, void* stream) {
    return dense_launch(A, planes, bias, C, M, N, K, lda, ldc, in_mode, in_scale, in_shift, mask_src, alpha,
                        accumulate ? C : nullptr, M, ldc, out_mask, nullptr, 0, nullptr, stream, true);
}

// ... + res[m % res_rows][n] (row stride ldr) in the store: the product of a concat part that several stacked evaluations share (the
// critic's context branch, computed once at B rows) joins each of the k B-row blocks of the stacked product without an add pass of its
// own.  res == C, res_rows >= M is the plain accumulate of ptts_dense_bf16x6.
static thread_local const float* g_om_scale = nullptr;        // (set around dense_launch by ptts_dense_bf16x6_bwd_affine)
static thread_local const float* g_om_shift = nullptr;

extern "C" int ptts_dense_bf16x6_res(const float* A, const void* planes, const float* bias, float* C, int M, int N, int K,
                                     long long lda, long long ldc, int in_mode, const float* in_scale, const float* in_shift,
                                     const float* mask_src, float alpha, const float* res, int res_rows, long long ldr,
                                     const float* out_mask, void* stream) {
    return dense_launch(A, planes, bias, C, M, N, K, lda, ldc, in_mode, in_scale, in_shift, mask_src, alpha, res, res_rows, ldr, out_mask,
                        nullptr, 0, nullptr, stream);
}

// The product of a Dense layer that feeds a BatchNormalization layer (pFC, reference networktts.py:59-63): the launch also leaves, per
// row tile, the column sums and the column sums of squares of what it stores -- stats[*nrows_out][2 N] doubles -- which
// ptts_bn_finalize_partials finishes: no statistics pass over the [M, N] activation (ptts_colstats: two launches, 16 us at 25 600 x 256).
extern "C" int ptts_dense_bf16x6_stats(const float* A, const void* planes, const float* bias, float* C, int M, int N, int K,
                                       long long lda, long long ldc, int in_mode, const float* in_scale, const float* in_shift,
                                       float alpha, double* stats, int capacity_rows, int* nrows_out, void* stream) {
    PTTS_REQUIRE(stats && nrows_out && capacity_rows > 0, "dense_bf16x6_stats: no room for the sums");
    return dense_launch(A, planes, bias, C, M, N, K, lda, ldc, in_mode, in_scale, in_shift, nullptr, alpha, nullptr, 0, 0, nullptr,
                        stats, capacity_rows, nrows_out, stream);
}
// Backward-data product of a Dense layer whose input was lrelu(scale z + shift) (a BatchNormalization in front: pFC, networktts.py:59-63):
// C = dz = (A . B) lrelu'(scale z + shift) scale with A = dy, B = W^T (planes of the transposed kernel), and per row tile the column sums
// of (A . B) lrelu'(.) z and of (A . B) lrelu'(.) -- the gradients of scale and shift -- as stats[*nrows_out][2 N] doubles
// (ptts_partial_rows_sum adds the rows).  Replaces the product + ptts_affine_act_bwd's pass over da and z.
extern "C" int ptts_dense_bf16x6_bwd_affine(const float* A, const void* planes, float* C, int M, int N, int K, long long lda, long long ldc,
                                            const float* z, const float* scale, const float* shift, float alpha,
                                            double* stats, int capacity_rows, int* nrows_out, void* stream) {
    PTTS_REQUIRE(z && scale && shift && stats && nrows_out && capacity_rows > 0, "dense_bf16x6_bwd_affine: null pointer");
    PTTS_REQUIRE((((uintptr_t)scale | (uintptr_t)shift) & 15) == 0, "dense_bf16x6_bwd_affine: scale / shift must be 16-byte aligned");
    g_om_scale = scale; g_om_shift = shift;
    const int rc = dense_launch(A, planes, nullptr, C, M, N, K, lda, ldc, PTTS_IN_NONE, nullptr, nullptr, nullptr, alpha, nullptr, 0, 0, z,
                                stats, capacity_rows, nrows_out, stream);
    g_om_scale = g_om_shift = nullptr;
    return rc;
}
// rows of sums ptts_dense_bf16x6_stats writes for an [M, N] product (the caller's capacity)
extern "C" int ptts_dense_bf16x6_stats_rows(int M, int N) {
    if (M <= 0 || N <= 0) return 0;
    const int mt = pick_mt(M, (N + NBLK - 1) / NBLK);
    return (M + 16 * mt - 1) / (16 * mt);
}

static int dense_launch(const float* A, const void* planes, const float* bias, float* C, int M, int N, int K,
                        long long lda, long long ldc, int in_mode, const float* in_scale, const float* in_shift,
                        const float* mask_src, float alpha, const float* res, int res_rows, long long ldr,
                        const float* out_mask, double* stats, int stats_capacity_rows, int* stats_rows_out, void* stream,
                        bool extra_tile) {
    const int accumulate = res != nullptr;
    PTTS_REQUIRE(!res || (res_rows > 0 && ldr >= N && M <= 8LL * res_rows), "dense_bf16x6: bad residual (rows %d, ldr %lld)", res_rows, ldr);
    PTTS_REQUIRE(A && planes && C, "dense_bf16x6: null matrix");
    PTTS_REQUIRE(ptts_dense_bf16x6_supported(M, N, K, lda, ldc), "dense_bf16x6: unsupported shape M=%d N=%d K=%d lda=%lld ldc=%lld (K and lda must be multiples of 4)", M, N, K, lda, ldc);
    PTTS_REQUIRE(lda >= K && ldc >= N, "dense_bf16x6: bad leading dims");
    PTTS_REQUIRE(in_mode >= 0 && in_mode <= 2, "dense_bf16x6: bad in_mode %d", in_mode);
    PTTS_REQUIRE((in_scale == nullptr) == (in_shift == nullptr), "dense_bf16x6: scale/shift must come together");
    PTTS_REQUIRE(in_mode != PTTS_IN_MASKMUL || mask_src, "dense_bf16x6: MASKMUL needs mask_src");
    PTTS_REQUIRE(in_mode == PTTS_IN_LRELU || !in_scale, "dense_bf16x6: scale/shift need PTTS_IN_LRELU");
    PTTS_REQUIRE(!(out_mask && bias), "dense_bf16x6: out_mask with bias is not defined");
    PTTS_REQUIRE(alpha >= 0.f && alpha <= 1.f, "dense_bf16x6: LeakyReLU slope %g outside [0, 1]", alpha);
    const bool vec_out = N % 4 == 0 && ldc % 4 == 0 && ((uintptr_t)C & 15) == 0 && (!bias || ((uintptr_t)bias & 15) == 0) &&
                         (!out_mask || ((uintptr_t)out_mask & 15) == 0) && (!res || (((uintptr_t)res & 15) == 0 && ldr % 4 == 0));
    PTTS_REQUIRE(((uintptr_t)A & 15) == 0 && (!mask_src || ((uintptr_t)mask_src & 15) == 0) &&
                 (!in_scale || (((uintptr_t)in_scale | (uintptr_t)in_shift) & 15) == 0), "dense_bf16x6: A, its mask and scale/shift must be 16-byte aligned");
    DenseArgs g;
    g.A = A; g.mask_src = mask_src; g.in_scale = in_scale; g.in_shift = in_shift; g.planes = (const u16*)planes; g.bias = bias;
    g.out_mask = out_mask; g.C = C; g.M = M; g.N = N; g.K = K;
    g.NT = (N + NBLK - 1) / NBLK * (NBLK / 16); g.KS = (K + BK - 1) / BK;
    g.lda = lda; g.ldc = ldc; g.alpha = alpha; g.out_alpha = alpha; g.accumulate = accumulate; g.has_affine = in_scale != nullptr; g.vec_out = vec_out;
    g.res = res; g.res_rows = res ? res_rows : 1; g.ldr = ldr;
    g.bsA = g.bsP = g.bsC = 0;
    const bool xt = extra_tile && !stats && !g_om_scale && N > NBLK && N % NBLK >= 1 && N % NBLK <= 16;
    const int cb = xt ? N / NBLK : (N + NBLK - 1) / NBLK;
    int mt = pick_mt(M, cb);
    if (xt && mt == 8) mt = 7;                                // (dense_launch_kernel)
    const dim3 grid((unsigned)((M + 16 * mt - 1) / (16 * mt)), (unsigned)cb);
    g.stats = stats;
    g.om_scale = g_om_scale; g.om_shift = g_om_shift;
    if (stats) {
        PTTS_REQUIRE(vec_out, "dense_bf16x6_stats: N and ldc must be multiples of 4, C (and bias) 16-byte aligned");
        PTTS_REQUIRE(stats_capacity_rows >= (int)grid.x, "dense_bf16x6_stats: room for %d rows of sums, %d needed", stats_capacity_rows, (int)grid.x);
        *stats_rows_out = (int)grid.x;
    }
    hipStream_t st = (hipStream_t)stream;
    const bool one = ptts::bf16_products();
#define DNS_L(MODE, AFF, MT) do { if (one) dense_launch_kernel<MODE, AFF, MT, 1>(xt, grid, st, g); \
                                  else dense_launch_kernel<MODE, AFF, MT, 3>(xt, grid, st, g); } while (0)
#define DNS_M(MT)                                                                \
    do {                                                                         \
        if (in_mode == PTTS_IN_LRELU) { if (in_scale) DNS_L(PTTS_IN_LRELU, true, MT); else DNS_L(PTTS_IN_LRELU, false, MT); } \
        else if (in_mode == PTTS_IN_MASKMUL) DNS_L(PTTS_IN_MASKMUL, false, MT);  \
        else DNS_L(PTTS_IN_NONE, false, MT);                                     \
    } while (0)
    switch (mt) {
        case 4: DNS_M(4); break;
        case 5: DNS_M(5); break;
        case 6: DNS_M(6); break;
        case 7: DNS_M(7); break;
        default: DNS_M(8); break;
    }
#undef DNS_M
#undef DNS_L
    return check_launch("dense_bf16x6");
}

// planes of [Wr_f ; Wi_f] [2 Kh][N] for f = 0 .. NB-1 (each ptts_dense_planes_bytes(N, 2 Kh) long) from the kernel w [KW][Cin][N] and
// the twiddle rows tw [(f, part)][KW] = cos / -sin(2 pi f (pl - k) / P)
extern "C" int ptts_conv1d_freq_kernel_planes(const float* w, const float* tw, void* planes, int NB, int KW, int Cin, int N, int Kh,
                                              void* stream) {
    PTTS_REQUIRE(w && tw && planes && NB > 0 && Cin > 0 && N > 0, "conv1d_freq_kernel_planes: bad arguments");
    PTTS_REQUIRE(Kh >= Cin && Kh % 8 == 0, "conv1d_freq_kernel_planes: Kh=%d must be a multiple of 8 and >= Cin=%d", Kh, Cin);
    const int NT = (N + NBLK - 1) / NBLK * (NBLK / 16), KS = (2 * Kh + BK - 1) / BK;
    const long long total = (long long)NT * KS * 64;
    const long long fstride = (long long)(ptts_dense_planes_bytes(N, 2 * Kh) / sizeof(u16));
    const dim3 grid((unsigned)((total + 255) / 256), (unsigned)((NB + WDFT_FCH - 1) / WDFT_FCH));
#define WDFT(KWv) hipLaunchKernelGGL(conv1d_wdft_planes_kernel<KWv>, grid, dim3(256), 0, (hipStream_t)stream, w, tw, (u16*)planes, fstride, NB, Cin, N, Kh, NT, KS)
    switch (KW) {
        case 3: WDFT(3); break;
        case 5: WDFT(5); break;
        case 7: WDFT(7); break;
        case 9: WDFT(9); break;
        case 11: WDFT(11); break;
        case 21: WDFT(21); break;
        default: set_error("conv1d_freq_kernel_planes: KW=%d not instantiated (3, 5, 7, 9, 11, 21)", KW); return PTTS_EINVAL;
    }
#undef WDFT
    return check_launch("conv1d_freq_kernel_planes");
}

// ---- the resident-left form of the batched product (dense_bf16x6_resident_kernel) ----------------------------------------------
// PTTS_DENSE_BATCHED_RESIDENT=0 (read once) or ptts_set_dense_batched_resident(0): every batched product on dense_bf16x6_kernel
static int g_batched_resident = -1;
static int batched_resident_on() {
    if (g_batched_resident < 0) { const char* e = getenv("PTTS_DENSE_BATCHED_RESIDENT"); g_batched_resident = e ? (atoi(e) != 0 ? 1 : 0) : 1; }
    return g_batched_resident;
}
extern "C" int ptts_set_dense_batched_resident(int on) {
    const int prev = batched_resident_on();
    g_batched_resident = on ? 1 : 0;
    return prev;
}
extern "C" int ptts_dense_batched_resident_enabled(void) { return batched_resident_on(); }
extern "C" int ptts_dense_batched_resident_eligible(long long strideA, int M, int N, int K, int planes_count) {
    return (strideA == 0 && M > 0 && M <= RES_M && N > 0 && K > 0 && K <= RES_K && K % 4 == 0 &&
            (planes_count == 1 || planes_count == 3)) ? 1 : 0;
}

template <int NPL, int MT, bool ROWS>
static void resident_set_lds() {
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&dense_bf16x6_resident_kernel<NPL, MT, 0, ROWS>), hipFuncAttributeMaxDynamicSharedMemorySize,
                              (int)resident_lds_bytes<NPL>());
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&dense_bf16x6_resident_kernel<NPL, MT, RES_KS, ROWS>), hipFuncAttributeMaxDynamicSharedMemorySize,
                              (int)resident_lds_bytes<NPL>());
    if constexpr (MT > 1) resident_set_lds<NPL, MT - 1, ROWS>();
}
// compute units of the current device (asked once per device; the first call also raises the kernels' LDS limit there); 0: error set
static int resident_cus() {
    constexpr int MAXDEV = 64;
    static int cus[MAXDEV];
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= MAXDEV) { set_error("dense_bf16x6_batched: no current device"); return 0; }
    if (!cus[dev]) {
        int n = 0;
        if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n <= 0) {
            set_error("dense_bf16x6_batched: the device does not tell its compute units"); return 0;
        }
        resident_set_lds<3, RES_M / 16, false>();
        resident_set_lds<1, RES_M / 16, false>();
        resident_set_lds<3, RES_M / 16, true>();
        resident_set_lds<1, RES_M / 16, true>();
        cus[dev] = n;
    }
    return cus[dev];
}
// g as ptts_dense_bf16x6_batched filled it; items = nbatch x 32-column slices; rows: the fp32-rows form of the right operand, or NULL
static int resident_launch(DenseArgs g, int slices, int items, int planes_count, const RowsArgs* rows, hipStream_t st) {
    const int cus = resident_cus();
    if (!cus) return PTTS_ELAUNCH;
    const int wgs = (items + 7) / 8;
    const dim3 grid((unsigned)(wgs < cus ? wgs : cus));
    const RowsArgs r = rows ? *rows : RowsArgs{};
#define DNS_RKR(NPL, MT, KSC) do { if (rows) hipLaunchKernelGGL((dense_bf16x6_resident_kernel<NPL, MT, KSC, true>), grid, dim3(THREADS), resident_lds_bytes<NPL>(), st, g, slices, items, r); \
                                   else hipLaunchKernelGGL((dense_bf16x6_resident_kernel<NPL, MT, KSC, false>), grid, dim3(THREADS), resident_lds_bytes<NPL>(), st, g, slices, items, r); } while (0)
#define DNS_RK(NPL, MT) do { if (g.KS == RES_KS) DNS_RKR(NPL, MT, RES_KS); else DNS_RKR(NPL, MT, 0); } while (0)
#define DNS_R(MT) do { if (planes_count == 1) DNS_RK(1, MT); else DNS_RK(3, MT); } while (0)
    switch ((g.M + 15) / 16) {
        case 1: DNS_R(1); break;
        case 2: DNS_R(2); break;
        case 3: DNS_R(3); break;
        case 4: DNS_R(4); break;
        case 5: DNS_R(5); break;
        case 6: DNS_R(6); break;
        case 7: DNS_R(7); break;
        default: DNS_R(8); break;
    }
#undef DNS_R
#undef DNS_RK
#undef DNS_RKR
    return check_launch("dense_bf16x6_batched");
}

// nbatch products C_z[M,N] = A_z[M,K] . B_z (+ bias) of ONE shape in one launch (blockIdx.z = z): A_z = A + z strideA, C_z = C + z strideC
// (floats; strideA = 0: the same left operand for every product), B_z = the planes at planes + z stride_planes_bytes.  No input
// transform, no masks.  planes_count: 3 = fp32 arithmetic (six products), 1 = one bf16 product -- explicit here, whatever
// ptts_set_bf16_products says.  What the frequency-domain context Conv1D is made of (ops._C1FFT): DFT, per-frequency products, inverse DFT.
// planes_count | PTTS_PLANES_ROWS: `planes` is a HOST pointer to one ptts_dense_rows_desc, read here -- B_z as fp32 rows (strided, or the
// windows of a frame sequence) that the resident-left kernel reads and splits itself, with the mirrored store if asked for; on a shape
// or a switch setting that does not take that kernel: PTTS_EINVAL, nothing launched.
extern "C" int ptts_dense_bf16x6_batched(const float* A, long long strideA, const void* planes, long long stride_planes_bytes,
                                         const float* bias, float* C, long long strideC, int nbatch, int M, int N, int K,
                                         long long lda, long long ldc, int planes_count, void* stream) {
    const bool rows = (planes_count & PTTS_PLANES_ROWS) != 0;         // `planes` is a host ptts_dense_rows_desc: the right operand as fp32 rows
    planes_count &= ~PTTS_PLANES_ROWS;
    PTTS_REQUIRE(A && planes && C && nbatch > 0 && nbatch <= 65535, "dense_bf16x6_batched: bad arguments");
    PTTS_REQUIRE(ptts_dense_bf16x6_supported(M, N, K, lda, ldc), "dense_bf16x6_batched: unsupported shape M=%d N=%d K=%d lda=%lld ldc=%lld", M, N, K, lda, ldc);
    PTTS_REQUIRE(lda >= K && ldc >= N && planes_count >= 1 && planes_count <= 3 && planes_count != 2, "dense_bf16x6_batched: bad leading dims / planes");
    PTTS_REQUIRE((rows || stride_planes_bytes % 16 == 0) && strideA % 4 == 0 && ((uintptr_t)A & 15) == 0, "dense_bf16x6_batched: strides of A / planes must keep 16-byte alignment");
    RowsArgs ra = {};
    if (rows) {
        const ptts_dense_rows_desc& d = *(const ptts_dense_rows_desc*)planes;
        PTTS_REQUIRE(batched_resident_on() && ptts_dense_batched_resident_eligible(strideA, M, N, K, planes_count),
                     "dense_bf16x6_batched: the fp32-rows form of the right operand exists on the resident-left kernel only (strideA == 0, M <= %d, K <= %d, "
                     "the switch on): strideA=%lld M=%d K=%d", RES_M, RES_K, strideA, M, K);
        PTTS_REQUIRE(d.B && d.ldb >= N && d.kvalid > 0 && d.kvalid <= K, "dense_bf16x6_batched: rows form: bad source, ldb=%lld or kvalid=%d", d.ldb, d.kvalid);
        // the last float a lane may read lies below 2^30 (32-bit byte offsets from d.B)
        long long span;
        if (d.windows) {
            PTTS_REQUIRE(d.nB > 0 && d.T > 0 && d.NS > 0 && d.S > 0 && (long long)d.nB * d.NS == nbatch && d.row_off > -(1 << 24) && d.row_off < (1 << 24),
                         "dense_bf16x6_batched: rows form: bad windows nB=%d T=%d NS=%d S=%d row_off=%d for %d members", d.nB, d.T, d.NS, d.S, d.row_off, nbatch);
            span = ((long long)d.nB * d.T - 1) * d.ldb + N;
        } else {
            PTTS_REQUIRE(d.strideB >= 0, "dense_bf16x6_batched: rows form: negative strideB");
            span = (long long)(nbatch - 1) * d.strideB + (long long)(d.kvalid - 1) * d.ldb + N;
        }
        PTTS_REQUIRE(span <= (1LL << 30), "dense_bf16x6_batched: rows form: the source spans more than 2^30 floats");
        PTTS_REQUIRE(d.mirror_cols >= 0 && (d.mirror_cols == 0 || (d.mirror_cols % 4 == 0 && d.mirror_cols >= N && (long long)d.mirror_cols + N <= ldc && M % 2 == 0)),
                     "dense_bf16x6_batched: rows form: mirror_cols=%d needs a multiple of 4, N <= mirror_cols, mirror_cols + N <= ldc and an even M", d.mirror_cols);
        ra.B = d.B; ra.strideB = d.strideB; ra.ldb = (int)d.ldb; ra.windows = d.windows ? 1 : 0;
        ra.T = d.T; ra.NS = d.NS; ra.S = d.S; ra.row_off = d.row_off; ra.kvalid = d.kvalid; ra.mirror = d.mirror_cols;
    }
    const bool vec_out = N % 4 == 0 && ldc % 4 == 0 && strideC % 4 == 0 && ((uintptr_t)C & 15) == 0 && (!bias || ((uintptr_t)bias & 15) == 0);
    DenseArgs g;
    g.A = A; g.mask_src = nullptr; g.in_scale = nullptr; g.in_shift = nullptr; g.planes = (const u16*)planes; g.bias = bias;
    g.out_mask = nullptr; g.C = C; g.M = M; g.N = N; g.K = K;
    g.NT = (N + NBLK - 1) / NBLK * (NBLK / 16); g.KS = (K + BK - 1) / BK;
    g.lda = lda; g.ldc = ldc; g.alpha = 0.f; g.out_alpha = 0.f; g.accumulate = 0; g.has_affine = 0; g.vec_out = vec_out;
    g.res = nullptr; g.res_rows = 1; g.ldr = 0;
    g.bsA = strideA; g.bsP = stride_planes_bytes / 2; g.bsC = strideC;
    g.stats = nullptr; g.om_scale = g.om_shift = nullptr;
    // a shared left operand of at most 128 x 128 stays in the LDS and the waves walk (member, 32-column slice) items (the transforms of
    // the frequency-domain Conv1D are the callers with strideA == 0); the same bits as the kernel below
    const long long items = (long long)nbatch * ((N + 31) / 32);
    if (batched_resident_on() && ptts_dense_batched_resident_eligible(strideA, M, N, K, planes_count) && items <= 0x3fffffffLL) {     // (item + 8 G stays an int)
        g.vec_out = ldc % 4 == 0 && strideC % 4 == 0 && ((uintptr_t)C & 15) == 0 && (!bias || ((uintptr_t)bias & 15) == 0);      // (per quad: n + 3 < N)
        if (rows) g.planes = nullptr;
        return resident_launch(g, (N + 31) / 32, (int)items, planes_count, rows ? &ra : nullptr, (hipStream_t)stream);
    }
    PTTS_REQUIRE(!rows, "dense_bf16x6_batched: rows form: too many work items");
    const int cb = (N + NBLK - 1) / NBLK;
    // rows per workgroup: every workgroup of a product reads that product's planes, so fewer row tiles = fewer reads of the right
    // operand, which is most of the traffic of these small-M products
    int mt = 8; double best_eff = -1.0;
    {
        static int forced = -1;
        if (forced < 0) { const char* e = getenv("PTTS_DENSE_BATCHED_MT"); forced = e ? atoi(e) : 0; }
        for (int m = 8; m >= 4; --m) {          // least row padding, then the taller tile (measured: 134 / 183 us against 163 / 213 for the
            const int tiles = (M + 16 * m - 1) / (16 * m);      // round-filling choice of pick_mt on the per-frequency products)
            const double eff = (double)M / (double)(tiles * 16 * m);
            if (eff > best_eff + 1e-9) { best_eff = eff; mt = m; }
        }
        if (forced >= 4 && forced <= 8) mt = forced;
    }
    const dim3 grid((unsigned)((M + 16 * mt - 1) / (16 * mt)), (unsigned)cb, (unsigned)nbatch);
    hipStream_t st = (hipStream_t)stream;
    const bool one = planes_count == 1;
#define DNS_B(MT) do { if (one) hipLaunchKernelGGL((dense_bf16x6_kernel<PTTS_IN_NONE, false, MT, 1>), grid, dim3(THREADS), 0, st, g); \
                       else hipLaunchKernelGGL((dense_bf16x6_kernel<PTTS_IN_NONE, false, MT, 3>), grid, dim3(THREADS), 0, st, g); } while (0)
    switch (mt) {
        case 4: DNS_B(4); break;
        case 5: DNS_B(5); break;
        case 6: DNS_B(6); break;
        case 7: DNS_B(7); break;
        default: DNS_B(8); break;
    }
#undef DNS_B
    return check_launch("dense_bf16x6_batched");
}

// nbatch products C_z[Kin,N] = A_z[M,Kin]^T . B_z[M,N] of ONE shape in one launch (dense_tn_bf16x6_kernel): both operands fp32,
// row-major, read once and split in the kernel -- for right operands that are activations used once, which ptts_dense_bf16x6_batched
// wants pre-split.  Kin and N are the store guards; the operands are read in quads, so lda / ldb cover Kin / N rounded up to 4.
extern "C" int ptts_dense_tn_bf16x6_batched(const float* A, long long strideA, const float* B, long long strideB, float* C,
                                            long long strideC, int nbatch, int M, int Kin, int N, long long lda, long long ldb,
                                            long long ldc, int planes_count, void* stream) {
    PTTS_REQUIRE(A && B && C && nbatch > 0 && nbatch <= 65535, "dense_tn_bf16x6_batched: bad arguments");
    PTTS_REQUIRE(M > 0 && Kin > 0 && N > 0, "dense_tn_bf16x6_batched: bad shape M=%d Kin=%d N=%d", M, Kin, N);
    PTTS_REQUIRE(planes_count == 1 || planes_count == 3, "dense_tn_bf16x6_batched: planes_count %d is neither 1 nor 3", planes_count);
    PTTS_REQUIRE(lda >= (Kin + 3) / 4 * 4 && ldb >= (N + 3) / 4 * 4 && ldc >= N, "dense_tn_bf16x6_batched: bad leading dims lda=%lld ldb=%lld ldc=%lld", lda, ldb, ldc);
    PTTS_REQUIRE(strideA >= 0 && strideB >= 0 && strideC >= 0, "dense_tn_bf16x6_batched: negative stride");
    PTTS_REQUIRE(lda % 4 == 0 && ldb % 4 == 0 && ldc % 4 == 0 && strideA % 4 == 0 && strideB % 4 == 0 && strideC % 4 == 0 &&
                 (((uintptr_t)A | (uintptr_t)B | (uintptr_t)C) & 15) == 0, "dense_tn_bf16x6_batched: pointers, leading dims and strides must keep 16-byte alignment");
    TnArgs g;
    g.A = A; g.B = B; g.C = C; g.strideA = strideA; g.strideB = strideB; g.strideC = strideC;
    g.lda = lda; g.ldb = ldb; g.ldc = ldc; g.Kin = Kin; g.N = N; g.M = M;
    g.tiles_n = (N + WT - 1) / WT;
    const long long tiles = (long long)((Kin + WT - 1) / WT) * g.tiles_n;
    PTTS_REQUIRE(tiles <= 0x7fffffffLL, "dense_tn_bf16x6_batched: too many tiles");
    const dim3 grid((unsigned)tiles, 1, (unsigned)nbatch);
    constexpr size_t lds = (size_t)2 * 6 * WPL * sizeof(u16);
    static bool attr = false;
    if (!attr) { (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&dense_tn_bf16x6_kernel<3>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
                 (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&dense_tn_bf16x6_kernel<1>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds); attr = true; }
    if (planes_count == 1) hipLaunchKernelGGL((dense_tn_bf16x6_kernel<1>), grid, dim3(THREADS), lds, (hipStream_t)stream, g);
    else hipLaunchKernelGGL((dense_tn_bf16x6_kernel<3>), grid, dim3(THREADS), lds, (hipStream_t)stream, g);
    return check_launch("dense_tn_bf16x6_batched");
}

// 1 when ptts_dense_wgrad_bf16x6 takes the shape
extern "C" int ptts_dense_wgrad_bf16x6_supported(int Kin, int N, int M, long long lda, long long ldb) {
    return (Kin > 0 && N > 0 && M > 0 && Kin % 4 == 0 && N % 4 == 0 && lda % 4 == 0 && ldb % 4 == 0 &&
            (long long)wgrad_tiles_k(Kin) * ((N + WT - 1) / WT) <= 65535) ? 1 : 0;
}

namespace {
int wgrad_split(int Kin, int N, int M) {
    const int tiles = wgrad_tiles_k(Kin) * ((N + WT - 1) / WT), steps = (M + 31) / 32;
    int split = (256 + tiles - 1) / tiles;                 // about one workgroup per CU
    static int env_split = -1;                              // measurement hook (tools/dense_split_probe.py)
    if (env_split < 0) { const char* e = getenv("PTTS_DENSE_WGRAD_SPLIT"); env_split = e ? atoi(e) : 0; }
    if (env_split > 0) split = env_split;
    if (split > steps) split = steps;
    return split < 1 ? 1 : split;
}
}  // namespace

extern "C" size_t ptts_dense_wgrad_workspace_bytes(int Kin, int N, int M) {
    if (Kin <= 0 || N <= 0 || M <= 0) return 0;
    const size_t tiles = (size_t)wgrad_tiles_k(Kin) * ((N + WT - 1) / WT);
    return tiles * wgrad_split(Kin, N, M) * wgrad_part(Kin) * sizeof(float);
}

// Stage 1 of a weight-gradient product dW[Kin,N] = T(A)[M,Kin]^T . dY[M,N] (+ column sums of dY): every workgroup's partial
// tile as a row of `workspace` ([tile][split][128*128 + 128 (+ 16*128: Kin % 128 in 1..16)] floats; *split_out = workgroups per tile).  Stage 2,
// ptts_dense_wgrad_reduce_grouped, adds the rows of several products into their gradient buffers in one launch.
extern "C" int ptts_dense_wgrad_bf16x6_partials(const float* A, const float* dY, const float* mask_src, const float* in_scale,
                                                const float* in_shift, void* workspace, size_t workspace_bytes, int* split_out,
                                                int Kin, int N, int M, long long lda, long long ldb, int in_mode, float alpha,
                                                void* stream) {
    PTTS_REQUIRE(A && dY && workspace && split_out, "dense_wgrad_bf16x6: null pointer");
    PTTS_REQUIRE(ptts_dense_wgrad_bf16x6_supported(Kin, N, M, lda, ldb), "dense_wgrad_bf16x6: unsupported shape Kin=%d N=%d M=%d lda=%lld ldb=%lld", Kin, N, M, lda, ldb);
    PTTS_REQUIRE(lda >= Kin && ldb >= N, "dense_wgrad_bf16x6: bad leading dims");
    PTTS_REQUIRE(in_mode >= 0 && in_mode <= 2, "dense_wgrad_bf16x6: bad in_mode %d", in_mode);
    PTTS_REQUIRE((in_scale == nullptr) == (in_shift == nullptr), "dense_wgrad_bf16x6: scale/shift must come together");
    PTTS_REQUIRE(in_mode != PTTS_IN_MASKMUL || mask_src, "dense_wgrad_bf16x6: MASKMUL needs mask_src");
    PTTS_REQUIRE(in_mode == PTTS_IN_LRELU || !in_scale, "dense_wgrad_bf16x6: scale/shift need PTTS_IN_LRELU");
    PTTS_REQUIRE(alpha >= 0.f && alpha <= 1.f, "dense_wgrad_bf16x6: LeakyReLU slope %g outside [0, 1]", alpha);
    PTTS_REQUIRE(((uintptr_t)A & 15) == 0 && ((uintptr_t)dY & 15) == 0 && (!mask_src || ((uintptr_t)mask_src & 15) == 0) &&
                 (!in_scale || (((uintptr_t)in_scale | (uintptr_t)in_shift) & 15) == 0), "dense_wgrad_bf16x6: operands must be 16-byte aligned");
    const size_t need = ptts_dense_wgrad_workspace_bytes(Kin, N, M);
    if (workspace_bytes < need) { set_error("dense_wgrad_bf16x6: workspace %zu < %zu", workspace_bytes, need); return PTTS_EWORKSPACE; }
    WgradArgs g;
    g.A = A; g.dY = dY; g.mask_src = mask_src; g.in_scale = in_scale; g.in_shift = in_shift; g.partials = (float*)workspace;
    g.Kin = Kin; g.N = N; g.M = M; g.lda = lda; g.ldb = ldb; g.alpha = alpha;
    const int tiles_k = wgrad_tiles_k(Kin);
    const bool xr = wgrad_has_rem(Kin);
    g.tiles_k = tiles_k; g.part = wgrad_part(Kin);
    g.tiles_n = (N + WT - 1) / WT;
    g.steps_total = (M + 31) / 32;
    const int tiles = tiles_k * g.tiles_n;
    g.split = wgrad_split(Kin, N, M);
    *split_out = g.split;
    const dim3 grid((unsigned)g.split, (unsigned)tiles);
    hipStream_t st = (hipStream_t)stream;
    constexpr size_t lds = (size_t)2 * 6 * WPL * sizeof(u16);
    constexpr size_t ldsx = lds + (size_t)2 * 3 * WXPL * sizeof(u16);   // 105 KB
    const bool one = ptts::bf16_products();
#define DNS_W(MODE, AFF)                                                                                                  \
    do {                                                                                                                  \
        static bool attr = false;                                                                                         \
        if (!attr) { (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&dense_wgrad_bf16x6_kernel<MODE, AFF, 3>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds); \
                     (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&dense_wgrad_bf16x6_kernel<MODE, AFF, 1>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds); \
                     (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&dense_wgrad_bf16x6_kernel<MODE, AFF, 3, true>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)ldsx); \
                     (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&dense_wgrad_bf16x6_kernel<MODE, AFF, 1, true>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)ldsx); attr = true; } \
        if (xr) {                                                                                                         \
            if (one) hipLaunchKernelGGL((dense_wgrad_bf16x6_kernel<MODE, AFF, 1, true>), grid, dim3(THREADS), ldsx, st, g); \
            else hipLaunchKernelGGL((dense_wgrad_bf16x6_kernel<MODE, AFF, 3, true>), grid, dim3(THREADS), ldsx, st, g);   \
        } else if (one) hipLaunchKernelGGL((dense_wgrad_bf16x6_kernel<MODE, AFF, 1>), grid, dim3(THREADS), lds, st, g);   \
        else hipLaunchKernelGGL((dense_wgrad_bf16x6_kernel<MODE, AFF, 3>), grid, dim3(THREADS), lds, st, g);              \
    } while (0)
    if (in_mode == PTTS_IN_LRELU) { if (in_scale) DNS_W(PTTS_IN_LRELU, true); else DNS_W(PTTS_IN_LRELU, false); }
    else if (in_mode == PTTS_IN_MASKMUL) DNS_W(PTTS_IN_MASKMUL, false);
    else DNS_W(PTTS_IN_NONE, false);
#undef DNS_W
    return check_launch("dense_wgrad_bf16x6_partials");
}

extern "C" int ptts_dense_wgrad_reduce_grouped(const ptts_dense_wgrad_reduce_desc* descs, int n, void* stream) {
    PTTS_REQUIRE(descs && n > 0, "dense_wgrad_reduce_grouped: nothing to reduce");
    for (int base = 0; base < n; base += DR_MAX) {
        DwReduceArgs a;
        a.n = n - base < DR_MAX ? n - base : DR_MAX;
        int blocks = 0;
        for (int i = 0; i < a.n; ++i) {
            const ptts_dense_wgrad_reduce_desc& d = descs[base + i];
            PTTS_REQUIRE(d.partials && d.C && d.split > 0 && d.Kin > 0 && d.N > 0 && d.ldc >= d.N, "dense_wgrad_reduce_grouped: bad product %d", base + i);
            a.blk_begin[i] = blocks;
            a.tiles_n[i] = (d.N + WT - 1) / WT;
            blocks += wgrad_tiles_k(d.Kin) * a.tiles_n[i] * dr_bpt(d.Kin);
            a.partials[i] = d.partials; a.C[i] = d.C; a.colsum[i] = d.colsum_b; a.split[i] = d.split; a.Kin[i] = d.Kin; a.N[i] = d.N; a.ldc[i] = d.ldc;
        }
        a.blk_begin[a.n] = blocks;
        hipLaunchKernelGGL(dense_wgrad_reduce_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, a);
        int rc = check_launch("dense_wgrad_reduce_grouped");
        if (rc) return rc;
    }
    return PTTS_OK;
}

// C[Kin,N] += T(A)[M,Kin]^T . dY[M,N] and, with colsum_b, colsum_b[N] += column sums of dY -- both stages for one product.
extern "C" int ptts_dense_wgrad_bf16x6(const float* A, const float* dY, const float* mask_src, const float* in_scale,
                                       const float* in_shift, float* C, float* colsum_b, void* workspace, size_t workspace_bytes,
                                       int Kin, int N, int M, long long lda, long long ldb, long long ldc, int in_mode,
                                       float alpha, void* stream) {
    PTTS_REQUIRE(C && ldc >= N, "dense_wgrad_bf16x6: bad output");
    int split = 0;
    int rc = ptts_dense_wgrad_bf16x6_partials(A, dY, mask_src, in_scale, in_shift, workspace, workspace_bytes, &split, Kin, N, M,
                                              lda, ldb, in_mode, alpha, stream);
    if (rc) return rc;
    ptts_dense_wgrad_reduce_desc d;
    d.partials = (const float*)workspace; d.split = split; d.Kin = Kin; d.N = N; d.ldc = ldc; d.C = C; d.colsum_b = colsum_b;
    return ptts_dense_wgrad_reduce_grouped(&d, 1, stream);
}
