// Dynamic time warping of a batch of utterance pairs ("DTW alignment": the build's own definition, the
// reference has no counterpart).  G [sum Tg, D] generated and R [sum Tr, D] reference rows, fp32, packed one utterance after the
// other by g_off / r_off [B+1] int64; the distance is taken over the columns [c0, c1).
//
//   local cost    c(i,j) = sqrt( sum_{d=c0}^{c1-1} (scale (G[i,d] - R[j,d]))^2 ), fp64 from the fp32 rows, the columns added in index
//                 order, one IEEE square root (contraction is off: t * t and the sum round separately, as the restatement does)
//   accumulated   A(0,0) = c(0,0); A(i,j) = c(i,j) + min(A(i-1,j-1), A(i-1,j), A(i,j-1)), a predecessor outside the matrix does not
//                 take part; the diagonal one wins a tie, then (i-1,j), then (i,j-1): a candidate replaces the best only if it is
//                 strictly smaller, tried in that order
//   path          the back-pointers from (Tg-1, Tr-1) to (0,0), reported forwards: gi[k], ri[k], k = 0 .. L-1,
//                 max(Tg,Tr) <= L <= Tg+Tr-1; cost = A(Tg-1,Tr-1)
//
// Four launches on the stream, nothing between workgroups but the order of the launches:
//   layout     one workgroup: info[b] (PTTS_DTW_*), L[b] = 0, cost[b], and the exclusive scan of the pairs' cell counts Tg Tr into
//              the workspace (a flagged pair has no cells)
//   costs      every cell of the batch in parallel, tiles of 32 x 32 cells, the rows staged in LDS in chunks of 32 columns.  The
//              matrix is stored SKEWED, diagonal-major: the cells of diagonal k = i + j lie one after the other in ascending i,
//              the diagonals one after the other with no padding (diag_start below), so the wavefront reads and writes a diagonal
//              coalesced -- in row-major a diagonal has the stride Tr - 1.  A thread of the tile owns the cells (x, (c - x) mod 32),
//              c = y, y + 8, ..: the 32 lanes of one c write two runs of consecutive cells of two diagonals, and both LDS reads are
//              free of bank conflicts (row stride 33).  A cost that is not finite sets PTTS_DTW_NOT_FINITE (one atomic OR per tile
//              on the status word, which is not a result).
//   wavefront  one workgroup per pair walks the diagonals in order, lane t owning the cells ilo + t and ilo + t + NT of a diagonal
//              (NT = 256, 512 or 1024 by the batch's longest short side: no per-lane loop, a diagonal has at most min(Tg,Tr)
//              <= 2 NT cells).  A of the last two diagonals and the one being written lie in LDS indexed by i (three buffers in
//              rotation), so ONE barrier separates two diagonals.  The local costs are read eight diagonals ahead, into registers:
//              a diagonal's step is then LDS latency and the barrier, not a round trip to memory (0.87 us a
//              diagonal with the loads waited for where they were issued, which is what the compiler made of a one-diagonal
//              look-ahead).  One back-pointer byte per cell, skewed like the costs.
//   backtrack  one wave per pair: lane 0 follows the back-pointers (L dependent byte loads) and writes the path backwards into
//              the workspace, then the wave copies it forwards into the pair's slots gi / ri [path_off[b] ..]: exactly L values
//              are written, the slots behind them are left as they were.
// No result depends on an atomic, a reduction order or another pair: the same input gives the same bytes, in any batch.
#include <climits>
#include <cmath>
#include "common.h"
#include "frame.h"

#pragma clang fp contract(off)

namespace ptts {

constexpr int DTW_MAX_FRAMES = 2048;            // the longest side of a pair: three diagonals of A in fp64 are 48 KiB of LDS
constexpr int DTW_TILE = 32;                    // the cost pass: cells per tile side, columns per chunk
constexpr int DTW_COST_THREADS = 256;
constexpr int DTW_LAYOUT_THREADS = 256;
constexpr int DTW_PREFETCH = 8;                 // diagonals whose costs a lane of the wavefront has in flight
constexpr int DTW_BP_DIAG = 0, DTW_BP_UP = 1, DTW_BP_LEFT = 2, DTW_BP_NONE = 3;

// The workspace: cell_off [B+1] int64, costs [cells] fp64, back-pointers [cells] bytes, the backward paths [2][path_total] int32.
struct DtwWorkspace {
    long long* cell_off;
    double* cost;
    unsigned char* bp;
    int* back;
};
inline size_t dtw_cell_off_bytes(int B) { return align_up(((size_t)B + 1) * sizeof(long long), 256); }
inline size_t dtw_workspace_bytes(long long cells, int B, long long path_total) {
    return dtw_cell_off_bytes(B) + align_up((size_t)cells * sizeof(double), 256) + align_up((size_t)cells, 256) +
           2 * (size_t)path_total * sizeof(int);
}
inline DtwWorkspace dtw_carve(void* workspace, long long cells, int B) {
    char* p = (char*)workspace;
    DtwWorkspace w;
    w.cell_off = (long long*)p;  p += dtw_cell_off_bytes(B);
    w.cost = (double*)p;         p += align_up((size_t)cells * sizeof(double), 256);
    w.bp = (unsigned char*)p;    p += align_up((size_t)cells, 256);
    w.back = (int*)p;
    return w;
}

// The first cell of diagonal k of a Tg x Tr matrix in the skewed order: the number of cells on the diagonals before it.
__host__ __device__ __forceinline__ long long diag_start(int k, int Tg, int Tr) {
    const long long m = Tg < Tr ? Tg : Tr, M = Tg < Tr ? Tr : Tg;
    if (k <= m) return (long long)k * (k + 1) / 2;
    if (k <= M) return m * (m + 1) / 2 + (k - m) * m;
    const long long n = (long long)Tg + Tr - 1 - k;         // the diagonals from k on hold n, n - 1, .., 1 cells
    return (long long)Tg * Tr - n * (n + 1) / 2;
}
__host__ __device__ __forceinline__ int diag_ilo(int k, int Tr) { return k > Tr - 1 ? k - (Tr - 1) : 0; }

// The pair's sizes and status from its offsets; false: the pair takes no part (its status bits say why).
struct DtwPair {
    long long g0, r0, p0;
    int Tg, Tr;
};
__device__ __forceinline__ int dtw_pair(const long long* g_off, const long long* r_off, const long long* path_off, int b,
                                        long long g_total, long long r_total, long long path_total, int max_gen, int max_ref,
                                        DtwPair& p) {
    const long long g0 = g_off[b], g1 = g_off[b + 1], r0 = r_off[b], r1 = r_off[b + 1], p0 = path_off[b];
    if (g0 < 0 || g1 < g0 || g1 > g_total || r0 < 0 || r1 < r0 || r1 > r_total) return PTTS_DTW_BAD_OFFSETS;
    if (g1 == g0 || r1 == r0) return PTTS_DTW_EMPTY;
    if (g1 - g0 > max_gen || r1 - r0 > max_ref) return PTTS_DTW_TOO_LONG;
    if (p0 < 0 || p0 > path_total || (g1 - g0) + (r1 - r0) - 1 > path_total - p0) return PTTS_DTW_BAD_OFFSETS;
    p.g0 = g0; p.r0 = r0; p.p0 = p0;
    p.Tg = (int)(g1 - g0); p.Tr = (int)(r1 - r0);
    return 0;
}

// One workgroup: lane t owns the pairs t run .. (t + 1) run - 1.
__global__ __launch_bounds__(DTW_LAYOUT_THREADS) void dtw_layout_kernel(const long long* __restrict__ g_off, const long long* __restrict__ r_off,
                                                                       const long long* __restrict__ path_off, const int B,
                                                                       const long long g_total, const long long r_total,
                                                                       const long long path_total, const int max_gen, const int max_ref,
                                                                       const long long cells_total, long long* __restrict__ cell_off,
                                                                       int* __restrict__ L, double* __restrict__ cost, int* __restrict__ info) {
    __shared__ long long s_sum[DTW_LAYOUT_THREADS];
    const int tid = threadIdx.x, run = (B - 1) / DTW_LAYOUT_THREADS + 1;
    const int b0 = tid * run < B ? tid * run : B, b1 = b0 + run < B ? b0 + run : B;
    long long sum = 0;
    for (int b = b0; b < b1; ++b) {
        DtwPair p;
        const int st = dtw_pair(g_off, r_off, path_off, b, g_total, r_total, path_total, max_gen, max_ref, p);
        if (!st) sum += (long long)p.Tg * p.Tr;
    }
    s_sum[tid] = sum;
    __syncthreads();
    for (int d = 1; d < DTW_LAYOUT_THREADS; d <<= 1) {      // inclusive scan over the lanes (Hillis-Steele)
        const long long v = tid >= d ? s_sum[tid - d] : 0;
        __syncthreads();
        s_sum[tid] += v;
        __syncthreads();
    }
    long long at = s_sum[tid] - sum;
    for (int b = b0; b < b1; ++b) {
        DtwPair p;
        int st = dtw_pair(g_off, r_off, path_off, b, g_total, r_total, path_total, max_gen, max_ref, p);
        const long long n = st ? 0 : (long long)p.Tg * p.Tr;
        if (at + n > cells_total) { st = st | PTTS_DTW_BAD_OFFSETS; }      // more cells than the workspace was sized for
        cell_off[b] = at;
        at += st ? 0 : n;
        info[b] = st;
        L[b] = 0;
        cost[b] = st ? nan("") : 0.0;
    }
    if (tid == DTW_LAYOUT_THREADS - 1) cell_off[B] = at;
}

// grid (tiles along j, tiles along i, B), 256 threads: lane x = tid & 31 is the row of the tile, y = tid >> 5.
__global__ __launch_bounds__(DTW_COST_THREADS) void dtw_cost_kernel(const float* __restrict__ G, const float* __restrict__ R,
                                                                   const long long* __restrict__ g_off, const long long* __restrict__ r_off,
                                                                   const long long* __restrict__ cell_off, const int D, const int c0,
                                                                   const int c1, const double scale, double* __restrict__ cost,
                                                                   int* __restrict__ info) {
    __shared__ float s_g[DTW_TILE][DTW_TILE + 1], s_r[DTW_TILE][DTW_TILE + 1];
    const int b = blockIdx.z, tid = threadIdx.x, x = tid & 31, y = tid >> 5;
    if (info[b] & (PTTS_DTW_EMPTY | PTTS_DTW_TOO_LONG | PTTS_DTW_BAD_OFFSETS)) return;
    const long long g0 = g_off[b], r0 = r_off[b];
    const int Tg = (int)(g_off[b + 1] - g0), Tr = (int)(r_off[b + 1] - r0);
    const int i0 = blockIdx.y * DTW_TILE, j0 = blockIdx.x * DTW_TILE;
    if (i0 >= Tg || j0 >= Tr) return;
    double acc[4] = {0.0, 0.0, 0.0, 0.0};
    for (int c = c0; c < c1; c += DTW_TILE) {
        const int dn = c1 - c < DTW_TILE ? c1 - c : DTW_TILE;
        __syncthreads();
#pragma unroll
        for (int q = 0; q < 4; ++q) {                       // row y + 8 q of both tiles, column x: 32 consecutive floats per row
            const int row = y + 8 * q;
            s_g[row][x] = (i0 + row < Tg && x < dn) ? G[(g0 + i0 + row) * D + c + x] : 0.f;
            s_r[row][x] = (j0 + row < Tr && x < dn) ? R[(r0 + j0 + row) * D + c + x] : 0.f;
        }
        __syncthreads();
        for (int d = 0; d < dn; ++d) {
            const double g = (double)s_g[x][d];
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const double t = scale * (g - (double)s_r[(y + 8 * q - x) & 31][d]);
                acc[q] = acc[q] + t * t;
            }
        }
    }
    const int i = i0 + x;
    double* out = cost + cell_off[b];
    int bad = 0;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int j = j0 + ((y + 8 * q - x) & 31);
        if (i < Tg && j < Tr) {
            const double v = sqrt(acc[q]);
            bad |= !(v - v == 0.0);
            const int k = i + j;
            out[diag_start(k, Tg, Tr) + (i - diag_ilo(k, Tr))] = v;
        }
    }
    if (__syncthreads_or(bad) && tid == 0) atomicOr(info + b, PTTS_DTW_NOT_FINITE);
}

// The costs of the lane's two cells on each of the diagonals k0 .. k0 + DTW_PREFETCH - 1: unconditional loads (a lane without a
// cell reads c[0]), so that nothing but the use of a value waits for it.
template <int NT>
__device__ __forceinline__ void dtw_load_costs(const double* __restrict__ c, const int k0, const int ndiag, const int Tg, const int Tr,
                                               const int tid, double (&dst)[DTW_PREFETCH][2]) {
#pragma unroll
    for (int u = 0; u < DTW_PREFETCH; ++u) {
        const int k = k0 + u < ndiag ? k0 + u : ndiag - 1;
        const int ilo = diag_ilo(k, Tr), ihi = k < Tg - 1 ? k : Tg - 1, len = k0 + u < ndiag ? ihi - ilo + 1 : 0;
        const long long start = diag_start(k, Tg, Tr);
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            const int t = tid + q * NT;
            dst[u][q] = c[t < len ? start + t : 0];
        }
    }
}

// One workgroup of NT lanes per pair, min(Tg, Tr) <= 2 NT.
template <int NT>
__global__ __launch_bounds__(NT) void dtw_wavefront_kernel(const long long* __restrict__ g_off, const long long* __restrict__ r_off,
                                                          const long long* __restrict__ cell_off, const double* __restrict__ cost,
                                                          unsigned char* __restrict__ bp, double* __restrict__ total,
                                                          const int* __restrict__ info) {
    __shared__ double s_a[3][DTW_MAX_FRAMES];               // A of three diagonals in rotation, indexed by i
    const int b = blockIdx.x, tid = threadIdx.x;
    if (info[b]) return;
    const int Tg = (int)(g_off[b + 1] - g_off[b]), Tr = (int)(r_off[b + 1] - r_off[b]);
    if ((Tg < Tr ? Tg : Tr) > 2 * NT) return;               // (the launcher picks NT from the caps; never taken)
    const double* c = cost + cell_off[b];
    unsigned char* p = bp + cell_off[b];
    const int ndiag = Tg + Tr - 1;
    double* cur = s_a[0];
    double* p1 = s_a[1];                                    // diagonal k - 1
    double* p2 = s_a[2];                                    // diagonal k - 2
    double cc[DTW_PREFETCH][2], cn[DTW_PREFETCH][2];
    dtw_load_costs<NT>(c, 0, ndiag, Tg, Tr, tid, cc);
    long long start = 0;
    for (int k0 = 0; k0 < ndiag; k0 += DTW_PREFETCH) {
        dtw_load_costs<NT>(c, k0 + DTW_PREFETCH, ndiag, Tg, Tr, tid, cn);      // in flight while this block's diagonals are walked
#pragma unroll
        for (int u = 0; u < DTW_PREFETCH; ++u) {
            const int k = k0 + u;
            if (k < ndiag) {                                // (the same for every lane: the barrier below is reached by all or none)
                const int ilo = diag_ilo(k, Tr), ihi = k < Tg - 1 ? k : Tg - 1, len = ihi - ilo + 1;
#pragma unroll
                for (int q = 0; q < 2; ++q) {
                    const int t = tid + q * NT;
                    if (t < len) {
                        const int i = ilo + t, j = k - i, im = i > 0 ? i - 1 : 0;
                        const double d = p2[im], up = p1[im], left = p1[i];     // what lies outside the matrix is read and not used
                        double best = d;
                        int from = i > 0 && j > 0 ? DTW_BP_DIAG : DTW_BP_NONE;
                        if (i > 0 && (from == DTW_BP_NONE || up < best)) { best = up; from = DTW_BP_UP; }
                        if (j > 0 && (from == DTW_BP_NONE || left < best)) { best = left; from = DTW_BP_LEFT; }
                        const double a = from == DTW_BP_NONE ? cc[u][q] : cc[u][q] + best;
                        cur[i] = a;
                        p[start + t] = (unsigned char)from;
                        if (k == ndiag - 1) total[b] = a;
                    }
                }
                start += len;
                double* const o = p2;
                p2 = p1; p1 = cur; cur = o;
                __syncthreads();
            }
        }
#pragma unroll
        for (int u = 0; u < DTW_PREFETCH; ++u) { cc[u][0] = cn[u][0]; cc[u][1] = cn[u][1]; }
    }
}

// One wave per pair.
__global__ __launch_bounds__(WAVE) void dtw_backtrack_kernel(const long long* __restrict__ g_off, const long long* __restrict__ r_off,
                                                            const long long* __restrict__ path_off, const long long* __restrict__ cell_off,
                                                            const unsigned char* __restrict__ bp, int* __restrict__ back,
                                                            const long long path_total, int* __restrict__ gi, int* __restrict__ ri,
                                                            int* __restrict__ L, const int* __restrict__ info) {
    __shared__ int s_len;
    const int b = blockIdx.x, tid = threadIdx.x;
    if (info[b]) return;
    const int Tg = (int)(g_off[b + 1] - g_off[b]), Tr = (int)(r_off[b + 1] - r_off[b]);
    const long long p0 = path_off[b];
    const unsigned char* p = bp + cell_off[b];
    int* bg = back + p0;
    int* br = back + path_total + p0;
    if (tid == 0) {
        int i = Tg - 1, j = Tr - 1, n = 0;
        const int cap = Tg + Tr - 1;
        while (n < cap) {
            bg[n] = i;
            br[n] = j;
            ++n;
            if (i == 0 && j == 0) break;
            const int k = i + j;
            int from = p[diag_start(k, Tg, Tr) + (i - diag_ilo(k, Tr))];
            if (i == 0) from = DTW_BP_LEFT;                 // (what the wavefront wrote there anyway: the walk cannot leave the matrix)
            else if (j == 0) from = DTW_BP_UP;
            if (from != DTW_BP_LEFT) --i;
            if (from != DTW_BP_UP) --j;
        }
        s_len = n;
        L[b] = n;
    }
    __syncthreads();                                        // lane 0's stores to `back` are the wave's own: visible after the barrier
    const int n = s_len;
    for (int k = tid; k < n; k += WAVE) {
        gi[p0 + k] = bg[n - 1 - k];
        ri[p0 + k] = br[n - 1 - k];
    }
}

}  // namespace ptts

using namespace ptts;

extern "C" int ptts_dtw_max_frames(void) { return DTW_MAX_FRAMES; }

extern "C" size_t ptts_dtw_workspace_bytes(long long cells, int B, long long path_total) {
    if (cells < 0 || B < 0 || B > PACKED_MAX_UTTS || path_total < 0 || cells >= (1LL << 40) || path_total >= (1LL << 40)) return 0;
    return dtw_workspace_bytes(cells, B, path_total);
}

extern "C" int ptts_dtw_align_batch(const float* G, const long long* g_off, long long g_total, const float* R, const long long* r_off,
                                    long long r_total, int B, int D, int c0, int c1, double scale, int max_gen, int max_ref,
                                    long long cells, const long long* path_off, long long path_total, int* gi, int* ri, int* L,
                                    double* cost, int* info, int phases, void* workspace, size_t workspace_bytes, void* stream) {
    PTTS_REQUIRE(B >= 0 && B <= PACKED_MAX_UTTS && g_total >= 0 && r_total >= 0 && path_total >= 0 && cells >= 0 &&
                     cells < (1LL << 40) && path_total < (1LL << 40),
                 "dtw_align_batch: B=%d g_total=%lld r_total=%lld path_total=%lld cells=%lld", B, g_total, r_total, path_total, cells);
    PTTS_REQUIRE(D >= 1 && c0 >= 0 && c0 < c1 && c1 <= D, "dtw_align_batch: D=%d columns [%d, %d)", D, c0, c1);
    PTTS_REQUIRE(scale - scale == 0.0, "dtw_align_batch: scale is not finite");
    PTTS_REQUIRE(max_gen >= 0 && max_gen <= DTW_MAX_FRAMES && max_ref >= 0 && max_ref <= DTW_MAX_FRAMES,
                 "dtw_align_batch: max_gen=%d max_ref=%d (at most %d frames a side)", max_gen, max_ref, DTW_MAX_FRAMES);
    PTTS_REQUIRE(phases >= 1 && phases <= PTTS_DTW_PHASE_ALL, "dtw_align_batch: phases=%d", phases);
    PTTS_REQUIRE(g_total < (1LL << 40) && r_total < (1LL << 40), "dtw_align_batch: g_total=%lld r_total=%lld", g_total, r_total);
    if (B == 0) return PTTS_OK;
    PTTS_REQUIRE(g_off && r_off && path_off && L && cost && info && (G || g_total == 0) && (R || r_total == 0) &&
                     ((gi && ri) || path_total == 0),
                 "dtw_align_batch: null tensor");
    const size_t need = dtw_workspace_bytes(cells, B, path_total);
    if (!workspace || workspace_bytes < need) {
        set_error("dtw_align_batch: workspace of %zu bytes, %zu needed", workspace_bytes, need);
        return PTTS_EWORKSPACE;
    }
    const DtwWorkspace w = dtw_carve(workspace, cells, B);
    hipStream_t st = (hipStream_t)stream;
    if (phases & PTTS_DTW_PHASE_COSTS) {
        hipLaunchKernelGGL(dtw_layout_kernel, dim3(1), dim3(DTW_LAYOUT_THREADS), 0, st, g_off, r_off, path_off, B, g_total, r_total,
                           path_total, max_gen, max_ref, cells, w.cell_off, L, cost, info);
        if (max_gen > 0 && max_ref > 0)
            hipLaunchKernelGGL(dtw_cost_kernel, dim3((max_ref + DTW_TILE - 1) / DTW_TILE, (max_gen + DTW_TILE - 1) / DTW_TILE, B),
                               dim3(DTW_COST_THREADS), 0, st, G, R, g_off, r_off, w.cell_off, D, c0, c1, scale, w.cost, info);
    }
    if ((phases & PTTS_DTW_PHASE_WAVEFRONT) && max_gen > 0 && max_ref > 0) {
        const int side = max_gen < max_ref ? max_gen : max_ref;
        if (side <= 512)
            hipLaunchKernelGGL(dtw_wavefront_kernel<256>, dim3(B), dim3(256), 0, st, g_off, r_off, w.cell_off, w.cost, w.bp, cost, info);
        else if (side <= 1024)
            hipLaunchKernelGGL(dtw_wavefront_kernel<512>, dim3(B), dim3(512), 0, st, g_off, r_off, w.cell_off, w.cost, w.bp, cost, info);
        else
            hipLaunchKernelGGL(dtw_wavefront_kernel<1024>, dim3(B), dim3(1024), 0, st, g_off, r_off, w.cell_off, w.cost, w.bp, cost, info);
    }
    if ((phases & PTTS_DTW_PHASE_BACKTRACK) && max_gen > 0 && max_ref > 0)
        hipLaunchKernelGGL(dtw_backtrack_kernel, dim3(B), dim3(WAVE), 0, st, g_off, r_off, path_off, w.cell_off, w.bp, w.back, path_total,
                           gi, ri, L, info);
    return check_launch("dtw_align_batch");
}
