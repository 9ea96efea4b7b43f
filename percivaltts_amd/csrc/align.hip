// Forced alignment by Viterbi training ("Forced alignment": the build's own definition, the reference has no
// counterpart and no claim is made about HTK's numbers).  X [t_total, Dx] fp32 feature rows, the utterances packed one after the
// other by frame_off [B+1]; gauss [n_total] int32, the utterances' chains packed by state_off [B+1]: chain state n of utterance b
// uses the diagonal Gaussian gauss[state_off[b] + n] in [0, Q) -- the kernels know nothing else about phones.  All arithmetic fp64.
//
//   emission    e(t,n) = -0.5 (sum_{d} ((x_d - mu[q,d]) (x_d - mu[q,d])) w[q,d] + g[q]), x = X[t, c0:c1], q = gauss[n], the columns
//               added in index order, no contraction; w = 1 / var, g = sum_d log var (D log 2 pi is dropped)
//   alignment   V(0,0) = e(0,0), V(0,n>0) unreachable; V(t,n) = e(t,n) + max(V(t-1,n), V(t-1,n-1)), an unreachable predecessor does
//               not take part.  TIE RULE: staying wins, the advance from n-1 replaces it only if it is strictly greater.  The path is
//               followed back from (T-1, N-1): dur[n] >= 1 frames in chain state n, sum dur = T; state[t]; score = V(T-1,N-1)
//   accumulate  count[q] += frames, s1[q,d] += sum x_d, s2[q,d] += sum x_d x_d over the frames whose chain state uses q
//   update      mu = s1 / count, var = max(s2 / count - mu mu, floor[d]), w = 1 / var, g = sum_d log var in index order
//
// ptts_align_viterbi_batch is four launches on the stream, nothing between workgroups but the order of the launches:
//   layout     one workgroup: info[b] (PTTS_ALIGN_*), the exclusive scans of the utterances' cells T N and emission tiles into the
//              workspace (a flagged utterance has neither)
//   emissions  every cell of the batch in parallel, tiles of 16 frames x 64 states, a workgroup finding its utterance by bisection of
//              the tile scan; the rows of X and the chain's mu, w staged in LDS in chunks of 32 columns; e row-major fp64 in the
//              workspace, a row of align_stride(N) values.  A value that is not finite sets PTTS_ALIGN_NOT_FINITE, an index outside [0, Q) PTTS_ALIGN_BAD_GAUSS
//              (one vector atomic OR on the flag word, which is not a result)
//   time loop  ONE WAVE per utterance and no barrier: the recurrence looks at one neighbour only, so lane l keeps V of the K
//              consecutive states l K .. l K + K - 1 in registers (K = 1, 2, .., 32: the smallest power of two with 64 K >= N) and
//              fetches one value per frame, V(t-1, l K - 1), from the lane below.  The lane's K back-pointer bits are one word, a
//              frame's 64 words one coalesced row.  The emissions are read ALIGN_LOOKAHEAD / K frames ahead into registers.
//   backtrack  one wave per utterance: every lane loads its own word of sixteen rows at a time (the loads do not depend on the
//              path), the walk reads the word of the path's lane with v_readlane; dur, state (a coalesced row per 64 frames) and
//              the outputs of the flagged utterances (dur 0, state -1, score NaN) are written here.
// ptts_align_accumulate: one wave per utterance scans dur into the first row of every chain state, then one workgroup per Gaussian
// and 64 columns walks the occurrence table the host sorted by Gaussian, four frames at a time, and adds its four partial sums in
// a fixed order.  ptts_align_update: one thread per Gaussian.
// No result depends on an atomic, a reduction order that varies or another utterance: the same input gives the same bytes.
#include <climits>
#include <cmath>
#include "common.h"
#include "frame.h"

#pragma clang fp contract(off)

namespace ptts {

constexpr int ALIGN_MAX_STATES = 2048;          // 64 lanes x 32 states: a lane's back-pointer bits are one 32-bit word
constexpr int ALIGN_TILE_T = 16, ALIGN_TILE_N = 64, ALIGN_CHUNK = 32;
constexpr int ALIGN_EMIT_THREADS = 256;
constexpr int ALIGN_LAYOUT_THREADS = 256;
constexpr int ALIGN_LOOKAHEAD = 32;             // emissions a lane of the time loop holds ahead of the frame it works on, per buffer
constexpr int ALIGN_BT_ROWS = 16;               // back-pointer rows a lane of the backtrack has in flight
constexpr int ALIGN_ACC_GROUPS = 4;             // frames of a Gaussian added side by side
constexpr int ALIGN_FLAGS_LAYOUT = PTTS_ALIGN_EMPTY | PTTS_ALIGN_TOO_LONG | PTTS_ALIGN_TOO_SHORT | PTTS_ALIGN_BAD_OFFSETS;

// The workspace: cell_off [B+1] and tile_off [B+1] int64, the time loop's scores [B] fp64, the emissions fp64, the back-pointer rows [t_total][64] words.  A row of
// emissions has align_stride(N) values, N rounded up to the K states of a lane, so that a lane's K values are one aligned run;
// that is at most 31 more than N: cells + 32 t_total values hold every batch of `cells` cells.
struct AlignWorkspace {
    long long* cell_off;
    long long* tile_off;
    double* score;
    double* e;
    unsigned* bp;
};
inline size_t align_off_bytes(int B) { return align_up(((size_t)B + 1) * sizeof(long long), 256); }
inline size_t align_workspace_bytes(long long cells, int B, long long t_total) {
    return 3 * align_off_bytes(B) + align_up((size_t)(cells + 32 * t_total) * sizeof(double), 256) + (size_t)t_total * WAVE * sizeof(unsigned);
}
// States a lane of the time loop holds: the smallest power of two with 64 K >= N.
__host__ __device__ __forceinline__ int align_lane_states(int N) {
    return N <= 64 ? 1 : N <= 128 ? 2 : N <= 256 ? 4 : N <= 512 ? 8 : N <= 1024 ? 16 : 32;
}
__host__ __device__ __forceinline__ int align_stride(int N) {
    const int K = align_lane_states(N);
    return (N + K - 1) / K * K;
}
inline AlignWorkspace align_carve(void* workspace, long long cells, int B, long long t_total) {
    char* p = (char*)workspace;
    AlignWorkspace w;
    w.cell_off = (long long*)p;  p += align_off_bytes(B);
    w.tile_off = (long long*)p;  p += align_off_bytes(B);
    w.score = (double*)p;        p += align_off_bytes(B);
    w.e = (double*)p;            p += align_up((size_t)(cells + 32 * t_total) * sizeof(double), 256);
    w.bp = (unsigned*)p;
    return w;
}
// An upper bound of the batch's emission tiles from what the host knows: ceil(T/16) ceil(N/64) <= T N / 1024 + T / 16 + N / 64 + 1.
inline long long align_tile_bound(long long cells, int B, long long t_total, long long n_total) {
    return cells / (ALIGN_TILE_T * ALIGN_TILE_N) + t_total / ALIGN_TILE_T + n_total / ALIGN_TILE_N + 2LL * B + 1;
}

struct AlignUtt {
    long long f0, s0;
    int T, N;
};
// The utterance's sizes and flags from its offsets; a flagged one takes no part.
__device__ __forceinline__ int align_utt(const long long* frame_off, const long long* state_off, int b, long long t_total,
                                         long long n_total, AlignUtt& u) {
    const long long f0 = frame_off[b], f1 = frame_off[b + 1], s0 = state_off[b], s1 = state_off[b + 1];
    u.f0 = 0; u.s0 = 0; u.T = 0; u.N = 0;
    if (f0 < 0 || f1 < f0 || f1 > t_total || s0 < 0 || s1 < s0 || s1 > n_total) return PTTS_ALIGN_BAD_OFFSETS;
    u.f0 = f0; u.s0 = s0;
    u.T = (int)(f1 - f0 < INT_MAX ? f1 - f0 : INT_MAX); u.N = (int)(s1 - s0 < INT_MAX ? s1 - s0 : INT_MAX);
    if (f1 == f0 || s1 == s0) return PTTS_ALIGN_EMPTY;
    if (s1 - s0 > ALIGN_MAX_STATES) return PTTS_ALIGN_TOO_LONG;
    if (f1 - f0 < s1 - s0) return PTTS_ALIGN_TOO_SHORT;
    return 0;
}
__device__ __forceinline__ long long align_tiles(int T, int N) {
    return (long long)((T + ALIGN_TILE_T - 1) / ALIGN_TILE_T) * ((N + ALIGN_TILE_N - 1) / ALIGN_TILE_N);
}

// One workgroup: lane t owns the utterances t run .. (t + 1) run - 1.
__global__ __launch_bounds__(ALIGN_LAYOUT_THREADS) void align_layout_kernel(const long long* __restrict__ frame_off,
                                                                           const long long* __restrict__ state_off, const int B,
                                                                           const long long t_total, const long long n_total,
                                                                           const long long cells_total, const long long tiles_total,
                                                                           long long* __restrict__ cell_off, long long* __restrict__ tile_off,
                                                                           int* __restrict__ info) {
    __shared__ long long s_cells[ALIGN_LAYOUT_THREADS], s_tiles[ALIGN_LAYOUT_THREADS];
    const int tid = threadIdx.x, run = (B - 1) / ALIGN_LAYOUT_THREADS + 1;
    const int b0 = tid * run < B ? tid * run : B, b1 = b0 + run < B ? b0 + run : B;
    long long cells = 0, tiles = 0;
    for (int b = b0; b < b1; ++b) {
        AlignUtt u;
        if (!align_utt(frame_off, state_off, b, t_total, n_total, u)) {
            cells += (long long)u.T * align_stride(u.N);
            tiles += align_tiles(u.T, u.N);
        }
    }
    s_cells[tid] = cells;
    s_tiles[tid] = tiles;
    __syncthreads();
    for (int d = 1; d < ALIGN_LAYOUT_THREADS; d <<= 1) {    // inclusive scans over the lanes (Hillis-Steele)
        const long long vc = tid >= d ? s_cells[tid - d] : 0, vt = tid >= d ? s_tiles[tid - d] : 0;
        __syncthreads();
        s_cells[tid] += vc;
        s_tiles[tid] += vt;
        __syncthreads();
    }
    long long at = s_cells[tid] - cells, tat = s_tiles[tid] - tiles;
    for (int b = b0; b < b1; ++b) {
        AlignUtt u;
        int st = align_utt(frame_off, state_off, b, t_total, n_total, u);
        const long long n = st ? 0 : (long long)u.T * align_stride(u.N), nt = st ? 0 : align_tiles(u.T, u.N);
        if (at + n > cells_total || tat + nt > tiles_total) st |= PTTS_ALIGN_BAD_OFFSETS;   // more than the workspace was sized for
        cell_off[b] = at;
        tile_off[b] = tat;
        if (!st) { at += n; tat += nt; }
        info[b] = st;
    }
    if (tid == ALIGN_LAYOUT_THREADS - 1) { cell_off[B] = at; tile_off[B] = tat; }
}

// grid: the host's bound of the tiles; 256 threads: lane x = tid & 63 is the state of the tile, y = tid >> 6 owns the frames
// y, y + 4, y + 8, y + 12 of it.
__global__ __launch_bounds__(ALIGN_EMIT_THREADS) void align_emit_kernel(const float* __restrict__ X, const long long* __restrict__ frame_off,
                                                                       const int Dx, const int c0, const int c1,
                                                                       const int* __restrict__ gauss, const long long* __restrict__ state_off,
                                                                       const double* __restrict__ mu, const double* __restrict__ w,
                                                                       const double* __restrict__ g, const int Q, const int B,
                                                                       const long long* __restrict__ cell_off,
                                                                       const long long* __restrict__ tile_off, double* __restrict__ e,
                                                                       int* __restrict__ info) {
    __shared__ float s_x[ALIGN_TILE_T][ALIGN_CHUNK + 1];
    __shared__ double s_mu[ALIGN_TILE_N][ALIGN_CHUNK + 1], s_w[ALIGN_TILE_N][ALIGN_CHUNK + 1];
    const long long tile = blockIdx.x;
    if (tile >= tile_off[B]) return;
    int lo = 0, hi = B - 1;                                 // the last utterance whose first tile is <= tile (empty ones share it)
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (tile_off[mid] <= tile) lo = mid; else hi = mid - 1;
    }
    const int b = lo, tid = threadIdx.x, x = tid & 63, y = tid >> 6;
    if (info[b] & ALIGN_FLAGS_LAYOUT) return;               // (never: such an utterance has no tile)
    const long long f0 = frame_off[b], s0 = state_off[b];
    const int T = (int)(frame_off[b + 1] - f0), N = (int)(state_off[b + 1] - s0), D = c1 - c0;
    const int tiles_n = (N + ALIGN_TILE_N - 1) / ALIGN_TILE_N;
    const int local = (int)(tile - tile_off[b]);
    const int t0 = (local / tiles_n) * ALIGN_TILE_T, n0 = (local % tiles_n) * ALIGN_TILE_N;
    if (t0 >= T) return;
    int bad = 0;
    const int n = n0 + x;
    int q = n < N ? gauss[s0 + n] : 0;
    if (q < 0 || q >= Q) { bad = PTTS_ALIGN_BAD_GAUSS; q = 0; }
    double acc[4] = {0.0, 0.0, 0.0, 0.0};
    for (int c = 0; c < D; c += ALIGN_CHUNK) {
        const int dn = D - c < ALIGN_CHUNK ? D - c : ALIGN_CHUNK;
        __syncthreads();
        {                                                   // 16 rows of 32 columns of X: two values a thread
            const int col = tid & 31, row = tid >> 5;
#pragma unroll
            for (int r = 0; r < 2; ++r) {
                const int rr = row + 8 * r;
                s_x[rr][col] = (t0 + rr < T && col < dn) ? X[(f0 + t0 + rr) * Dx + c0 + c + col] : 0.f;
            }
        }
        {                                                   // the tile's 64 Gaussians, 32 columns each: a wave reads two rows at a time
            const int col = tid & 31;
            for (int row = tid >> 5; row < ALIGN_TILE_N; row += ALIGN_EMIT_THREADS / 32) {
                int qq = n0 + row < N ? gauss[s0 + n0 + row] : 0;
                if (qq < 0 || qq >= Q) qq = 0;
                s_mu[row][col] = col < dn ? mu[(long long)qq * D + c + col] : 0.0;
                s_w[row][col] = col < dn ? w[(long long)qq * D + c + col] : 0.0;
            }
        }
        __syncthreads();
        for (int d = 0; d < dn; ++d) {
            const double m = s_mu[x][d], ww = s_w[x][d];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const double t = (double)s_x[y + 4 * k][d] - m;
                acc[k] = acc[k] + (t * t) * ww;
            }
        }
    }
    const int NS = align_stride(N);
    if (n < NS) {                                           // (the padding of a row holds zeros)
        const double gq = n < N ? g[q] : 0.0;
        double* out = e + cell_off[b];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int t = t0 + y + 4 * k;
            if (t < T) {
                const double v = n < N ? -0.5 * (acc[k] + gq) : 0.0;
                if (!(v - v == 0.0)) bad |= PTTS_ALIGN_NOT_FINITE;
                out[(long long)t * NS + n] = v;
            }
        }
    }
    const int any_nf = __syncthreads_or(bad & PTTS_ALIGN_NOT_FINITE), any_bg = __syncthreads_or(bad & PTTS_ALIGN_BAD_GAUSS);
    if ((any_nf || any_bg) && tid == 0) atomicOr(info + b, (any_nf ? PTTS_ALIGN_NOT_FINITE : 0) | (any_bg ? PTTS_ALIGN_BAD_GAUSS : 0));
}

// The emissions of the lane's K states on the frames t0 .. t0 + PF - 1, one aligned run of a row of NS values: unconditional loads
// (a lane without a state, a frame past the end read the row's first K), so that nothing but the use of a value waits for it.
template <int K, int PF>
__device__ __forceinline__ void align_load_rows(const double* __restrict__ e, const int t0, const int T, const int NS, const int lane,
                                                double (&dst)[PF][K]) {
#pragma unroll
    for (int u = 0; u < PF; ++u) {
        const double* __restrict__ p = (t0 + u < T && lane * K < NS) ? e + (long long)(t0 + u) * NS + lane * K : e;
#pragma unroll
        for (int k = 0; k < K; ++k) dst[u][k] = p[k];
    }
}

// One frame of the recurrence for the lane's K states, k descending so that v[k-1] is still the last frame's; returns the lane's
// back-pointer bits (bit k: chain state lane K + k was entered from the state below).
template <int K>
__device__ __forceinline__ unsigned align_step(double (&v)[K], const double (&ee)[K], const int lane) {
    double below = __shfl_up(v[K - 1], 1, WAVE);
    if (lane == 0) below = -INFINITY;
    unsigned bits = 0;
#pragma unroll
    for (int k = K - 1; k >= 0; --k) {
        const double adv = k > 0 ? v[k - 1] : below;
        const bool take = adv > v[k];                       // staying wins a tie; -inf is "unreachable" and never greater
        v[k] = ee[k] + (take ? adv : v[k]);
        bits |= take ? 1u << k : 0u;
    }
    return bits;
}

template <int K>
__device__ __forceinline__ void align_time_loop(const double* __restrict__ e, unsigned* __restrict__ bp, const int T, const int N, const int lane,
                                double* __restrict__ score) {
    constexpr int PF = ALIGN_LOOKAHEAD / K > 8 ? 8 : ALIGN_LOOKAHEAD / K;
    const int NS = (N + K - 1) / K * K;
    double v[K], cc[PF][K], cn[PF][K];
    align_load_rows<K, PF>(e, 0, T, NS, lane, cc);
    for (int t0 = 0; t0 < T; t0 += PF) {
        align_load_rows<K, PF>(e, t0 + PF, T, NS, lane, cn);                     // in flight while this block's frames are walked
#pragma unroll
        for (int u = 0; u < PF; ++u) {
            const int t = t0 + u;
            if (t < T) {
                unsigned bits = 0;
                if (t == 0) {
#pragma unroll
                    for (int k = 0; k < K; ++k) v[k] = (lane == 0 && k == 0) ? cc[0][0] : -INFINITY;
                } else {
                    bits = align_step<K>(v, cc[u], lane);
                }
                bp[(long long)t * WAVE + lane] = bits;
            }
        }
#pragma unroll
        for (int u = 0; u < PF; ++u)
#pragma unroll
            for (int k = 0; k < K; ++k) cc[u][k] = cn[u][k];
    }
    double last = 0.0;
#pragma unroll
    for (int k = 0; k < K; ++k)
        if (k == (N - 1) % K) last = v[k];
    if (lane == (N - 1) / K) *score = last;
}

// One wave per utterance.
__global__ __launch_bounds__(WAVE) void align_time_kernel(const long long* __restrict__ frame_off, const long long* __restrict__ state_off,
                                                         const long long* __restrict__ cell_off, const double* __restrict__ e,
                                                         unsigned* __restrict__ bp, double* __restrict__ score,
                                                         const int* __restrict__ info) {
    const int b = blockIdx.x, lane = threadIdx.x;
    if (info[b]) return;
    const long long f0 = frame_off[b];
    const int T = (int)(frame_off[b + 1] - f0), N = (int)(state_off[b + 1] - state_off[b]);
    const double* eb = e + cell_off[b];
    unsigned* pb = bp + f0 * WAVE;
    double* sb = score + b;
    if (N <= 64)        align_time_loop<1>(eb, pb, T, N, lane, sb);
    else if (N <= 128)  align_time_loop<2>(eb, pb, T, N, lane, sb);
    else if (N <= 256)  align_time_loop<4>(eb, pb, T, N, lane, sb);
    else if (N <= 512)  align_time_loop<8>(eb, pb, T, N, lane, sb);
    else if (N <= 1024) align_time_loop<16>(eb, pb, T, N, lane, sb);
    else                align_time_loop<32>(eb, pb, T, N, lane, sb);
}

// One wave per utterance: the path backwards, dur and state; what a flagged utterance gets.
__global__ __launch_bounds__(WAVE) void align_backtrack_kernel(const long long* __restrict__ frame_off, const long long* __restrict__ state_off,
                                                              const long long t_total, const long long n_total,
                                                              const unsigned* __restrict__ bp, int* __restrict__ dur,
                                                              int* __restrict__ state, const double* __restrict__ loop_score,
                                                              double* __restrict__ score, int* __restrict__ info) {
    const int b = blockIdx.x, lane = threadIdx.x;
    int st = info[b];
    const double total = st ? 0.0 : loop_score[b];
    const long long f0 = frame_off[b], f1 = frame_off[b + 1], s0 = state_off[b], s1 = state_off[b + 1];
    if (!st && !(total - total == 0.0)) {             // the sum along the path left the finite numbers
        st = PTTS_ALIGN_NOT_FINITE;
        if (lane == 0) info[b] = st;
    }
    if (st) {
        if (lane == 0) score[b] = nan("");
        if (st & PTTS_ALIGN_BAD_OFFSETS) {                  // its slots are not known: nothing else is written
            if (f0 < 0 || f1 < f0 || f1 > t_total || s0 < 0 || s1 < s0 || s1 > n_total) return;
        }
        for (long long n = s0 + lane; n < s1; n += WAVE) dur[n] = 0;
        if (state)
            for (long long t = f0 + lane; t < f1; t += WAVE) state[t] = -1;
        return;
    }
    const int T = (int)(f1 - f0), N = (int)(s1 - s0);
    const int K = align_lane_states(N);
    if (lane == 0) score[b] = total;
    const int shift = K == 1 ? 0 : K == 2 ? 1 : K == 4 ? 2 : K == 8 ? 3 : K == 16 ? 4 : 5;
    const unsigned* pb = bp + f0 * WAVE;
    int n = N - 1, run = 0, held = -1;                      // run: frames seen in chain state n; held: this lane's frame of the row of 64
    unsigned r[ALIGN_BT_ROWS], rn[ALIGN_BT_ROWS];
#pragma unroll
    for (int u = 0; u < ALIGN_BT_ROWS; ++u) r[u] = pb[(long long)(T - 1 - u > 0 ? T - 1 - u : 0) * WAVE + lane];
    for (int top = T - 1; top >= 0; top -= ALIGN_BT_ROWS) {
#pragma unroll
        for (int u = 0; u < ALIGN_BT_ROWS; ++u) {           // the next sixteen rows, in flight while these are walked
            const int t = top - ALIGN_BT_ROWS - u > 0 ? top - ALIGN_BT_ROWS - u : 0;
            rn[u] = pb[(long long)t * WAVE + lane];
        }
#pragma unroll
        for (int u = 0; u < ALIGN_BT_ROWS; ++u) {
            const int t = top - u;
            if (t >= 0) {                                   // (the same for every lane)
                if (lane == (t & 63)) held = n;
                if ((t & 63) == 0 && state) {               // the frames t .. t + 63 of the utterance, a coalesced row
                    if (t + lane < T) state[f0 + t + lane] = held;
                }
                ++run;
                const unsigned word = __builtin_amdgcn_readlane(r[u], __builtin_amdgcn_readfirstlane(n >> shift));
                const int adv = t > 0 ? (int)((word >> (n & (K - 1))) & 1u) : 1;
                if (adv) {
                    if (lane == 0) dur[s0 + n] = run;
                    run = 0;
                    n = n > 0 ? n - 1 : 0;                  // (t = 0 is reached in chain state 0: the walk cannot leave the chain)
                }
            }
        }
#pragma unroll
        for (int u = 0; u < ALIGN_BT_ROWS; ++u) r[u] = rn[u];
    }
}

// ---- accumulate and update ---------------------------------------------------------------------------------------------------
// One wave per utterance: start[s0 + n] = the first row of X of chain state n, from the exclusive scan of dur; an utterance whose
// durations are negative or do not fit its frames (a flagged one has zeros) gets -1: it adds nothing.
__global__ __launch_bounds__(WAVE) void align_starts_kernel(const long long* __restrict__ frame_off, const long long* __restrict__ state_off,
                                                           const long long t_total, const long long n_total, const int* __restrict__ dur,
                                                           long long* __restrict__ start) {
    const int b = blockIdx.x, lane = threadIdx.x;
    const long long f0 = frame_off[b], f1 = frame_off[b + 1], s0 = state_off[b], s1 = state_off[b + 1];
    if (s0 < 0 || s1 < s0 || s1 > n_total) return;
    const bool frames_ok = !(f0 < 0 || f1 < f0 || f1 > t_total);
    long long carry = 0;
    int bad = !frames_ok;
    for (long long base = s0; base < s1; base += WAVE) {
        const long long n = base + lane;
        const int d = n < s1 ? dur[n] : 0;
        bad |= d < 0;
        long long incl = d < 0 ? 0 : d;
#pragma unroll
        for (int o = 1; o < WAVE; o <<= 1) {
            const long long up = __shfl_up(incl, o, WAVE);
            if (lane >= o) incl += up;
        }
        if (n < s1) start[n] = f0 + carry + incl - (d < 0 ? 0 : d);
        carry += __shfl(incl, WAVE - 1, WAVE);
    }
    bad |= carry > f1 - f0;
    if (__any(bad))
        for (long long n = s0 + lane; n < s1; n += WAVE) start[n] = -1;
}

// grid (Q, ceil(D / 64)), block (64, 4): thread (x, y) adds column x of the frames y, y + 4, .. of every occurrence of Gaussian q,
// the occurrences in the table's order; the four partial sums are added in the order of y.
__global__ __launch_bounds__(WAVE * ALIGN_ACC_GROUPS) void align_accumulate_kernel(const float* __restrict__ X, const int Dx, const int c0,
                                                                                  const int D, const int* __restrict__ gauss,
                                                                                  const long long n_total, const int* __restrict__ dur,
                                                                                  const long long* __restrict__ start,
                                                                                  const int* __restrict__ occ,
                                                                                  const long long* __restrict__ occ_off,
                                                                                  long long* __restrict__ count, double* __restrict__ s1,
                                                                                  double* __restrict__ s2) {
    __shared__ double p1[ALIGN_ACC_GROUPS][WAVE], p2[ALIGN_ACC_GROUPS][WAVE];
    const int q = blockIdx.x, x = threadIdx.x, y = threadIdx.y, d = blockIdx.y * WAVE + x;
    const long long o0 = occ_off[q], o1 = occ_off[q + 1];
    if (o0 < 0 || o1 < o0 || o1 > n_total) return;
    double a1 = 0.0, a2 = 0.0;
    long long frames = 0;
    for (long long o = o0; o < o1; ++o) {
        const long long n = occ[o];
        if (n < 0 || n >= n_total || gauss[n] != q) continue;                   // (a table that is not of this chain adds nothing)
        const long long s = start[n];
        const int len = s < 0 ? 0 : dur[n];
        frames += len;
        if (d < D)
            for (int j = y; j < len; j += ALIGN_ACC_GROUPS) {
                const double v = (double)X[(s + j) * Dx + c0 + d];
                a1 = a1 + v;
                a2 = a2 + v * v;
            }
    }
    p1[y][x] = a1;
    p2[y][x] = a2;
    __syncthreads();
    if (frames == 0 || y != 0) return;                      // a Gaussian without frames is left untouched
    if (d < D) {
        double t1 = p1[0][x], t2 = p2[0][x];
#pragma unroll
        for (int k = 1; k < ALIGN_ACC_GROUPS; ++k) { t1 = t1 + p1[k][x]; t2 = t2 + p2[k][x]; }
        s1[(long long)q * D + d] = s1[(long long)q * D + d] + t1;
        s2[(long long)q * D + d] = s2[(long long)q * D + d] + t2;
    }
    if (x == 0 && blockIdx.y == 0) count[q] += frames;
}

// One thread per Gaussian.
__global__ __launch_bounds__(256) void align_update_kernel(const long long* __restrict__ count, const double* __restrict__ s1,
                                                          const double* __restrict__ s2, const double* __restrict__ floor_, const int Q,
                                                          const int D, const long long min_count, double* __restrict__ mu,
                                                          double* __restrict__ w, double* __restrict__ g, int* __restrict__ kept,
                                                          int* __restrict__ floored) {
    const int q = blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= Q) return;
    const long long c = count[q];
    if (c < min_count || c < 1) {
        kept[q] = 1;
        floored[q] = 0;
        return;
    }
    const double cnt = (double)c;
    double sum = 0.0;
    int nf = 0;
    for (int d = 0; d < D; ++d) {
        const long long i = (long long)q * D + d;
        const double m = s1[i] / cnt;
        double var = s2[i] / cnt - m * m;
        if (!(var >= floor_[d])) { var = floor_[d]; ++nf; }
        mu[i] = m;
        w[i] = 1.0 / var;
        sum = sum + log(var);
    }
    g[q] = sum;
    kept[q] = 0;
    floored[q] = nf;
}

}  // namespace ptts

using namespace ptts;

extern "C" int ptts_align_max_states(void) { return ALIGN_MAX_STATES; }

extern "C" size_t ptts_align_workspace_bytes(long long cells, int B, long long t_total) {
    if (cells < 0 || B < 0 || B > PACKED_MAX_UTTS || t_total < 0 || cells >= (1LL << 40) || t_total >= (1LL << 31)) return 0;
    return align_workspace_bytes(cells, B, t_total);
}

extern "C" int ptts_align_viterbi_batch(const float* X, const long long* frame_off, long long t_total, int Dx, int c0, int c1,
                                        const int* gauss, const long long* state_off, long long n_total, const double* mu,
                                        const double* w, const double* g, int Q, int B, long long cells, int* dur, int* state,
                                        double* score, int* info, int phases, void* workspace, size_t workspace_bytes, void* stream) {
    PTTS_REQUIRE(B >= 0 && B <= PACKED_MAX_UTTS && t_total >= 0 && n_total >= 0 && cells >= 0 && cells < (1LL << 40) &&
                     t_total < (1LL << 31) && n_total < (1LL << 31),
                 "align_viterbi_batch: B=%d t_total=%lld n_total=%lld cells=%lld", B, t_total, n_total, cells);
    PTTS_REQUIRE(Dx >= 1 && c0 >= 0 && c0 < c1 && c1 <= Dx, "align_viterbi_batch: Dx=%d columns [%d, %d)", Dx, c0, c1);
    PTTS_REQUIRE(Q >= 1, "align_viterbi_batch: Q=%d", Q);
    PTTS_REQUIRE(phases >= 1 && phases <= PTTS_ALIGN_PHASE_ALL, "align_viterbi_batch: phases=%d", phases);
    if (B == 0) return PTTS_OK;
    PTTS_REQUIRE(frame_off && state_off && mu && w && g && score && info && (X || t_total == 0) && ((gauss && dur) || n_total == 0),
                 "align_viterbi_batch: null tensor");
    const long long tiles = align_tile_bound(cells + 32 * t_total, B, t_total, n_total);
    PTTS_REQUIRE(tiles < INT_MAX, "align_viterbi_batch: %lld emission tiles in one call", tiles);
    const size_t need = align_workspace_bytes(cells, B, t_total);
    if (!workspace || workspace_bytes < need) {
        set_error("align_viterbi_batch: workspace of %zu bytes, %zu needed", workspace_bytes, need);
        return PTTS_EWORKSPACE;
    }
    const AlignWorkspace ws = align_carve(workspace, cells, B, t_total);
    hipStream_t st = (hipStream_t)stream;
    if (phases & PTTS_ALIGN_PHASE_EMISSIONS) {
        hipLaunchKernelGGL(align_layout_kernel, dim3(1), dim3(ALIGN_LAYOUT_THREADS), 0, st, frame_off, state_off, B, t_total, n_total,
                           cells + 32 * t_total, tiles, ws.cell_off, ws.tile_off, info);
        if (cells > 0)
            hipLaunchKernelGGL(align_emit_kernel, dim3((unsigned)tiles), dim3(ALIGN_EMIT_THREADS), 0, st, X, frame_off, Dx, c0, c1, gauss,
                               state_off, mu, w, g, Q, B, ws.cell_off, ws.tile_off, ws.e, info);
    }
    if (phases & PTTS_ALIGN_PHASE_TIME_LOOP)
        hipLaunchKernelGGL(align_time_kernel, dim3(B), dim3(WAVE), 0, st, frame_off, state_off, ws.cell_off, ws.e, ws.bp, ws.score, info);
    if (phases & PTTS_ALIGN_PHASE_BACKTRACK)
        hipLaunchKernelGGL(align_backtrack_kernel, dim3(B), dim3(WAVE), 0, st, frame_off, state_off, t_total, n_total, ws.bp, dur, state,
                           ws.score, score, info);
    return check_launch("align_viterbi_batch");
}

extern "C" size_t ptts_align_accumulate_workspace_bytes(long long n_total) {
    if (n_total < 0 || n_total >= (1LL << 40)) return 0;
    return align_up((size_t)n_total * sizeof(long long), 256) + 256;
}

extern "C" int ptts_align_accumulate(const float* X, const long long* frame_off, long long t_total, int Dx, int c0, int c1,
                                     const int* gauss, const long long* state_off, long long n_total, const int* dur, const int* occ,
                                     const long long* occ_off, int Q, int B, long long* count, double* s1, double* s2,
                                     void* workspace, size_t workspace_bytes, void* stream) {
    PTTS_REQUIRE(B >= 0 && B <= PACKED_MAX_UTTS && t_total >= 0 && n_total >= 0 && t_total < (1LL << 40) && n_total < (1LL << 31),
                 "align_accumulate: B=%d t_total=%lld n_total=%lld", B, t_total, n_total);
    PTTS_REQUIRE(Dx >= 1 && c0 >= 0 && c0 < c1 && c1 <= Dx, "align_accumulate: Dx=%d columns [%d, %d)", Dx, c0, c1);
    PTTS_REQUIRE(Q >= 1, "align_accumulate: Q=%d", Q);
    if (B == 0 || n_total == 0 || t_total == 0) return PTTS_OK;
    PTTS_REQUIRE(X && frame_off && state_off && gauss && dur && occ && occ_off && count && s1 && s2, "align_accumulate: null tensor");
    const size_t need = ptts_align_accumulate_workspace_bytes(n_total);
    if (!workspace || workspace_bytes < need) {
        set_error("align_accumulate: workspace of %zu bytes, %zu needed", workspace_bytes, need);
        return PTTS_EWORKSPACE;
    }
    hipStream_t st = (hipStream_t)stream;
    long long* start = (long long*)workspace;
    const int D = c1 - c0;
    hipLaunchKernelGGL(align_starts_kernel, dim3(B), dim3(WAVE), 0, st, frame_off, state_off, t_total, n_total, dur, start);
    hipLaunchKernelGGL(align_accumulate_kernel, dim3(Q, (D + WAVE - 1) / WAVE), dim3(WAVE, ALIGN_ACC_GROUPS), 0, st, X, Dx, c0, D, gauss,
                       n_total, dur, start, occ, occ_off, count, s1, s2);
    return check_launch("align_accumulate");
}

extern "C" int ptts_align_update(const long long* count, const double* s1, const double* s2, const double* floor, int Q, int D,
                                 long long min_count, double* mu, double* w, double* g, int* kept, int* floored, void* stream) {
    PTTS_REQUIRE(Q >= 0 && D >= 1 && min_count >= 1, "align_update: Q=%d D=%d min_count=%lld", Q, D, min_count);
    if (Q == 0) return PTTS_OK;
    PTTS_REQUIRE(count && s1 && s2 && floor && mu && w && g && kept && floored, "align_update: null tensor");
    hipLaunchKernelGGL(align_update_kernel, dim3((Q + 255) / 256), dim3(256), 0, (hipStream_t)stream, count, s1, s2, floor, Q, D, min_count,
                       mu, w, g, kept, floored);
    return check_launch("align_update");
}
