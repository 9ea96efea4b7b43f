// Label front end: HTS full-context labels -> the frame-level context matrix the networks read.  It restates, without regular
// expressions, what the reference's external/merlin/label_normalisation.py computes with `re` (load_question_set_continous,
// wildcards2regex, pattern_matching_binary, pattern_matching_continous_position) and with nested Python loops
// (load_labels_with_state_alignment :661-710, load_labels_with_phone_alignment :546-568).  Two launches per chunk of utterances:
//
// labels_match: one full-context label per PHONE (not per state) and a question table compiled on the host -> V [P, Q] fp32,
//   Q = nQS + nCQS, the QS columns first, both in file order.
//   * the labels are packed bytes with an int32 offsets array [P+1]; a workgroup walks labels p = blockIdx.x, + gridDim.x, ...,
//     stages the label in the LDS, and its 256 threads own whole questions q = tid, tid + 256, ...
//   * the pattern table (bytes, per pattern an offset and a word `length | anchor flags`) is staged once per workgroup in the LDS
//     when it fits (LAB_LDS_BYTES; the shipped 416-question set is 7 KB) and read from global memory otherwise.
//   * a QS pattern is what is left of the HTK question after its outer '*' are stripped: anchored at the start (end) when the
//     question held a '*' but did not begin (end) with one, a plain substring search otherwise; an inner '*' is any run of
//     characters, '?' exactly one.  The column is 1 as soon as one pattern of the question matches.  Patterns without wildcards
//     (all 916 of the shipped set) take a direct comparison loop; the others the classic greedy wildcard walk that restarts
//     behind the last '*' -- at most (L+1)(M+1) steps for a label of L and a pattern of M bytes.
//   * a CQS is prefix (capture) suffix, the capture a run of digits ((\d+)) or of digits and '.' (([\d\.]+)): the leftmost
//     start at which the prefix matches, the longest run after it, shortened while the suffix does not follow -- the order in
//     which `re` backtracks.  The value is an integer mantissa divided by a power of ten in fp64 (both exact up to 15 digits,
//     the IEEE division correctly rounded: Python's float() of the capture), then rounded to fp32; -1 without a match.
//     More than 15 digits, more than one '.', or no digit at all is an error: the label's word of `status` says which question.
//   * no atomics: every V element and every status word has one writer, the same input gives the same bytes.
//
// labels_expand: V [P, Q] and a segment table -> X [T, Q + F] fp32 for a chunk of utterances packed row-wise (as compose.hip packs
//   them).  A segment is one HMM state (state alignment) or one phone (phone alignment): 8 int32
//   {phone row, first output row, frame_number, state_index, state_index_backward, phone_duration, state_duration_base, 0}.
//   A workgroup takes LAB_ROWS output rows: its first LAB_ROWS threads find each row's segment by binary search over the first rows
//   (zero-frame segments own no row) and compute the F frame features -- ratios of small integers, divided in fp64 and rounded
//   once to fp32, which is the reference's "fp64 matrix, then numpy.array(data, 'float32')" bit for bit -- into the LDS; then
//   all threads write the block as one flat, 16-byte aligned span of float4 stores (LAB_ROWS rows of any width are a whole number
//   of float4), reading the phone rows of V with coalesced loads (a phone row is re-read for each of its frames: L2 hits).
//
// labels_segments: durations dur [P, D] fp32 (D = 5 states or 1 phone, in frames) of U utterances (unit_off [U+1] over the phones)
//   -> the segment table labels_expand reads, what parse_label_file builds on the host from a label file's times.  Three small
//   launches, no atomics, every word with one writer and no dependence on the launch geometry:
//   * totals: one workgroup per utterance rounds its durations (seg_frames: rint, ties to even; NaN and anything below min_frames
//     become min_frames, anything above max_frames becomes max_frames and sets PTTS_LABELS_SEG_CLAMPED in status[u]) and sums them
//     into rows[u];
//   * offsets: one workgroup scans rows [U] in place in tiles of SEG_TILE -> each utterance's first row, rows[U] = T;
//   * table: one workgroup per utterance scans its P_u * D frame counts in tiles of SEG_TILE (SEG_ITEMS consecutive elements a
//     thread, the wave's inclusive scan by wave shuffles, the four wave totals through the LDS, a carry from tile to tile) and writes
//     the eight words of every segment; a phone's duration and a state's base are re-summed from the phone's own D values.
//   The host bounds P * D * max_frames below 2^31, so no sum can leave int.
#include "common.h"

namespace ptts {

constexpr int LAB_THREADS = 256;
constexpr int LAB_MAX_LABEL = PTTS_LABELS_MAX_LABEL;
constexpr int LAB_LDS_BYTES = 48 << 10;         // pattern table (bytes + 8 per pattern) staged in the LDS up to this size
constexpr int LAB_META_LEN = 0xffff;            // pat_meta: length | flags
constexpr int LAB_ROWS = 16;                    // output rows per workgroup of labels_expand
constexpr int LAB_MAX_F = 9;
constexpr int LAB_CC_POINTS = PTTS_LABELS_CC_POINTS;
constexpr int SEG_ITEMS = 4;                    // consecutive elements per thread of a scan tile
constexpr int SEG_TILE = LAB_THREADS * SEG_ITEMS;
constexpr int SEG_MAX_D = PTTS_LABELS_SEG_STATES;

__host__ __device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// pattern p [M] without wildcards against the label s [L]
template <typename SP, typename PP>
__host__ __device__ bool match_plain(SP s, int L, PP p, int M, bool astart, bool aend) {
    if (M > L) return false;
    int lo = aend ? L - M : 0, hi = astart ? 0 : L - M;
    for (int i = lo; i <= hi; ++i) {
        int j = 0;
        while (j < M && s[i + j] == p[j]) ++j;
        if (j == M) return true;
    }
    return false;
}

// pattern with '*' (any run) and '?' (one character); without an anchor the pattern behaves as if it began (ended) with '*'
template <typename SP, typename PP>
__host__ __device__ bool match_wild(SP s, int L, PP p, int M, bool astart, bool aend) {
    int i = 0, j = 0, star = astart ? -1 : 0, mark = 0;
    int budget = 2 * (L + 1) * (M + 1);         // the walk needs at most (L+1)(M+1) steps; the guard only makes the bound explicit
    while (budget-- > 0) {
        if (!aend && j == M) return true;
        if (i >= L) break;
        const int c = j < M ? (int)p[j] : -1;
        if (c == '*') { star = j + 1; mark = i; ++j; }
        else if (c == '?' || c == (int)s[i]) { ++i; ++j; }
        else if (star >= 0) { j = star; ++mark; i = mark; }
        else return false;
    }
    while (j < M && p[j] == '*') ++j;
    return j == M && i >= L;
}

// fixed-length piece of a CQS ('?' is one character) at s
template <typename SP, typename PP>
__host__ __device__ __forceinline__ bool match_fixed(SP s, PP p, int M) {
    for (int j = 0; j < M; ++j) {
        const int c = p[j];
        if (c != '?' && c != (int)s[j]) return false;
    }
    return true;
}

__host__ __device__ __forceinline__ double pow10_exact(int k) {
    const double t[16] = {1e0, 1e1, 1e2, 1e3, 1e4, 1e5, 1e6, 1e7, 1e8, 1e9, 1e10, 1e11, 1e12, 1e13, 1e14, 1e15};
    return t[k & 15];
}

// A CQS on the label s [L]: prefix pre [MP] and suffix suf [MS] ('?' = one character) around a run of digits (and '.' with
// `dots`).  Leftmost prefix, longest run, shortened while the suffix does not follow.  Returns the captured decimal or -1;
// err = PTTS_LABELS_ERR_* when the capture is no number of at most 15 digits.
template <typename SP, typename PP>
__host__ __device__ float capture_value(SP s, int L, PP pre, int MP, PP suf, int MS, bool astart, bool aend, bool dots, int& err) {
    int cap = -1, capn = 0;
    const int last = astart ? 0 : L - MP - 1 - MS;              // prefix, one captured character at least, suffix
    for (int s0 = 0; s0 <= last && cap < 0; ++s0) {
        if (s0 + MP + 1 + MS > L) break;
        if (!match_fixed(s + s0, pre, MP)) continue;
        const int b = s0 + MP;
        int n = 0;
        while (b + n < L && ((s[b + n] >= '0' && s[b + n] <= '9') || (dots && s[b + n] == '.'))) ++n;
        n = n > L - MS - b ? L - MS - b : n;                    // the suffix has to fit behind the run
        for (; n >= 1; --n) {
            if (aend && b + n + MS != L) break;                 // a shorter run ends further from the label's end
            if (match_fixed(s + b + n, suf, MS)) { cap = b; capn = n; break; }
        }
    }
    if (cap < 0) return -1.0f;
    long long mant = 0;
    int nd = 0, ndot = 0, frac = 0;
    for (int i = 0; i < capn; ++i) {
        const int ch = s[cap + i];
        if (ch == '.') { ++ndot; continue; }
        ++nd;
        if (ndot) ++frac;
        if (nd <= 15) mant = mant * 10 + (ch - '0');
    }
    if (nd > 15 || ndot > 1 || nd == 0) {
        err = nd > 15 ? PTTS_LABELS_ERR_DIGITS : PTTS_LABELS_ERR_FORMAT;
        return -1.0f;
    }
    return (float)((double)mant / pow10_exact(frac));
}

struct LabelsTable {
    const unsigned char* pat_bytes;     // [n_pat_bytes]
    const int* pat_off;                 // [NP]
    const int* pat_meta;                // [NP] length | PTTS_LABELS_ANCHOR_START | _ANCHOR_END | _WILD
    const int* qs_first;                // [nQS + 1] first pattern of every QS question
    const int* cqs;                     // [nCQS][3] prefix pattern, suffix pattern, capture kind
    int n_pat_bytes, NP, nQS, nCQS;
};

// dynamic LDS: [label LAB_MAX_LABEL][error words LAB_THREADS * 4] and, with TABLE_IN_LDS, [pat_off NP*4][pat_meta NP*4][bytes]
template <bool TABLE_IN_LDS>
__global__ __launch_bounds__(LAB_THREADS) void labels_match_kernel(const unsigned char* __restrict__ labels,
                                                                   const int* __restrict__ label_off, const LabelsTable tb,
                                                                   float* __restrict__ V, int* __restrict__ status,
                                                                   const int P, const int label_bytes) {
    extern __shared__ __align__(16) unsigned char smem[];
    unsigned char* s_lab = smem;
    int* s_err = (int*)(smem + LAB_MAX_LABEL);
    int* s_off = s_err + LAB_THREADS;
    int* s_meta = s_off + tb.NP;
    unsigned char* s_pat = (unsigned char*)(s_meta + tb.NP);
    const int tid = threadIdx.x;
    const int NP = tb.NP, nQS = tb.nQS, Q = tb.nQS + tb.nCQS;
    if (TABLE_IN_LDS) {
        for (int i = tid; i < NP; i += LAB_THREADS) { s_off[i] = tb.pat_off[i]; s_meta[i] = tb.pat_meta[i]; }
        for (int i = tid; i < tb.n_pat_bytes; i += LAB_THREADS) s_pat[i] = tb.pat_bytes[i];
    }
    // pattern k -> its bytes (clamped into the table), length and flags
    auto pattern = [&](int k, int& M, int& flags) {
        k = clampi(k, 0, NP - 1);
        const int off = clampi(TABLE_IN_LDS ? s_off[k] : tb.pat_off[k], 0, tb.n_pat_bytes);
        const int meta = TABLE_IN_LDS ? s_meta[k] : tb.pat_meta[k];
        M = meta & LAB_META_LEN;
        M = M > tb.n_pat_bytes - off ? tb.n_pat_bytes - off : M;
        flags = meta;
        return off;
    };
    for (int p = blockIdx.x; p < P; p += gridDim.x) {
        __syncthreads();                // the previous label is done with; the table is staged
        const int b0 = clampi(label_off[p], 0, label_bytes);
        int L = clampi(label_off[p + 1], b0, label_bytes) - b0;
        L = L > LAB_MAX_LABEL ? LAB_MAX_LABEL : L;
        for (int i = tid; i < L; i += LAB_THREADS) s_lab[i] = labels[b0 + i];
        __syncthreads();
        int err = 0;
        for (int q = tid; q < Q; q += LAB_THREADS) {
            float v;
            if (q < nQS) {
                const int k0 = clampi(tb.qs_first[q], 0, NP), k1 = clampi(tb.qs_first[q + 1], k0, NP);
                bool hit = false;
                for (int k = k0; k < k1 && !hit; ++k) {
                    int M, fl;
                    const int off = pattern(k, M, fl);
                    const bool as = fl & PTTS_LABELS_ANCHOR_START, ae = fl & PTTS_LABELS_ANCHOR_END;
                    if (TABLE_IN_LDS)
                        hit = (fl & PTTS_LABELS_WILD) ? match_wild(s_lab, L, s_pat + off, M, as, ae) : match_plain(s_lab, L, s_pat + off, M, as, ae);
                    else
                        hit = (fl & PTTS_LABELS_WILD) ? match_wild(s_lab, L, tb.pat_bytes + off, M, as, ae)
                                                      : match_plain(s_lab, L, tb.pat_bytes + off, M, as, ae);
                }
                v = hit ? 1.0f : 0.0f;
            } else {
                const int c = q - nQS;
                int MP, fp, MS, fs;
                const int offp = pattern(tb.cqs[c * 3 + 0], MP, fp), offs = pattern(tb.cqs[c * 3 + 1], MS, fs);
                const bool dots = tb.cqs[c * 3 + 2] == PTTS_LABELS_CAPTURE_DECIMAL;
                const bool as = fp & PTTS_LABELS_ANCHOR_START, ae = fs & PTTS_LABELS_ANCHOR_END;
                int e = 0;
                v = TABLE_IN_LDS ? capture_value(s_lab, L, s_pat + offp, MP, s_pat + offs, MS, as, ae, dots, e)
                                 : capture_value(s_lab, L, tb.pat_bytes + offp, MP, tb.pat_bytes + offs, MS, as, ae, dots, e);
                if (e && !err) err = ((c + 1) << 2) | e;
            }
            V[(size_t)p * Q + q] = v;
        }
        // the label's status word: the error of the lowest thread that has one (threads own questions in ascending order)
        s_err[tid] = err;
        __syncthreads();
        if (tid == 0) {
            int e = 0;
            for (int t = 0; t < LAB_THREADS && !e; ++t) e = s_err[t];
            status[p] = e;
        }
    }
}

__device__ __forceinline__ int labels_feature_count(int mode) {
    return mode == PTTS_LABELS_FULL ? 9 : mode == PTTS_LABELS_MINIMAL_FRAME ? 2 : mode == PTTS_LABELS_STATE_ONLY ? 1
         : mode == PTTS_LABELS_MINIMAL_PHONEME ? 3 : mode == PTTS_LABELS_COARSE_CODING ? 4 : 0;
}

// The F frame features of output row i of a segment {phone, first row, fn, state, state backwards | pd, base, 0, 0}: ratios in
// fp64, rounded once.  cc [3][LAB_CC_POINTS] is read for coarse coding only.
__host__ __device__ inline void frame_features(int mode, int4 a, int4 b, int i, const float* cc, float* f) {
    const double fn = (double)a.z, pd = (double)b.y, base = (double)b.z, di = (double)i;
    if (mode == PTTS_LABELS_FULL) {
        f[0] = (float)((di + 1.0) / fn);                    // fraction through the state, forwards
        f[1] = (float)((fn - di) / fn);                     // ... backwards
        f[2] = (float)a.z;                                  // frames of the state
        f[3] = (float)a.w;                                  // state index, forwards
        f[4] = (float)b.x;                                  // ... backwards
        f[5] = (float)b.y;                                  // frames of the phone
        f[6] = (float)(fn / pd);                            // share of the phone this state takes
        f[7] = (float)((pd - di - base) / pd);              // fraction through the phone, backwards
        f[8] = (float)((base + di + 1.0) / pd);             // ... forwards
    } else if (mode == PTTS_LABELS_MINIMAL_FRAME) {
        f[0] = (float)((di + 1.0) / fn);
        f[1] = (float)a.w;
    } else if (mode == PTTS_LABELS_STATE_ONLY) {
        f[0] = (float)a.w;
    } else if (mode == PTTS_LABELS_MINIMAL_PHONEME) {
        f[0] = (float)((di + 1.0) / fn);
        f[1] = (float)((fn - di) / fn);
        f[2] = (float)a.z;
    } else if (mode == PTTS_LABELS_COARSE_CODING) {
        // frames counted from the phone's start; the clamp keeps a bad table inside cc, a consistent one never reaches it
        const int rel = clampi((int)((200.0 / pd) * (base + di)), 0, LAB_CC_POINTS - 301);
        f[0] = cc[0 * LAB_CC_POINTS + 300 + rel];
        f[1] = cc[1 * LAB_CC_POINTS + 200 + rel];
        f[2] = cc[2 * LAB_CC_POINTS + 100 + rel];
        f[3] = (float)b.y;
    }
}

// grid ceil(T / LAB_ROWS), block LAB_THREADS.  seg [S][8], cc [3][LAB_CC_POINTS] (coarse coding only)
__global__ __launch_bounds__(LAB_THREADS) void labels_expand_kernel(const float* __restrict__ V, const int* __restrict__ seg,
                                                                    const float* __restrict__ cc, float* __restrict__ X, const int P,
                                                                    const int Q, const int S, const int T, const int mode) {
    __shared__ int s_phone[LAB_ROWS];
    __shared__ float s_feat[LAB_ROWS][LAB_MAX_F + 1];
    const int tid = threadIdx.x;
    const int F = labels_feature_count(mode), W = Q + F;
    const int row0 = blockIdx.x * LAB_ROWS;
    const int rows = T - row0 < LAB_ROWS ? T - row0 : LAB_ROWS;
    if (tid < rows) {
        const int row = row0 + tid;
        int lo = 0, hi = S;             // first segment that starts behind `row`; the one before it owns the row
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (seg[(size_t)mid * 8 + 1] <= row) lo = mid + 1; else hi = mid;
        }
        const int4* sp = (const int4*)(seg + (size_t)(lo > 0 ? lo - 1 : 0) * 8);
        const int4 a = sp[0], b = sp[1];
        s_phone[tid] = clampi(a.x, 0, P - 1);
        frame_features(mode, a, b, row - a.y, cc, s_feat[tid]);
    }
    __syncthreads();
    const int n = rows * W;                                     // LAB_ROWS * W floats at the most: far inside int
    float* xb = X + (size_t)row0 * W;                           // 16-byte aligned: row0 * W is a multiple of LAB_ROWS
    for (int g = tid * 4; g < n; g += LAB_THREADS * 4) {
        int r = g / W, c = g - r * W;
        float v[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            v[k] = 0.f;
            if (g + k < n) v[k] = c < Q ? V[(size_t)s_phone[r] * Q + c] : s_feat[r][c - Q];
            if (++c == W) { c = 0; ++r; }
        }
        if (g + 4 <= n) {
            *(float4*)(xb + g) = make_float4(v[0], v[1], v[2], v[3]);
        } else {
            for (int k = 0; g + k < n; ++k) xb[g + k] = v[k];
        }
    }
}

// frames of one duration: rint (ties to even), NaN and n < lo -> lo, n > hi -> hi with `clamped` set.  lo <= hi <= 2^24 are exact
// in fp32, so the comparisons decide before the conversion to int and no value outside int is ever converted.
__host__ __device__ __forceinline__ int seg_frames(float d, int lo, int hi, int& clamped) {
    const float r = rintf(d);
    if (!(r >= (float)lo)) return lo;
    if (r > (float)hi) { clamped = 1; return hi; }
    return (int)r;
}

// exclusive scan of one value per thread over the workgroup: returns the sum of the threads before this one, `total` the sum of
// all.  s_w [LAB_THREADS / 64]; two barriers, so s_w is free again on return.
__device__ __forceinline__ int block_exclusive_scan(int v, int* s_w, int& total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int incl = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int up = __shfl_up(incl, o, 64);
        if (lane >= o) incl += up;
    }
    __syncthreads();
    if (lane == 63) s_w[wave] = incl;
    __syncthreads();
    int before = 0, all = 0;
#pragma unroll
    for (int w = 0; w < LAB_THREADS / 64; ++w) {
        before += w < wave ? s_w[w] : 0;
        all += s_w[w];
    }
    total = all;
    return before + incl - v;
}

// the phones [p0, p1) of utterance u, clamped into [0, P] and made monotone
__device__ __forceinline__ void seg_unit(const int* __restrict__ unit_off, int u, int P, int& p0, int& p1) {
    p0 = clampi(unit_off[u], 0, P);
    p1 = clampi(unit_off[u + 1], p0, P);
}

// grid U: rows[u] = frames of utterance u, status[u] = PTTS_LABELS_SEG_CLAMPED when a duration was above max_frames
__global__ __launch_bounds__(LAB_THREADS) void labels_segments_totals_kernel(const float* __restrict__ dur, const int* __restrict__ unit_off,
                                                                             int* __restrict__ rows, int* __restrict__ status, const int P,
                                                                             const int D, const int lo, const int hi) {
    __shared__ int s_w[LAB_THREADS / 64];
    const int u = blockIdx.x;
    int p0, p1;
    seg_unit(unit_off, u, P, p0, p1);
    const int e0 = p0 * D, n = (p1 - p0) * D;
    int sum = 0, clamped = 0;
    for (int e = threadIdx.x; e < n; e += LAB_THREADS) sum += seg_frames(dur[e0 + e], lo, hi, clamped);
    int total, any;
    block_exclusive_scan(sum, s_w, total);
    block_exclusive_scan(clamped, s_w, any);
    if (threadIdx.x == 0) {
        rows[u] = total;
        status[u] = any ? PTTS_LABELS_SEG_CLAMPED : 0;
    }
}

// grid 1: rows [U] totals -> rows [U+1] first rows, in place
__global__ __launch_bounds__(LAB_THREADS) void labels_segments_offsets_kernel(int* __restrict__ rows, const int U) {
    __shared__ int s_w[LAB_THREADS / 64];
    int carry = 0;
    for (int t0 = 0; t0 < U; t0 += SEG_TILE) {
        const int i0 = t0 + threadIdx.x * SEG_ITEMS;
        int v[SEG_ITEMS], sum = 0;
#pragma unroll
        for (int k = 0; k < SEG_ITEMS; ++k) { v[k] = i0 + k < U ? rows[i0 + k] : 0; sum += v[k]; }
        int total;
        int at = carry + block_exclusive_scan(sum, s_w, total);
#pragma unroll
        for (int k = 0; k < SEG_ITEMS; ++k) {
            if (i0 + k < U) rows[i0 + k] = at;
            at += v[k];
        }
        carry += total;
    }
    if (threadIdx.x == 0) rows[U] = carry;
}

// grid U: seg [P*D][8] of utterance u's phones; rows[u] is its first output row
__global__ __launch_bounds__(LAB_THREADS) void labels_segments_table_kernel(const float* __restrict__ dur, const int* __restrict__ unit_off,
                                                                            const int* __restrict__ rows, int* __restrict__ seg, const int P,
                                                                            const int D, const int lo, const int hi) {
    __shared__ int s_w[LAB_THREADS / 64];
    const int u = blockIdx.x;
    int p0, p1;
    seg_unit(unit_off, u, P, p0, p1);
    const int e0 = p0 * D, n = (p1 - p0) * D;
    int carry = rows[u], unused = 0;
    for (int t0 = 0; t0 < n; t0 += SEG_TILE) {
        const int i0 = t0 + threadIdx.x * SEG_ITEMS;
        int v[SEG_ITEMS], sum = 0;
#pragma unroll
        for (int k = 0; k < SEG_ITEMS; ++k) { v[k] = i0 + k < n ? seg_frames(dur[e0 + i0 + k], lo, hi, unused) : 0; sum += v[k]; }
        int total;
        int at = carry + block_exclusive_scan(sum, s_w, total);
#pragma unroll
        for (int k = 0; k < SEG_ITEMS; ++k) {
            const int e = e0 + i0 + k;                          // < P * D inside the bound below
            if (i0 + k < n) {
                const int p = e / D, st = e - p * D;
                int pd = 0, base = 0;
                for (int j = 0; j < D; ++j) {
                    const int f = seg_frames(dur[p * D + j], lo, hi, unused);
                    pd += f;
                    base += j < st ? f : 0;
                }
                int4* sp = (int4*)(seg + (size_t)e * 8);
                sp[0] = make_int4(p, at, v[k], D > 1 ? st + 1 : 0);
                sp[1] = make_int4(D > 1 ? D - st : 0, pd, base, 0);
            }
            at += v[k];
        }
        carry += total;
    }
}

static int labels_cus() {
    static int cus = 0;
    if (cus == 0) {
        int dev = 0, n = 0;
        if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n < 1)
            n = 256;
        cus = n;
    }
    return cus;
}

}  // namespace ptts

using namespace ptts;

extern "C" int ptts_labels_feature_count(int mode) {
    switch (mode) {
        case PTTS_LABELS_FULL: return 9;
        case PTTS_LABELS_MINIMAL_FRAME: return 2;
        case PTTS_LABELS_STATE_ONLY: return 1;
        case PTTS_LABELS_NONE: return 0;
        case PTTS_LABELS_MINIMAL_PHONEME: return 3;
        case PTTS_LABELS_COARSE_CODING: return 4;
    }
    return -1;
}

extern "C" int ptts_labels_match(const unsigned char* labels, const int* label_off, int P, int label_bytes, int max_label_len,
                                 const unsigned char* pat_bytes, int n_pat_bytes, const int* pat_off, const int* pat_meta, int NP,
                                 const int* qs_first, int nQS, const int* cqs, int nCQS, float* V, int* status, void* stream) {
    PTTS_REQUIRE(labels && label_off && V && status, "labels_match: null tensor");
    PTTS_REQUIRE(P > 0 && label_bytes >= 0, "labels_match: bad dims P=%d label_bytes=%d", P, label_bytes);
    PTTS_REQUIRE(max_label_len >= 0 && max_label_len <= LAB_MAX_LABEL, "labels_match: a label of %d bytes exceeds the %d the kernel stages",
                 max_label_len, LAB_MAX_LABEL);
    PTTS_REQUIRE(nQS >= 0 && nCQS >= 0 && nQS + nCQS > 0, "labels_match: bad question counts nQS=%d nCQS=%d", nQS, nCQS);
    PTTS_REQUIRE(NP > 0 && n_pat_bytes >= 0 && pat_off && pat_meta && (pat_bytes || n_pat_bytes == 0),
                 "labels_match: bad pattern table NP=%d bytes=%d", NP, n_pat_bytes);
    PTTS_REQUIRE((nQS == 0 || qs_first) && (nCQS == 0 || cqs), "labels_match: null question table");
    PTTS_REQUIRE((long long)P * (nQS + nCQS) < (1ll << 40), "labels_match: P=%d questions=%d too large", P, nQS + nCQS);
    LabelsTable tb{pat_bytes, pat_off, pat_meta, qs_first, cqs, n_pat_bytes, NP, nQS, nCQS};
    hipStream_t st = (hipStream_t)stream;
    const size_t base = LAB_MAX_LABEL + LAB_THREADS * sizeof(int);
    const size_t table = (size_t)NP * 8 + (size_t)n_pat_bytes;
    const int grid = P < labels_cus() * 8 ? P : labels_cus() * 8;
    if (table <= (size_t)LAB_LDS_BYTES)
        hipLaunchKernelGGL(labels_match_kernel<true>, dim3(grid), dim3(LAB_THREADS), base + table, st, labels, label_off, tb, V, status, P, label_bytes);
    else
        hipLaunchKernelGGL(labels_match_kernel<false>, dim3(grid), dim3(LAB_THREADS), base, st, labels, label_off, tb, V, status, P, label_bytes);
    return check_launch("labels_match");
}

extern "C" int ptts_labels_expand(const float* V, const int* seg, const float* cc_table, float* X, int P, int Q, int S, int T,
                                  int mode, void* stream) {
    PTTS_REQUIRE(V && seg && X, "labels_expand: null tensor");
    PTTS_REQUIRE(P > 0 && Q > 0 && S > 0 && T > 0, "labels_expand: bad dims P=%d Q=%d S=%d T=%d", P, Q, S, T);
    const int F = ptts_labels_feature_count(mode);
    PTTS_REQUIRE(F >= 0, "labels_expand: unknown mode %d", mode);
    PTTS_REQUIRE(mode != PTTS_LABELS_COARSE_CODING || cc_table, "labels_expand: coarse coding needs its table");
    PTTS_REQUIRE(((size_t)X & 15) == 0 && ((size_t)seg & 15) == 0, "labels_expand: X and seg have to be 16-byte aligned");
    PTTS_REQUIRE((long long)LAB_ROWS * (Q + F) < (1ll << 30), "labels_expand: Q=%d too wide", Q);
    hipLaunchKernelGGL(labels_expand_kernel, dim3((T + LAB_ROWS - 1) / LAB_ROWS), dim3(LAB_THREADS), 0, (hipStream_t)stream, V, seg,
                       cc_table, X, P, Q, S, T, mode);
    return check_launch("labels_expand");
}

extern "C" int ptts_labels_segments(const float* dur, const int* unit_off, int P, int D, int U, int min_frames, int max_frames, int* seg,
                                    int* rows, int* status, void* stream) {
    PTTS_REQUIRE(unit_off && rows && status, "labels_segments: null tensor");
    PTTS_REQUIRE(P >= 0 && U > 0 && (D == SEG_MAX_D || D == 1), "labels_segments: bad dims P=%d D=%d U=%d (D is %d or 1)", P, D, U, SEG_MAX_D);
    PTTS_REQUIRE(P == 0 || (dur && seg), "labels_segments: null tensor");
    PTTS_REQUIRE(((size_t)seg & 15) == 0, "labels_segments: seg has to be 16-byte aligned");
    PTTS_REQUIRE(min_frames >= 0 && min_frames <= max_frames && max_frames <= PTTS_LABELS_SEG_MAX_FRAMES,
                 "labels_segments: bad bounds min_frames=%d max_frames=%d (0 <= min <= max <= %d)", min_frames, max_frames,
                 PTTS_LABELS_SEG_MAX_FRAMES);
    PTTS_REQUIRE((long long)P * D * max_frames < (1ll << 31), "labels_segments: P=%d D=%d max_frames=%d allow 2^31 rows or more", P, D,
                 max_frames);
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(labels_segments_totals_kernel, dim3(U), dim3(LAB_THREADS), 0, st, dur, unit_off, rows, status, P, D, min_frames,
                       max_frames);
    hipLaunchKernelGGL(labels_segments_offsets_kernel, dim3(1), dim3(LAB_THREADS), 0, st, rows, U);
    hipLaunchKernelGGL(labels_segments_table_kernel, dim3(U), dim3(LAB_THREADS), 0, st, dur, unit_off, rows, seg, P, D, min_frames,
                       max_frames);
    return check_launch("labels_segments");
}
