// One training batch cut out of a corpus that lives on the device (data.DeviceCorpus): the cropped utterances of up to three
// streams (inputs, outputs, time weights) are packed row-wise, src_k [N_total][D_k], behind one table of utterance starts, and
// row b of the batch is the window of n[b] frames at shift[b] of utterance utt[b], zero-padded to T frames.  For one batch row
// the real part is ONE contiguous run of n*D floats in source and destination alike and the padding is one contiguous run of
// zeros behind it, so the kernel is a copy of runs: every element of the destination is written exactly once (no memset in
// front), and one launch serves all streams (blockIdx.z).
//
// Access width.  D = 601 is odd, so the two runs start at any multiple of 4 bytes relative to each other and neither start is
// 16-byte aligned in general.  The destination is walked in groups of four floats that ARE 16-byte aligned (a scalar head of
// up to three elements in front, a scalar tail behind): each lane stores one aligned float4.  Its four source floats are
// contiguous but only 4-byte aligned; global memory takes a 16-byte load at any 4-byte boundary (the loads below are declared
// with that alignment, one global_load_dwordx4 each), and consecutive lanes still read consecutive 16 bytes.
#include "common.h"
#include <cstdint>

namespace ptts {

constexpr int BG_THREADS = 256;
constexpr int BG_GROUPS_PER_THREAD = 4;      // float4 groups per lane: four independent loads in flight
constexpr int BG_MAX_STREAMS = 3;

struct bg_streams {                           // by value in the kernel arguments
    const float* src0; const float* src1; const float* src2;
    float* dst0; float* dst1; float* dst2;
    int D0, D1, D2;
};

typedef float bg_f4 __attribute__((ext_vector_type(4)));
struct __attribute__((packed, aligned(4))) bg_f4_a4 { bg_f4 v; };      // four floats at a 4-byte boundary

// grid (chunks of the row, B, streams).  All source indices in 64 bits; an index inside one destination row fits an int
// (the entry point checks T * D).  A row whose table entries do not lie inside its utterance copies nothing (all zeros): the
// caller validates the tables on the host, the kernel only makes sure that nothing it is given can make it read out of bounds.
__global__ __launch_bounds__(BG_THREADS) void batch_windows_kernel(bg_streams s, const long long* __restrict__ row_off, int U,
                                                                  const int* __restrict__ utt, const int* __restrict__ shift,
                                                                  const int* __restrict__ nreal, int T) {
    const int k = blockIdx.z, b = blockIdx.y;
    const float* __restrict__ src = k == 0 ? s.src0 : (k == 1 ? s.src1 : s.src2);
    float* __restrict__ dst = k == 0 ? s.dst0 : (k == 1 ? s.dst1 : s.dst2);
    const int D = k == 0 ? s.D0 : (k == 1 ? s.D1 : s.D2);
    const int total = T * D;
    const int u = utt[b], sh = shift[b];
    int n = nreal[b];
    long long first = 0;
    if (u < 0 || u >= U || sh < 0 || n < 0 || n > T) {
        n = 0;
    } else {
        first = row_off[u] + sh;
        if (first + n > row_off[u + 1]) n = 0;
    }
    const int real = n * D;                                  // elements copied; [real, total) are zeros
    src += first * (long long)D;
    dst += (long long)b * total;

    int head = (int)((4 - (((uintptr_t)dst >> 2) & 3)) & 3);     // elements in front of the first 16-byte boundary
    if (head > total) head = total;
    const int ngroups = (total - head) >> 2;
    const int tail0 = head + (ngroups << 2);
    if (blockIdx.x == 0) {
        const int t = threadIdx.x;
        if (t < head) dst[t] = t < real ? src[t] : 0.f;
        else if (t >= 4 && t - 4 + tail0 < total) {
            const int i = t - 4 + tail0;
            dst[i] = i < real ? src[i] : 0.f;
        }
    }
    for (int g = blockIdx.x * BG_THREADS + threadIdx.x; g < ngroups; g += gridDim.x * BG_THREADS) {
        const int i = head + (g << 2);
        bg_f4 v;
        if (i + 4 <= real) {
            v = reinterpret_cast<const bg_f4_a4*>(src + i)->v;
        } else {
            v.x = i < real ? src[i] : 0.f;
            v.y = i + 1 < real ? src[i + 1] : 0.f;
            v.z = i + 2 < real ? src[i + 2] : 0.f;
            v.w = 0.f;
        }
        *reinterpret_cast<bg_f4*>(dst + i) = v;
    }
}

}  // namespace ptts

using namespace ptts;

extern "C" int ptts_batch_windows(const float* src0, const float* src1, const float* src2, float* dst0, float* dst1, float* dst2,
                                  int D0, int D1, int D2, int nstreams, const long long* row_off, int U, const int* utt,
                                  const int* shift, const int* n, int B, int T, void* stream) {
    PTTS_REQUIRE(nstreams >= 1 && nstreams <= BG_MAX_STREAMS, "batch_windows: %d streams (1..%d)", nstreams, BG_MAX_STREAMS);
    PTTS_REQUIRE(row_off && utt && shift && n && U > 0 && B > 0 && T > 0, "batch_windows: bad args");
    PTTS_REQUIRE(B <= 65535, "batch_windows: B=%d rows (at most 65535)", B);
    const float* srcs[BG_MAX_STREAMS] = {src0, src1, src2};
    float* dsts[BG_MAX_STREAMS] = {dst0, dst1, dst2};
    const int Ds[BG_MAX_STREAMS] = {D0, D1, D2};
    long long widest = 0;
    for (int k = 0; k < nstreams; ++k) {
        PTTS_REQUIRE(srcs[k] && dsts[k] && Ds[k] > 0, "batch_windows: stream %d: bad args", k);
        PTTS_REQUIRE((long long)T * Ds[k] < (1LL << 31) - 8, "batch_windows: stream %d: T*D = %lld does not fit an int", k,
                     (long long)T * Ds[k]);
        PTTS_REQUIRE((uintptr_t)srcs[k] % 4 == 0 && (uintptr_t)dsts[k] % 4 == 0, "batch_windows: stream %d: misaligned", k);
        if ((long long)T * Ds[k] > widest) widest = (long long)T * Ds[k];
    }
    const long long per_block = (long long)BG_THREADS * BG_GROUPS_PER_THREAD * 4;
    long long chunks = (widest + per_block - 1) / per_block;
    if (chunks < 1) chunks = 1;
    if (chunks > 4096) chunks = 4096;      // the kernel strides over the rest
    bg_streams s = {src0, src1, src2, dst0, dst1, dst2, D0, D1, D2};
    hipLaunchKernelGGL(batch_windows_kernel, dim3((unsigned)chunks, (unsigned)B, (unsigned)nstreams), dim3(BG_THREADS), 0,
                       (hipStream_t)stream, s, row_off, U, utt, shift, n, T);
    return check_launch("batch_windows");
}
