// Conv2D layers outside the 4 -> 4 5x5 corner -- 8 / 12 / 16 filters, non-square windows, the 1 -> C and C -> 1 layers around a wide
// stack -- as implicit GEMMs on the fp32-input matrix instruction v_mfma_f32_16x16x4_f32 (exact fp32: a k-ordered fmaf chain, so
// the fp32 stencil's tolerances hold).  Semantics are those of the generic kernels of conv2d.hip: [B,T,F,C] fp32 maps, HWIO
// kernels, in() = none / lrelu(x*scale+shift) / x*lrelu'(mask_src), time dilation, 'same' or causal padding in time.
//
//   conv_kernel<false>  forward: the halo tile of in(x) (TT + (KT-1) dil rows x Fw + KF-1 columns, zeros for padding) and the
//                       kernel go to the LDS; M = 16 consecutive pixels of the flattened TT x Fw tile, N = Cout padded to 16,
//                       K = (tap, ci) flattened: a K-step is 4 input channels of one tap (Cin = 1: 4 taps of one kernel row).
//   conv_kernel<true>   backward data: the same loop over dy with the taps flipped and the channel roles swapped; the store
//                       applies lrelu'(p) and scale, and sums dscale / dshift per workgroup.
//   wgrad_kernel        dW / dbias: M = 16 rows of the flattened (tap, ci) axis, N = Cout, K = pixels; accumulators stay in
//                       registers over all tiles of a (persistent) workgroup, waves split rows x pixels, one fixed-order
//                       combine through the LDS at the end.
// Weight-side sums leave as rows [nblocks][npart] = dw | dbias | dscale | dshift for ptts_conv2d_reduce_grouped: no atomics here.
#include "common.h"

namespace ptts {
namespace c2w {

typedef float f32x4w __attribute__((ext_vector_type(4)));

constexpr int WTHREADS = 512, WWAVES = WTHREADS / 64;
constexpr int MT = 4;             // conv_kernel: 16-pixel m-tiles a wave carries through one K loop (independent accumulators)
constexpr int MTW = 13;           // wgrad_kernel: 16-row m-tiles of (tap, ci) per wave (49 at 7x7x16, over 4 row groups)
constexpr int MAX_C = 16, MAX_K = 7;
constexpr size_t LDS_TWO = 76 * 1024, LDS_ONE = 150 * 1024;      // two workgroups per CU where a useful tile fits, else one

struct Args {
    const float* in;          // forward: x [B,T,F,CI]; backward data: dy [B,T,F,CI] (CI = the layer's Cout)
    const float* w;           // the layer's kernel [KT][KF][Cin][Cout]
    const float* bias; const float* scale; const float* shift; const float* mask_src;
    const float* xpre;        // backward data: the layer's input x [B,T,F,CO], else NULL
    const float* dy;          // wgrad: dy [B,T,F,CO]
    float* out;               // y / dx (may be NULL in backward data: sums only)
    float* parts;             // partial rows [gridDim.x][npart] or NULL
    int npart, aff_off;
    int B, T, F, CI, CO, KT, KF, dil, pad_t, in_mode;
    float alpha;
    int PS, KFp, TT, Fw, ntt, nfb, Cc, R, ntiles;
    int want_aff;
};

// The halo tile of in(a.in) for tile (b, t0, f0): tile[(r * Cc + c) * PS + ci], zeros outside the image.
__device__ __forceinline__ void stage_tile(const Args& a, float* __restrict__ tile, int b, int t0, int f0, bool transform) {
    const int PF = (a.KF - 1) / 2;
    const int mode = transform ? a.in_mode : PTTS_IN_NONE;
    if (a.CI == 1) {
        const int n = a.R * a.Cc;
        for (int e = threadIdx.x; e < n; e += WTHREADS) {
            const int r = e / a.Cc, c = e - r * a.Cc;
            const int t = t0 + r - a.pad_t, f = f0 + c - PF;
            float v = 0.f;
            if (t >= 0 && t < a.T && f >= 0 && f < a.F) {
                const long long off = ((long long)b * a.T + t) * a.F + f;
                v = a.in[off];
                if (mode == PTTS_IN_LRELU) {
                    if (a.scale) v = v * a.scale[0] + a.shift[0];
                    v = lrelu(v, a.alpha);
                } else if (mode == PTTS_IN_MASKMUL) {
                    v *= lrelu_d(a.mask_src[off], a.alpha);
                }
            }
            tile[e] = v;
        }
        return;
    }
    const int c4n = a.CI >> 2;
    const int n = a.R * a.Cc * c4n;
    for (int e = threadIdx.x; e < n; e += WTHREADS) {
        const int c4 = e % c4n, rc = e / c4n;
        const int r = rc / a.Cc, c = rc - r * a.Cc;
        const int t = t0 + r - a.pad_t, f = f0 + c - PF;
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (t >= 0 && t < a.T && f >= 0 && f < a.F) {
            const long long off = (((long long)b * a.T + t) * a.F + f) * a.CI + 4 * c4;
            v = *reinterpret_cast<const float4*>(a.in + off);
            if (mode == PTTS_IN_LRELU) {
                if (a.scale) {
                    const float4 s = *reinterpret_cast<const float4*>(a.scale + 4 * c4);
                    const float4 h = *reinterpret_cast<const float4*>(a.shift + 4 * c4);
                    v.x = v.x * s.x + h.x; v.y = v.y * s.y + h.y; v.z = v.z * s.z + h.z; v.w = v.w * s.w + h.w;
                }
                v.x = lrelu(v.x, a.alpha); v.y = lrelu(v.y, a.alpha); v.z = lrelu(v.z, a.alpha); v.w = lrelu(v.w, a.alpha);
            } else if (mode == PTTS_IN_MASKMUL) {
                const float4 m = *reinterpret_cast<const float4*>(a.mask_src + off);
                v.x *= lrelu_d(m.x, a.alpha); v.y *= lrelu_d(m.y, a.alpha); v.z *= lrelu_d(m.z, a.alpha); v.w *= lrelu_d(m.w, a.alpha);
            }
        }
        *reinterpret_cast<float4*>(tile + (size_t)rc * a.PS + 4 * c4) = v;
    }
}

__device__ __forceinline__ void tile_coords(const Args& a, int tile_id, int& b, int& t0, int& f0) {
    const int fb = tile_id % a.nfb;
    const int r = tile_id / a.nfb;
    b = r / a.ntt;
    t0 = (r - b * a.ntt) * a.TT;
    f0 = fb * a.Fw;
}

// grid <= ntiles (forward) or the number of partial rows (backward data); WTHREADS threads;
// LDS: kernel [nk][16] | tile [R][Cc][PS] (BWD: its head is reused for the 2 x [WWAVES][16] sums at the end)
template <bool BWD>
__global__ __launch_bounds__(WTHREADS) void conv_kernel(const Args a) {
    extern __shared__ __align__(16) float lds[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int m = lane & 15, k = lane >> 4, n = m, q = k;
    const int nk = a.CI == 1 ? a.KT * a.KFp : a.KT * a.KF * a.CI;      // K, a multiple of 4
    float* wl = lds;
    float* tile = lds + (size_t)nk * 16;
    // the kernel as the B operand: wl[kidx][n], zero for n >= CO and for the taps that pad a Cin = 1 kernel row to 4
    for (int e = tid; e < nk * 16; e += WTHREADS) {
        const int nn = e & 15, kidx = e >> 4;
        int kt, kf, ci;
        if (a.CI == 1) { kt = kidx / a.KFp; kf = kidx - kt * a.KFp; ci = 0; }
        else { ci = kidx % a.CI; const int tap = kidx / a.CI; kt = tap / a.KF; kf = tap - kt * a.KF; }
        float v = 0.f;
        if (nn < a.CO && kf < a.KF) {
            if (!BWD) v = a.w[((kt * a.KF + kf) * a.CI + ci) * a.CO + nn];
            else v = a.w[(((a.KT - 1 - kt) * a.KF + (a.KF - 1 - kf)) * a.CO + nn) * a.CI + ci];
        }
        wl[e] = v;
    }
    const int NP = a.TT * a.Fw;
    const int NG = (NP + 16 * MT - 1) / (16 * MT);
    const float bias_n = (!BWD && a.bias && n < a.CO) ? a.bias[n] : 0.f;
    float sc_n = 1.f, sh_n = 0.f;
    const bool bwd_lrelu = BWD && a.in_mode == PTTS_IN_LRELU;
    if (bwd_lrelu && a.scale && n < a.CO) { sc_n = a.scale[n]; sh_n = a.shift[n]; }
    float s_scale = 0.f, s_shift = 0.f;

    for (int tile_id = blockIdx.x; tile_id < a.ntiles; tile_id += gridDim.x) {
        int b, t0, f0;
        tile_coords(a, tile_id, b, t0, f0);
        __syncthreads();                       // the previous tile's readers (and the kernel staging) are done
        stage_tile(a, tile, b, t0, f0, !BWD);
        __syncthreads();
        for (int g = wave; g < NG; g += WWAVES) {
            int pb[MT];
#pragma unroll
            for (int i = 0; i < MT; ++i) {
                int p = (g * MT + i) * 16 + m;
                if (p > NP - 1) p = NP - 1;
                const int t = p / a.Fw, f = p - t * a.Fw;
                pb[i] = (t * a.Cc + f) * a.PS + k;
            }
            f32x4w acc[MT];
#pragma unroll
            for (int i = 0; i < MT; ++i) acc[i] = f32x4w{0.f, 0.f, 0.f, 0.f};
            const float* wp = wl + k * 16 + n;
            if (a.CI == 1) {
                const int nj = a.KFp >> 2;
                for (int kt = 0; kt < a.KT; ++kt) {
                    const int ro = kt * a.dil * a.Cc;
                    for (int j = 0; j < nj; ++j) {
                        const float bv = *wp; wp += 64;
#pragma unroll
                        for (int i = 0; i < MT; ++i)
                            acc[i] = __builtin_amdgcn_mfma_f32_16x16x4f32(tile[pb[i] + ro + 4 * j], bv, acc[i], 0, 0, 0);
                    }
                }
            } else {
                const int c4n = a.CI >> 2;
                for (int kt = 0; kt < a.KT; ++kt) {
                    for (int kf = 0; kf < a.KF; ++kf) {
                        const int ro = (kt * a.dil * a.Cc + kf) * a.PS;
                        for (int c4 = 0; c4 < c4n; ++c4) {
                            const float bv = *wp; wp += 64;
#pragma unroll
                            for (int i = 0; i < MT; ++i)
                                acc[i] = __builtin_amdgcn_mfma_f32_16x16x4f32(tile[pb[i] + ro + 4 * c4], bv, acc[i], 0, 0, 0);
                        }
                    }
                }
            }
            // C/D layout: col = lane & 15 -> output channel n, row = 4 (lane >> 4) + r -> pixel
#pragma unroll
            for (int i = 0; i < MT; ++i)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int p = (g * MT + i) * 16 + 4 * q + r;
                    const int t = p / a.Fw, f = p - t * a.Fw;
                    if (p < NP && t0 + t < a.T && f0 + f < a.F && n < a.CO) {
                        const long long o = ((((long long)b * a.T + t0 + t) * a.F) + f0 + f) * a.CO + n;
                        float v = acc[i][r];
                        if (!BWD) v += bias_n;
                        else if (bwd_lrelu) {
                            const float xr = a.xpre[o];
                            float pp = xr;
                            if (a.scale) pp = pp * sc_n + sh_n;
                            v *= lrelu_d(pp, a.alpha);
                            s_scale += v * xr;
                            s_shift += v;
                            if (a.scale) v *= sc_n;
                        }
                        if (a.out) a.out[o] = v;
                    }
                }
        }
    }
    if (BWD && a.parts) {
        // dscale | dshift of this workgroup: lanes sharing a channel, then the waves, in a fixed order
        __syncthreads();
        float* red = tile;
        s_scale += __shfl_xor(s_scale, 16, 64); s_scale += __shfl_xor(s_scale, 32, 64);
        s_shift += __shfl_xor(s_shift, 16, 64); s_shift += __shfl_xor(s_shift, 32, 64);
        if (lane < 16) { red[wave * 16 + lane] = s_scale; red[(WWAVES + wave) * 16 + lane] = s_shift; }
        __syncthreads();
        if (tid < 2 * a.CO) {
            const int which = tid / a.CO, c = tid - which * a.CO;
            float s = 0.f;
#pragma unroll
            for (int wv = 0; wv < WWAVES; ++wv) s += red[(which * WWAVES + wv) * 16 + c];
            a.parts[(size_t)blockIdx.x * a.npart + a.aff_off + which * a.CO + c] = a.want_aff ? s : 0.f;
        }
    }
}

// grid = the number of partial rows; WTHREADS threads; CI = the layer's Cin, CO = its Cout.
// LDS: max(tile [R][Cc][PS] | dy [TT*Fw][CO],  combine [nmt*16][16] | bias sums [WWAVES][16])
__global__ __launch_bounds__(WTHREADS, 4) void wgrad_kernel(const Args a) {
    extern __shared__ __align__(16) float lds[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int m = lane & 15, k = lane >> 4, n = m, q = k;
    const int NR = a.KT * a.KF * a.CI, nmt = (NR + 15) >> 4;
    const int WM = nmt <= MTW ? 1 : nmt <= 2 * MTW ? 2 : 4, WK = WWAVES / WM;
    const int wm = wave % WM, wk = wave / WM;
    const int nmine = (nmt - wm + WM - 1) / WM;                   // m-tiles wm, wm + WM, ...
    float* tile = lds;
    float* dyl = lds + (size_t)a.R * a.Cc * a.PS;
    int aoff[MTW];
#pragma unroll
    for (int i = 0; i < MTW; ++i) {
        int rho = 16 * (wm + i * WM) + m;
        if (rho > NR - 1) rho = NR - 1;
        const int ci = rho % a.CI, tap = rho / a.CI;
        const int kt = tap / a.KF, kf = tap - kt * a.KF;
        aoff[i] = (kt * a.dil * a.Cc + kf) * a.PS + ci;
    }
    f32x4w acc[MTW];
#pragma unroll
    for (int i = 0; i < MTW; ++i) acc[i] = f32x4w{0.f, 0.f, 0.f, 0.f};
    float bsum = 0.f;
    const int S = (a.Fw + 3) >> 2, nsteps = a.TT * S;
    const int ndy = a.TT * a.Fw * a.CO;

    for (int tile_id = blockIdx.x; tile_id < a.ntiles; tile_id += gridDim.x) {
        int b, t0, f0;
        tile_coords(a, tile_id, b, t0, f0);
        __syncthreads();
        stage_tile(a, tile, b, t0, f0, true);
        for (int e = tid; e < ndy; e += WTHREADS) {
            const int co = e % a.CO, p = e / a.CO;
            const int t = p / a.Fw, f = p - t * a.Fw;
            float v = 0.f;
            if (t0 + t < a.T && f0 + f < a.F) v = a.dy[((((long long)b * a.T + t0 + t) * a.F) + f0 + f) * a.CO + co];
            dyl[e] = v;
        }
        __syncthreads();
        for (int st = wk; st < nsteps; st += WK) {
            const int t = st / S, f = 4 * (st - t * S) + k;
            const int fc = f < a.Fw ? f : a.Fw - 1;
            const float bv = (f < a.Fw && n < a.CO) ? dyl[(t * a.Fw + f) * a.CO + n] : 0.f;
            const float* ap = tile + (t * a.Cc + fc) * a.PS;
            bsum += bv;
#pragma unroll
            for (int i = 0; i < MTW; ++i)
                if (i < nmine) acc[i] = __builtin_amdgcn_mfma_f32_16x16x4f32(ap[aoff[i]], bv, acc[i], 0, 0, 0);
        }
    }
    // combine the WK pixel groups in a fixed order: red[row][16]
    float* red = lds;
    float* redb = lds + (size_t)nmt * 256;
    for (int phase = 0; phase < WK; ++phase) {
        __syncthreads();
        if (wk == phase) {
#pragma unroll
            for (int i = 0; i < MTW; ++i)
                if (i < nmine) {
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const int idx = ((wm + i * WM) * 16 + 4 * q + r) * 16 + n;
                        red[idx] = phase == 0 ? acc[i][r] : red[idx] + acc[i][r];
                    }
                }
        }
    }
    bsum += __shfl_xor(bsum, 16, 64); bsum += __shfl_xor(bsum, 32, 64);
    if (wm == 0 && lane < 16) redb[wk * 16 + lane] = bsum;
    __syncthreads();
    float* out = a.parts + (size_t)blockIdx.x * a.npart;
    const int nw = NR * a.CO;
    for (int j = tid; j < nw; j += WTHREADS) {
        const int co = j % a.CO, rho = j / a.CO;
        out[j] = red[rho * 16 + co];
    }
    if (tid < a.CO) {
        float s = 0.f;
        for (int g = 0; g < WK; ++g) s += redb[g * 16 + tid];
        out[nw + tid] = s;
    }
}

// ------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------
static int host_pix_stride(int c) { return c == 1 ? 1 : (((c >> 2) & 1) ? c : c + 4); }

struct Plan { bool ok; int TT, Fw, ntt, nfb, PS, KFp, Cc, R; size_t lds; };

// The tile of a kernel whose LDS holds `fixed` bytes whatever the tile, the halo tile of CI channels and `extra` floats per
// owned pixel: the (TT, Fw) with the most owned pixels per staged pixel under 76 KB (two workgroups a CU), else under 150 KB.
static Plan plan(int T, int F, int CI, int KT, int KF, int dil, size_t fixed, int extra, size_t floor_bytes) {
    Plan best{};
    best.ok = false;
    const int PS = host_pix_stride(CI), KFp = CI == 1 ? (KF + 3) / 4 * 4 : KF, halo = (KT - 1) * dil;
    for (int pass = 0; pass < 2 && !best.ok; ++pass) {
        const size_t budget = pass == 0 ? LDS_TWO : LDS_ONE;
        if (fixed >= budget) continue;
        double best_eff = 0.0;
        for (int nfb = 1; nfb <= 32; ++nfb) {
            const int Fw = (F + nfb - 1) / nfb;
            if ((F + Fw - 1) / Fw != nfb) continue;                   // the same width came with fewer blocks
            const int Cc = Fw + KFp - 1;
            const size_t row = (size_t)Cc * PS * 4, own = (size_t)Fw * extra * 4;
            const size_t avail = budget - fixed;
            if (avail < (size_t)(halo + 1) * row + own) { if (Fw == 1) break; continue; }
            int TT = (int)((avail - (size_t)halo * row) / (row + own));
            if (TT > T) TT = T;
            if (TT > 64) TT = 64;
            const int ntt = (T + TT - 1) / TT;
            TT = (T + ntt - 1) / ntt;
            const double eff = ((double)T * F) / ((double)ntt * nfb * (TT + halo) * Cc);
            if (eff > best_eff * 1.02) {
                best_eff = eff;
                best.ok = true; best.TT = TT; best.Fw = Fw; best.ntt = ntt; best.nfb = nfb;
                best.PS = PS; best.KFp = KFp; best.Cc = Cc; best.R = TT + halo;
                best.lds = fixed + (size_t)best.R * row + (size_t)TT * own;
            }
            if (Fw == 1) break;
        }
        // a short tile under a tall halo re-stages most of what it reads: give the workgroup the whole LDS instead
        if (pass == 0 && best.ok && best.TT < T && best.TT < 2 * halo) best.ok = false;
    }
    if (best.ok && best.lds < floor_bytes) best.lds = floor_bytes;
    return best;
}

static size_t kernel_bytes(int CI, int KT, int KF) {
    return (size_t)(CI == 1 ? KT * ((KF + 3) / 4 * 4) : KT * KF * CI) * 16 * 4;
}
static Plan plan_conv(int T, int F, int CI, int KT, int KF, int dil) {
    return plan(T, F, CI, KT, KF, dil, kernel_bytes(CI, KT, KF), 0, 2 * WWAVES * 16 * 4 + kernel_bytes(CI, KT, KF));
}
static Plan plan_wgrad(int T, int F, int Cin, int Cout, int KT, int KF, int dil) {
    const int nmt = (KT * KF * Cin + 15) / 16;
    return plan(T, F, Cin, KT, KF, dil, 0, Cout, ((size_t)nmt * 256 + WWAVES * 16) * 4);
}

static bool chan_ok(int c) { return c == 1 || (c % 4 == 0 && c >= 4 && c <= MAX_C); }
static bool win_ok(int kk) { return kk >= 3 && kk <= MAX_K && (kk & 1); }
// the shapes the packed-FMA stencil (PTTS_CONV_CASES) and the 4 -> 4 5x5 matrix-core kernels take
static bool taken_elsewhere(int Cin, int Cout, int KT, int KF) {
    const bool small = (Cin == 1 || Cin == 2 || Cin == 4) && (Cout == 1 || Cout == 2 || Cout == 4);
    return small && KT == KF && (KT == 3 || KT == 5);
}

static bool supported(int F, int Cin, int Cout, int KT, int KF, int dil) {
    if (F <= 0 || dil <= 0 || !chan_ok(Cin) || !chan_ok(Cout) || !win_ok(KT) || !win_ok(KF)) return false;
    if (taken_elsewhere(Cin, Cout, KT, KF)) return false;
    if ((long long)(KT - 1) * dil > 4096) return false;
    const int T = 1 << 20;
    return plan_conv(T, F, Cin, KT, KF, dil).ok && plan_conv(T, F, Cout, KT, KF, dil).ok &&
           plan_wgrad(T, F, Cin, Cout, KT, KF, dil).ok;
}

static void fill_geometry(Args& a, const Plan& p, int B) {
    a.PS = p.PS; a.KFp = p.KFp; a.TT = p.TT; a.Fw = p.Fw; a.ntt = p.ntt; a.nfb = p.nfb; a.Cc = p.Cc; a.R = p.R;
    a.ntiles = B * p.ntt * p.nfb;
}

enum { K_FWD = 0, K_BWD_DATA = 1, K_WGRAD = 2 };
// (the LDS limit of a kernel is raised once, before its first launch: not an operation of the stream, so not inside a capture either)
static int launch(void (*kernel)(const Args), int id, const char* what, const Args& a, int grid, size_t lds, hipStream_t st) {
    static bool attr[3] = {false, false, false};
    if (!attr[id]) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)LDS_ONE);
        if (e != hipSuccess) { set_error("%s: hipFuncSetAttribute: %s", what, hipGetErrorString(e)); return PTTS_ELAUNCH; }
        attr[id] = true;
    }
    hipLaunchKernelGGL(kernel, dim3(grid), dim3(WTHREADS), lds, st, a);
    return check_launch(what);
}

static int pad_of(int KT, int dil, int pad_mode) {
    const int span = (KT - 1) * dil;
    return pad_mode == PTTS_PAD_CAUSAL ? span : span / 2;
}

// rows of partial sums a backward pass leaves: one per (persistent) workgroup; 256 keeps the grouped reduction to two
// slabs, whose sum does not depend on their order (deterministic mode)
static int rows_for(int B, int T, int F, int Cin, int Cout, int KT, int KF, int dil) {
    const Plan pw = plan_wgrad(T, F, Cin, Cout, KT, KF, dil), pd = plan_conv(T, F, Cout, KT, KF, dil);
    long long nt = (long long)B * pw.ntt * pw.nfb, nd = (long long)B * pd.ntt * pd.nfb;
    if (nd > nt) nt = nd;
    const int cap = deterministic() ? 256 : 512;
    return (int)(nt < cap ? nt : cap);
}

}  // namespace c2w
}  // namespace ptts

using namespace ptts;
using namespace ptts::c2w;

static bool aligned16(const void* p) { return ((size_t)p & 15) == 0; }

extern "C" int ptts_conv2d_wide_supported(int F, int Cin, int Cout, int KT, int KF, int dil_t) {
    return supported(F, Cin, Cout, KT, KF, dil_t) ? 1 : 0;
}

extern "C" int ptts_conv2d_wide_fwd(const float* x, const float* w, const float* bias, const float* in_scale,
                                    const float* in_shift, const float* mask_src, float* y, int B, int T, int F, int Cin,
                                    int Cout, int KT, int KF, int dil_t, int pad_mode, int in_mode, float alpha, void* stream) {
    PTTS_REQUIRE(x && w && y, "conv2d_wide_fwd: null tensor");
    PTTS_REQUIRE(B > 0 && T > 0 && F > 0 && Cin > 0 && Cout > 0 && KT > 0 && KF > 0 && dil_t > 0,
                 "conv2d_wide_fwd: bad dims B=%d T=%d F=%d Cin=%d Cout=%d KT=%d KF=%d dil=%d", B, T, F, Cin, Cout, KT, KF, dil_t);
    PTTS_REQUIRE(in_mode >= 0 && in_mode <= 2, "conv2d_wide_fwd: bad in_mode %d", in_mode);
    PTTS_REQUIRE(pad_mode == PTTS_PAD_SAME || pad_mode == PTTS_PAD_CAUSAL, "conv2d_wide_fwd: bad pad_mode %d", pad_mode);
    PTTS_REQUIRE((in_scale == nullptr) == (in_shift == nullptr), "conv2d_wide_fwd: scale/shift must come together");
    PTTS_REQUIRE(in_mode != PTTS_IN_MASKMUL || mask_src, "conv2d_wide_fwd: MASKMUL needs mask_src");
    PTTS_REQUIRE((long long)B * T * F * 16 < (1LL << 31), "conv2d_wide_fwd: map too large");
    PTTS_REQUIRE(supported(F, Cin, Cout, KT, KF, dil_t),
                 "conv2d_wide_fwd: unsupported shape F=%d Cin=%d Cout=%d KT=%d KF=%d dil=%d (ptts_conv2d_wide_supported)", F, Cin, Cout, KT, KF, dil_t);
    PTTS_REQUIRE(aligned16(x) && aligned16(in_scale) && aligned16(in_shift) && aligned16(mask_src),
                 "conv2d_wide_fwd: x, in_scale, in_shift and mask_src must be 16-byte aligned");
    const Plan p = plan_conv(T, F, Cin, KT, KF, dil_t);
    PTTS_REQUIRE(p.ok, "conv2d_wide_fwd: no tile fits");
    Args a{};
    a.in = x; a.w = w; a.bias = bias; a.scale = in_scale; a.shift = in_shift; a.mask_src = mask_src; a.out = y;
    a.B = B; a.T = T; a.F = F; a.CI = Cin; a.CO = Cout; a.KT = KT; a.KF = KF; a.dil = dil_t;
    a.pad_t = pad_of(KT, dil_t, pad_mode); a.in_mode = in_mode; a.alpha = alpha;
    fill_geometry(a, p, B);
    const int cap = p.lds <= LDS_TWO ? 512 : 256;
    return launch(conv_kernel<false>, K_FWD, "conv2d_wide_fwd", a, a.ntiles < cap ? a.ntiles : cap, p.lds, (hipStream_t)stream);
}

extern "C" size_t ptts_conv2d_wide_bwd_workspace_bytes(int B, int T, int F, int Cin, int Cout, int KT, int KF, int dil_t) {
    if (B <= 0 || T <= 0 || !supported(F, Cin, Cout, KT, KF, dil_t)) return 0;
    // the row count outside deterministic mode, the larger of the two
    const Plan pw = plan_wgrad(T, F, Cin, Cout, KT, KF, dil_t), pd = plan_conv(T, F, Cout, KT, KF, dil_t);
    long long nt = (long long)B * pw.ntt * pw.nfb, nd = (long long)B * pd.ntt * pd.nfb;
    if (nd > nt) nt = nd;
    const long long rows = nt < 512 ? nt : 512;
    return (size_t)rows * (size_t)(KT * KF * Cin * Cout + Cout + 2 * Cin) * sizeof(float);
}

extern "C" int ptts_conv2d_wide_bwd_partials(const float* dy, const float* x, const float* w, const float* in_scale,
                                             const float* in_shift, const float* mask_src, float* dx, void* workspace,
                                             size_t workspace_bytes, int* nblocks_out, int* npart_out, int want_dw,
                                             int want_affine, int B, int T, int F, int Cin, int Cout, int KT, int KF,
                                             int dil_t, int pad_mode, int in_mode, float alpha, void* stream) {
    PTTS_REQUIRE(dy && x && w, "conv2d_wide_bwd: null tensor");
    PTTS_REQUIRE(nblocks_out && npart_out, "conv2d_wide_bwd: nblocks_out / npart_out is NULL");
    PTTS_REQUIRE(B > 0 && T > 0 && F > 0 && Cin > 0 && Cout > 0 && KT > 0 && KF > 0 && dil_t > 0, "conv2d_wide_bwd: bad dims");
    PTTS_REQUIRE(in_mode >= 0 && in_mode <= 2, "conv2d_wide_bwd: bad in_mode %d", in_mode);
    PTTS_REQUIRE(pad_mode == PTTS_PAD_SAME || pad_mode == PTTS_PAD_CAUSAL, "conv2d_wide_bwd: bad pad_mode %d", pad_mode);
    PTTS_REQUIRE((in_scale == nullptr) == (in_shift == nullptr), "conv2d_wide_bwd: scale/shift must come together");
    PTTS_REQUIRE(in_mode != PTTS_IN_MASKMUL || mask_src, "conv2d_wide_bwd: MASKMUL needs mask_src");
    PTTS_REQUIRE(!(in_mode == PTTS_IN_MASKMUL && dx), "conv2d_wide_bwd: dx is not defined for MASKMUL (weight-only sweep)");
    PTTS_REQUIRE(!want_affine || (in_mode == PTTS_IN_LRELU && in_scale), "conv2d_wide_bwd: dscale needs LRELU with scale/shift");
    PTTS_REQUIRE((long long)B * T * F * 16 < (1LL << 31), "conv2d_wide_bwd: map too large");
    PTTS_REQUIRE(supported(F, Cin, Cout, KT, KF, dil_t),
                 "conv2d_wide_bwd: unsupported shape F=%d Cin=%d Cout=%d KT=%d KF=%d dil=%d (ptts_conv2d_wide_supported)", F, Cin, Cout, KT, KF, dil_t);
    PTTS_REQUIRE(aligned16(dy) && aligned16(x) && aligned16(in_scale) && aligned16(in_shift) && aligned16(mask_src),
                 "conv2d_wide_bwd: dy, x, in_scale, in_shift and mask_src must be 16-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    const int nw = KT * KF * Cin * Cout, npart = nw + Cout + 2 * Cin;
    const bool sums = want_dw || want_affine;
    const int rows = rows_for(B, T, F, Cin, Cout, KT, KF, dil_t);
    *nblocks_out = sums ? rows : 0;
    *npart_out = npart;
    if (!dx && !sums) return PTTS_OK;
    if (sums) {
        const size_t need = (size_t)rows * npart * sizeof(float);
        if (!workspace || workspace_bytes < need) {
            set_error("conv2d_wide_bwd: workspace %zu < %zu", workspace_bytes, need);
            return PTTS_EWORKSPACE;
        }
    }
    const int span = (KT - 1) * dil_t, pad_t = pad_of(KT, dil_t, pad_mode);
    if (dx || want_affine || sums) {
        // backward data over dy (taps flipped, channel roles swapped); it also writes the dscale | dshift columns of every row
        const Plan p = plan_conv(T, F, Cout, KT, KF, dil_t);
        PTTS_REQUIRE(p.ok, "conv2d_wide_bwd: no tile fits");
        if (dx || want_affine) {
            Args a{};
            a.in = dy; a.w = w; a.scale = in_scale; a.shift = in_shift; a.xpre = x; a.out = dx;
            a.parts = sums ? (float*)workspace : nullptr; a.npart = npart; a.aff_off = nw + Cout; a.want_aff = want_affine;
            a.B = B; a.T = T; a.F = F; a.CI = Cout; a.CO = Cin; a.KT = KT; a.KF = KF; a.dil = dil_t;
            a.pad_t = span - pad_t; a.in_mode = in_mode; a.alpha = alpha;
            fill_geometry(a, p, B);
            int grid = rows;
            if (!sums) { const int cap = p.lds <= LDS_TWO ? 512 : 256; grid = a.ntiles < cap ? a.ntiles : cap; }
            const int rc = launch(conv_kernel<true>, K_BWD_DATA, "conv2d_wide_bwd_data", a, grid, p.lds, st);
            if (rc) return rc;
        }
    }
    if (want_dw) {
        const Plan p = plan_wgrad(T, F, Cin, Cout, KT, KF, dil_t);
        PTTS_REQUIRE(p.ok, "conv2d_wide_bwd: no tile fits");
        Args a{};
        a.in = x; a.w = w; a.scale = in_scale; a.shift = in_shift; a.mask_src = mask_src; a.dy = dy;
        a.parts = (float*)workspace; a.npart = npart; a.aff_off = nw + Cout;
        a.B = B; a.T = T; a.F = F; a.CI = Cin; a.CO = Cout; a.KT = KT; a.KF = KF; a.dil = dil_t;
        a.pad_t = pad_t; a.in_mode = in_mode; a.alpha = alpha;
        fill_geometry(a, p, B);
        const int rc = launch(wgrad_kernel, K_WGRAD, "conv2d_wide_wgrad", a, rows, p.lds, st);
        if (rc) return rc;
    }
    return PTTS_OK;
}
