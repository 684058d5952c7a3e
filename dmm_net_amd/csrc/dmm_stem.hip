// The 7x7 / stride 2 / padding 3 STEM convolution (3 -> 64) of the training encoder for the DETERMINISTIC mode: forward and
// weight gradient on MFMA (include/dmm_match.h (10f); dmm_net_amd/train_encoder.py, set_deterministic_conv("own_stem")).
//
// Why a kernel of its own.  Three input channels are 6-byte pixels: the 16-byte operand pieces of dmm_conv.hip / dmm_wgrad.hip
// do not exist here, and an image row of 6 W bytes has only 2-byte alignment.  What does exist: for ONE kernel row the
// 7 taps x 3 channels = 21 values of a window are contiguous in the image row.  So the reduction is laid out as
//     K = 7 kernel rows x 32 lanes  (21 real, 11 that are ZERO on both operands)
// and a 64-pixel stage of it is built in LDS by 2-byte loads -- a value outside the image or beyond the last pixel is loaded
// from a valid address (the tensor's first element) and replaced by an exact zero on its way to LDS, and the lanes k >= 21 are
// zeroed once and never written again: whatever sits in memory around the tensor, or in the tensor next to a window, cannot
// reach a product.  The loads of the NEXT stage are issued into registers before the MFMAs of the current one and written to
// LDS after them.  The image (8 MB at 12 x 255 x 448) stays in the caches; the kernels move their 44 MB of y / dy once.
//
// Forward (stem_conv_kernel): implicit GEMM [64 co] x [64 pixels] per stage on mfma_f32_32x32x16_bf16, 14 k-steps (7 kernel
// rows x 2), one 32 x 32 tile per wave, no split of the reduction: the summation order of an output element is a function of
// nothing but the position of a term in the 147-term reduction -- an image's bits do not depend on its batch.  A workgroup
// stages the weights once and walks a run of consecutive pixel tiles (at most STEM_FWD_WGS workgroups share the tiles).
// Bias added in fp32, ONE rounding, 16-byte stores through LDS.
//
// Weight gradient (stem_wgrad_kernel + stem_wgrad_fold_kernel): dw = dy^T [64, pixels] x patches [pixels, 7 x 32], the
// pixels on the MFMA's k.  Both operands are written TRANSPOSED into LDS ([column][pixel], so that a fragment's 8 pixels are
// 16 contiguous bytes); a workgroup owns a slab of consecutive 64-pixel chunks and keeps its [64, 7 x 32] tile in
// accumulators (wave = one half of the channels x every other kernel row), then stores the 147 real columns as an fp32
// partial table.  The fold sums the tables in slab order (four interleaved slices, then a fixed-order add) into the
// parameter's own [64, 3, 7, 7] layout.  The slab count is a function of (B, H, W) alone; no atomics, nothing to zero.
#include "dmm_common.h"

namespace dmm {

typedef __bf16 bf16x8s __attribute__((ext_vector_type(8)));
typedef float f32x16s __attribute__((ext_vector_type(16)));
typedef uint32_t u32x4s __attribute__((ext_vector_type(4)));
typedef uint32_t u32x2s __attribute__((ext_vector_type(2)));

constexpr int STEM_PX = 64;              // output pixels per stage
constexpr int STEM_KR = 32;              // K lanes per kernel row
constexpr int STEM_KREAL = 21;           // of which real: 7 taps x 3 channels
constexpr int STEM_CO = 64;
constexpr int STEM_CV = 147;             // 7 x 7 x 3
constexpr int STEM_FWD_WGS = 512;        // forward: at most this many workgroups, each a run of pixel tiles (weights staged once)
constexpr int STEM_SLABS = 256;          // weight gradient: at most this many slabs (one workgroup each)
constexpr int STEM_TLD = STEM_PX + 8;    // row length of the transposed LDS images: 144 bytes, 16-byte aligned rows

__device__ __forceinline__ uint32_t stem_bf16_rne(float v) {
    const uint32_t u = __float_as_uint(v);
    if ((u & 0x7fffffffu) > 0x7f800000u) return (u >> 16) | 0x40u;
    return (u + 0x7fffu + ((u >> 16) & 1u)) >> 16;
}

// element offset of lane k (0..31) of (kernel row kh, row r) in a [7][64][32] bf16 LDS image; the 16-byte pieces of a row
// are swizzled by the row so that the 32 rows a fragment read touches spread over the banks
__device__ __forceinline__ int stem_at(int kh, int r, int k) {
    return (kh * 64 + r) * STEM_KR + ((((k >> 3) ^ ((r >> 2) & 3)) << 3) | (k & 7));
}

// What the staging needs to know of the 64 output pixels m0 .. m0 + 63, computed by 64 threads once per stage.
struct StemPixels {
    int64_t base[STEM_PX];               // element offset of x[b, 2ho - 3, 2wo - 3, 0] (may lie outside: never dereferenced there)
    int h0[STEM_PX], w0[STEM_PX];        // 2ho - 3 (far below zero for a pixel beyond M: every row fails), 2wo - 3
};

__device__ __forceinline__ void stem_pixels(StemPixels &px, int64_t m0, int64_t M, int H, int W, int Ho, int Wo) {
    const int p = threadIdx.x;
    if (p >= STEM_PX) return;
    const int64_t m = m0 + p;
    const bool in = m < M;
    const int64_t mm = in ? m : 0;
    const int64_t q = mm / Wo;
    const int wo = (int)(mm - q * Wo);
    const int b = (int)(q / Ho);
    const int ho = (int)(q - (int64_t)b * Ho);
    px.h0[p] = in ? 2 * ho - 3 : -(1 << 20);
    px.w0[p] = 2 * wo - 3;
    px.base[p] = (((int64_t)b * H + (2 * ho - 3)) * W + (2 * wo - 3)) * 3;
}

// The patch rows of a stage, first half: this thread's values into registers.  Element (kh, p, k) = x[b, 2ho + kh - 3,
// 2wo - 3 + k / 3, k % 3] where the position lies inside the image and the pixel below M, else ZERO -- loaded from x[0] (a
// valid address) and replaced, so no load is predicated and all of them can be in flight at once.  Thread = one k < 21 and
// 8 pixels; the threads of k >= 21 fetch nothing.
__device__ __forceinline__ void stem_fetch(const uint16_t *__restrict__ x, const StemPixels &px, int H, int W,
                                           uint32_t (&v)[STEM_PX / 8][7]) {
    const int k = threadIdx.x & 31, p0 = threadIdx.x >> 5;
    if (k >= STEM_KREAL) return;
    const int kw = k / 3;
    const int64_t row = (int64_t)W * 3;
#pragma unroll
    for (int n = 0; n < STEM_PX / 8; ++n) {
        const int p = p0 + 8 * n;
        const int hi0 = px.h0[p], wi = px.w0[p] + kw;
        const bool col_in = wi >= 0 && wi < W;
        const int64_t base = px.base[p] + k;
#pragma unroll
        for (int kh = 0; kh < 7; ++kh) {
            const int hi = hi0 + kh;
            const bool ok = col_in && hi >= 0 && hi < H;
            const uint32_t got = x[ok ? base + kh * row : (int64_t)0];
            v[n][kh] = ok ? got : 0u;
        }
    }
}

// second half: the registers into the LDS image, element (kh, p, k) at lds[at(kh, p, k)]
template <class At>
__device__ __forceinline__ void stem_stash(const uint32_t (&v)[STEM_PX / 8][7], uint16_t *lds, At at) {
    const int k = threadIdx.x & 31, p0 = threadIdx.x >> 5;
    if (k >= STEM_KREAL) return;
#pragma unroll
    for (int n = 0; n < STEM_PX / 8; ++n)
#pragma unroll
        for (int kh = 0; kh < 7; ++kh) lds[at(kh, p0 + 8 * n, k)] = (uint16_t)v[n][kh];
}

// once per workgroup: the lanes k >= 21 of every (kh, p) are zero and stay zero (stem_stash never writes them)
template <class At>
__device__ __forceinline__ void stem_zero_pads(uint16_t *lds, At at) {
    const int k = threadIdx.x & 31, p0 = threadIdx.x >> 5;
    if (k < STEM_KREAL) return;
#pragma unroll
    for (int n = 0; n < STEM_PX / 8; ++n)
#pragma unroll
        for (int kh = 0; kh < 7; ++kh) lds[at(kh, p0 + 8 * n, k)] = 0;
}

__global__ __launch_bounds__(256) void stem_conv_kernel(const uint16_t *__restrict__ x, const uint16_t *__restrict__ w,
                                                        const uint16_t *__restrict__ bias, uint16_t *__restrict__ y, int H,
                                                        int W, int Ho, int Wo, int64_t M, int64_t tiles,
                                                        int64_t tiles_per_wg) {
    constexpr int OUT_LD = STEM_CO + 8;
    __shared__ __attribute__((aligned(16))) uint16_t ws_[7 * STEM_CO * STEM_KR];     // [kh][co][32]
    __shared__ __attribute__((aligned(16))) uint16_t xs_[7 * STEM_PX * STEM_KR];     // [kh][pixel][32]
    __shared__ __attribute__((aligned(16))) uint16_t os_[STEM_PX * OUT_LD];          // the output image of a stage
    __shared__ StemPixels px[2];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int r = lane & 31, h = lane >> 5;
    const int wco = wave & 1, wpx = wave >> 1;

    {   // the weights [co][kh][21] -> [kh][co][32], lanes 21..31 zero
        const int k = t & 31;
#pragma unroll
        for (int n = 0; n < STEM_CO / 8; ++n) {
            const int co = (t >> 5) + 8 * n;
#pragma unroll
            for (int kh = 0; kh < 7; ++kh) {
                uint16_t v = 0;
                if (k < STEM_KREAL) v = w[co * STEM_CV + kh * STEM_KREAL + k];
                ws_[stem_at(kh, co, k)] = v;
            }
        }
    }
    // D layout: column (the pixel side) = lane & 31, row (the channel side) = (reg & 3) + 8 * (reg >> 2) + 4 * (lane >> 5)
    float bv[4][4];
#pragma unroll
    for (int g4 = 0; g4 < 4; ++g4)
#pragma unroll
        for (int e = 0; e < 4; ++e)
            bv[g4][e] = bias ? __uint_as_float((uint32_t)bias[wco * 32 + 8 * g4 + 4 * h + e] << 16) : 0.0f;

    const auto at = [](int kh, int p, int k) { return stem_at(kh, p, k); };
    stem_zero_pads(xs_, at);
    const int64_t tile0 = (int64_t)blockIdx.x * tiles_per_wg;
    int64_t tile1 = tile0 + tiles_per_wg;
    if (tile1 > tiles) tile1 = tiles;
    uint32_t v[STEM_PX / 8][7];
    stem_pixels(px[0], tile0 * STEM_PX, M, H, W, Ho, Wo);
    __syncthreads();
    stem_fetch(x, px[0], H, W, v);
    int cur = 0;
    for (int64_t tile = tile0; tile < tile1; ++tile) {     // (the same run for every thread of the workgroup)
        const int64_t m0 = tile * STEM_PX;
        const bool more = tile + 1 < tile1;
        stem_stash(v, xs_, at);                            // (the previous stage's reads of xs_ ended before its second barrier)
        if (more) stem_pixels(px[cur ^ 1], m0 + STEM_PX, M, H, W, Ho, Wo);
        __syncthreads();                                   // (and: the previous stage's reads of os_ are done)
        if (more) stem_fetch(x, px[cur ^ 1], H, W, v);     // in flight during the MFMAs and the stores below
        cur ^= 1;
        f32x16s acc;
#pragma unroll
        for (int q = 0; q < 16; ++q) acc[q] = 0.0f;
#pragma unroll
        for (int kh = 0; kh < 7; ++kh)
#pragma unroll
            for (int s = 0; s < 2; ++s) {
                const bf16x8s fa = *reinterpret_cast<const bf16x8s *>(ws_ + stem_at(kh, wco * 32 + r, 16 * s + 8 * h));
                const bf16x8s fb = *reinterpret_cast<const bf16x8s *>(xs_ + stem_at(kh, wpx * 32 + r, 16 * s + 8 * h));
                acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa, fb, acc, 0, 0, 0);
            }
        const int pl = wpx * 32 + r;
#pragma unroll
        for (int g4 = 0; g4 < 4; ++g4) {
            const int cl = wco * 32 + 8 * g4 + 4 * h;
            u32x2s o;
            o[0] = stem_bf16_rne(acc[4 * g4] + bv[g4][0]) | (stem_bf16_rne(acc[4 * g4 + 1] + bv[g4][1]) << 16);
            o[1] = stem_bf16_rne(acc[4 * g4 + 2] + bv[g4][2]) | (stem_bf16_rne(acc[4 * g4 + 3] + bv[g4][3]) << 16);
            *reinterpret_cast<u32x2s *>(os_ + pl * OUT_LD + cl) = o;
        }
        __syncthreads();
#pragma unroll
        for (int n = 0; n < STEM_PX * (STEM_CO / 8) / 256; ++n) {
            const int idx = t + 256 * n, po = idx >> 3, p8 = idx & 7;
            const int64_t m = m0 + po;
            if (m < M)
                *reinterpret_cast<u32x4s *>(y + m * STEM_CO + 8 * p8) = *reinterpret_cast<const u32x4s *>(os_ + po * OUT_LD + 8 * p8);
        }
    }
}

// part[blockIdx.x][co][kh * 21 + k] = sum over the slab's pixels of dy[pixel][co] * patch[pixel][kh][k]
__global__ __launch_bounds__(256) void stem_wgrad_kernel(const uint16_t *__restrict__ dy, const uint16_t *__restrict__ x,
                                                         float *__restrict__ part, int H, int W, int Ho, int Wo, int64_t M,
                                                         int64_t chunks, int64_t chunks_per_slab) {
    __shared__ __attribute__((aligned(16))) uint16_t ps_[7 * STEM_KR * STEM_TLD];    // [kh * 32 + k][pixel]
    __shared__ __attribute__((aligned(16))) uint16_t ds_[STEM_CO * STEM_TLD];        // [co][pixel]
    __shared__ StemPixels px[2];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int r = lane & 31, h = lane >> 5;
    const int ct = wave & 1, kh0 = wave >> 1;              // this wave: channels 32 ct .. + 31, kernel rows kh0, kh0 + 2, ...
    f32x16s acc[4];
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int q = 0; q < 16; ++q) acc[j][q] = 0.0f;
    const int64_t c0 = (int64_t)blockIdx.x * chunks_per_slab;
    int64_t c1 = c0 + chunks_per_slab;
    if (c1 > chunks) c1 = chunks;
    const auto at = [](int kh, int p, int k) { return (kh * STEM_KR + k) * STEM_TLD + p; };
    // this thread's dy pieces of a chunk: 8 channels of pixel (t + 256 n) >> 3; beyond M a valid address, replaced by zero
    const auto fetch_dy = [&](int64_t m0, u32x4s (&d)[2]) {
#pragma unroll
        for (int n = 0; n < 2; ++n) {
            const int idx = t + 256 * n;
            const int64_t m = m0 + (idx >> 3);
            const bool ok = m < M;
            const u32x4s got = *reinterpret_cast<const u32x4s *>(dy + (ok ? m * STEM_CO + 8 * (idx & 7) : (int64_t)0));
            const u32x4s z = {0u, 0u, 0u, 0u};
            d[n] = ok ? got : z;
        }
    };
    stem_zero_pads(ps_, at);
    uint32_t v[STEM_PX / 8][7];
    u32x4s d[2];
    stem_pixels(px[0], c0 * STEM_PX, M, H, W, Ho, Wo);
    __syncthreads();
    stem_fetch(x, px[0], H, W, v);
    fetch_dy(c0 * STEM_PX, d);
    int cur = 0;
    for (int64_t c = c0; c < c1; ++c) {
        const int64_t m0 = c * STEM_PX;
        const bool more = c + 1 < c1;
        stem_stash(v, ps_, at);                            // (the previous chunk's fragment reads ended before its second barrier)
#pragma unroll
        for (int n = 0; n < 2; ++n) {
            const int idx = t + 256 * n, p = idx >> 3, c8 = idx & 7;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                ds_[(8 * c8 + 2 * e) * STEM_TLD + p] = (uint16_t)(d[n][e] & 0xFFFFu);
                ds_[(8 * c8 + 2 * e + 1) * STEM_TLD + p] = (uint16_t)(d[n][e] >> 16);
            }
        }
        if (more) stem_pixels(px[cur ^ 1], m0 + STEM_PX, M, H, W, Ho, Wo);
        __syncthreads();
        if (more) {                                        // in flight during the MFMAs below
            stem_fetch(x, px[cur ^ 1], H, W, v);
            fetch_dy(m0 + STEM_PX, d);
        }
        cur ^= 1;
#pragma unroll
        for (int s = 0; s < STEM_PX / 16; ++s) {
            const bf16x8s fa = *reinterpret_cast<const bf16x8s *>(ds_ + (ct * 32 + r) * STEM_TLD + 16 * s + 8 * h);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int kh = kh0 + 2 * j;
                if (kh < 7) {
                    const bf16x8s fb = *reinterpret_cast<const bf16x8s *>(ps_ + (kh * STEM_KR + r) * STEM_TLD + 16 * s + 8 * h);
                    acc[j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa, fb, acc[j], 0, 0, 0);
                }
            }
        }
        __syncthreads();                                   // (the fragment reads are done: the next chunk may be stashed)
    }
    // D layout: column (the patch side) = lane & 31, row (the channel side) = (reg & 3) + 8 * (reg >> 2) + 4 * (lane >> 5)
    float *o = part + (int64_t)blockIdx.x * (STEM_CO * STEM_CV);
    if (r >= STEM_KREAL) return;                           // (the zero lanes of a kernel row: no column of dw)
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int kh = kh0 + 2 * j;
        if (kh < 7) {
#pragma unroll
            for (int reg = 0; reg < 16; ++reg) {
                const int co = ct * 32 + (reg & 3) + 8 * (reg >> 2) + 4 * h;
                o[co * STEM_CV + kh * STEM_KREAL + r] = acc[j][reg];
            }
        }
    }
}

// dw[co, ci, kh, kw] = sum over the slabs, in slab order, of part[slab][co][(kh * 7 + kw) * 3 + ci]: four slices take the
// slabs round robin, their sums are added in slice order.  9408 outputs = 147 workgroups of 64.
__global__ __launch_bounds__(256) void stem_wgrad_fold_kernel(const float *__restrict__ part, int slabs, float *__restrict__ dw) {
    __shared__ float fold[4][64];
    const int o = threadIdx.x & 63, sl = threadIdx.x >> 6;
    const int j = blockIdx.x * 64 + o;
    const int co = j / STEM_CV, rem = j - co * STEM_CV;
    const int ci = rem / 49, tap = rem - ci * 49;
    const float *p = part + co * STEM_CV + tap * 3 + ci;
    float acc = 0.0f;
    for (int g = sl; g < slabs; g += 4) acc += p[(int64_t)g * (STEM_CO * STEM_CV)];
    fold[sl][o] = acc;
    __syncthreads();
    if (sl == 0) dw[j] = ((fold[0][o] + fold[1][o]) + fold[2][o]) + fold[3][o];
}

struct StemGeom {
    int Ho, Wo;
    int64_t M, chunks, chunks_per_slab, slabs;
};

// (B * H * W <= 2^56: every element and byte offset of x, y and dy fits an int64 with room to spare)
static bool stem_sizes_ok(int B, int H, int W) {
    return B >= 0 && H > 0 && W > 0 && (B == 0 || (int64_t)H * W <= (1LL << 56) / B);
}

// (B, H, W) -> the pixel chunks and the slabs of the weight gradient: a function of nothing else
static StemGeom stem_geom(int B, int H, int W) {
    StemGeom g;
    g.Ho = (H - 1) / 2 + 1;
    g.Wo = (W - 1) / 2 + 1;
    g.M = (int64_t)B * g.Ho * g.Wo;
    g.chunks = (g.M + STEM_PX - 1) / STEM_PX;
    g.chunks_per_slab = (g.chunks + STEM_SLABS - 1) / STEM_SLABS;
    if (g.chunks_per_slab < 1) g.chunks_per_slab = 1;
    g.slabs = (g.chunks + g.chunks_per_slab - 1) / g.chunks_per_slab;
    return g;
}

}  // namespace dmm

extern "C" int dmm_conv7x7s2_stem_bf16(const void *x, const void *w, const void *bias, int B, int H, int W, void *y,
                                       dmm_stream_t stream) {
    if (!dmm::stem_sizes_ok(B, H, W)) return DMM_ERR_BAD_ARG;
    if (B == 0) return DMM_OK;
    if (!x || !w || !y) return DMM_ERR_BAD_ARG;
    if (((uintptr_t)x & 1) || ((uintptr_t)w & 15) || ((uintptr_t)y & 15) || ((uintptr_t)bias & 1)) return DMM_ERR_BAD_ARG;
    const dmm::StemGeom g = dmm::stem_geom(B, H, W);
    const int64_t per_wg = (g.chunks + dmm::STEM_FWD_WGS - 1) / dmm::STEM_FWD_WGS;         // (chunks >= 1: B, H, W > 0)
    const int64_t groups = (g.chunks + per_wg - 1) / per_wg;
    hipLaunchKernelGGL(dmm::stem_conv_kernel, dim3((unsigned)groups), dim3(256), 0, (hipStream_t)stream, (const uint16_t *)x,
                       (const uint16_t *)w, (const uint16_t *)bias, (uint16_t *)y, H, W, g.Ho, g.Wo, g.M, g.chunks, per_wg);
    return dmm::check_launch();
}

extern "C" size_t dmm_wgrad7x7s2_stem_workspace_bytes(int B, int H, int W) {
    if (B <= 0 || !dmm::stem_sizes_ok(B, H, W)) return 0;
    const dmm::StemGeom g = dmm::stem_geom(B, H, W);
    return sizeof(float) * (size_t)(g.slabs * dmm::STEM_CO * dmm::STEM_CV);
}

extern "C" int dmm_wgrad7x7s2_stem_bf16(const void *dy, const void *x, int B, int H, int W, float *dw, void *workspace,
                                        size_t workspace_bytes, dmm_stream_t stream) {
    if (!dmm::stem_sizes_ok(B, H, W)) return DMM_ERR_BAD_ARG;
    if (!dw || ((uintptr_t)dw & 3)) return DMM_ERR_BAD_ARG;
    hipStream_t s = (hipStream_t)stream;
    if (B == 0) {
        DMM_HIP_TRY(dmm::zero_async(dw, sizeof(float) * (size_t)dmm::STEM_CO * dmm::STEM_CV, s));
        return DMM_OK;
    }
    if (!dy || !x || ((uintptr_t)dy & 15) || ((uintptr_t)x & 1)) return DMM_ERR_BAD_ARG;
    const dmm::StemGeom g = dmm::stem_geom(B, H, W);
    if (!workspace || workspace_bytes < sizeof(float) * (size_t)(g.slabs * dmm::STEM_CO * dmm::STEM_CV)) return DMM_ERR_WORKSPACE;
    if ((uintptr_t)workspace & 3) return DMM_ERR_BAD_ARG;                                       // (fp32 partial tables)
    hipLaunchKernelGGL(dmm::stem_wgrad_kernel, dim3((unsigned)g.slabs), dim3(256), 0, s, (const uint16_t *)dy,
                       (const uint16_t *)x, (float *)workspace, H, W, g.Ho, g.Wo, g.M, g.chunks, g.chunks_per_slab);
    int rc = dmm::check_launch();
    if (rc != DMM_OK) return rc;
    hipLaunchKernelGGL(dmm::stem_wgrad_fold_kernel, dim3(dmm::STEM_CV), dim3(256), 0, s, (const float *)workspace, (int)g.slabs,
                       dw);
    return dmm::check_launch();
}
