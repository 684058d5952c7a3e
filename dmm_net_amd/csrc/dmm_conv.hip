// dmm_conv.hip -- 3x3 / padding 1 convolution (stride 1 or 2) of the encoder on gfx950 for the DETERMINISTIC mode: bf16
// channels-last in, bf16 out, implicit GEMM on v_mfma_f32_32x32x16_bf16, fp32 accumulation, the bias added in fp32, ONE rounding.
//
// Reference: the forward of conv2 of a bottleneck and of the 3x3 head convolutions (dmm/modules/vision.py:6-38, base.py:35-54)
// under cudnn.deterministic (train.py:46).  With that flag MIOpen runs its naive reference kernel for every bf16 NHWC 3x3
// convolution on gfx950 (profiles/r07_deterministic_cost.md: 808 ms per config-4 step against 12.5).  The data gradient of such a
// convolution is the same problem on dy with the flipped, transposed weight (dmm_wprep3x3_bf16 writes it), so this one kernel
// serves both directions.
//
// Product.  y[m, co] = sum_k w[co, k] * patch[m, k]:  m = (b, ho, wo) the output pixel, k = (kh, kw, ci) -- both operands have
// the reduction index fastest in memory (x is [B, H, W, ci], the channels-last weight [co, kh, kw, ci]), which is what an MFMA
// fragment wants: 8 consecutive k per lane, one 16-byte LDS read, no transposes.  The weight is the A operand and the pixels
// the B operand: a lane of the result then holds 4 consecutive output channels of ONE pixel per register group, which pack into
// 8-byte pieces of y's rows.
//
// Workgroup = 4 waves = a tile of TCO (128, or 64 where 128 does not divide co) output channels x 128 output pixels; a wave
// owns 64 channels x 64 (32) pixels = 2 x 2 (2 x 1) MFMA tiles.  K is walked tap by tap in stages of 64 input channels: a
// stage is TCO + 128 rows of 128 bytes in LDS, fetched in 16-byte pieces one stage ahead into registers, two LDS buffers, one
// barrier per stage.  The pixels of a tile stay the same for the whole K walk, so each thread computes the (image, row,
// column) of its four pixel rows ONCE; a stage only adds the tap's offset.  The fetch is branch-free: a piece outside the image
// (or beyond the last pixel, or of the stage after the last) is loaded from a valid address and zeroed on its way to LDS --
// never a neighbouring row's or image's pixel.  LDS rows are XOR-swizzled by (row >> 1) & 7 in units of 16 bytes: the
// fragment reads (32 rows x 2 pieces per instruction) and the piece stores are both conflict free.
//
// Determinism.  No atomics.  K is cut into `splits` contiguous runs of stages where the pixel tiles alone cannot fill the chip
// (layer4 at 12 x 255 x 448: 44 tiles); split s stores its fp32 partial tile with plain stores into slab s of the caller's
// workspace, and a second launch sums the slabs in the order s = 0, 1, ..., adds the bias and rounds.  The number of splits is
// a function of (H, W, ci, co, stride) -- NOT of the batch -- so an image's result does not depend on the batch it sits in.
//
// conv3x3_narrow_kernel (further down, with its own header) is the same product for widths that are multiples of 32 only, at
// stride 1 and without a split: the 32-channel level-2 heads (dmm_conv3x3_narrow_bf16, include/dmm_match.h (10e)).
#include "dmm_common.h"

namespace dmm {

typedef __bf16 bf16x8c __attribute__((ext_vector_type(8)));
typedef float f32x16c __attribute__((ext_vector_type(16)));
typedef float f32x4c __attribute__((ext_vector_type(4)));
typedef uint32_t u32x4c __attribute__((ext_vector_type(4)));
typedef uint32_t u32x2c __attribute__((ext_vector_type(2)));

constexpr int CONV_PX = 128;             // output pixels per workgroup
constexpr int CONV_BK = 64;              // input channels per stage (one tap)

struct ConvGeom {
    int H, W, Ho, Wo, stride, Ci, Co;
    int64_t M;                           // B * Ho * Wo
    int stages;                          // 9 * Ci / 64
    int per_split;                       // stages per split (the last split may run short)
};

__device__ __forceinline__ uint32_t conv_bf16_rne(float v) {
    const uint32_t u = __float_as_uint(v);
    if ((u & 0x7fffffffu) > 0x7f800000u) return (u >> 16) | 0x40u;
    return (u + 0x7fffu + ((u >> 16) & 1u)) >> 16;
}

// element offset of 16-byte piece p (0..7) of row r in a [rows][64] bf16 LDS image
__device__ __forceinline__ int conv_lds_at(int r, int p) { return r * CONV_BK + ((p ^ ((r >> 1) & 7)) << 3); }

// SPLIT = false: y = bf16(acc + bias), through LDS in 16-byte pieces.  SPLIT = true: blockIdx.z = the split; the fp32 tile goes
// to part + split * M * Co ([M][Co]).
template <int TCO, bool SPLIT>
__global__ __launch_bounds__(256) void conv3x3_mfma_kernel(const uint16_t *__restrict__ x, const uint16_t *__restrict__ w,
                                                           const uint16_t *__restrict__ bias, uint16_t *__restrict__ y,
                                                           float *__restrict__ part, ConvGeom g) {
    constexpr int NJ = TCO / 64;                         // pixel MFMA tiles per wave: 64 channels x 32 * NJ pixels
    constexpr int WCO = TCO / 64;                        // waves along the channels; 4 / WCO along the pixels
    constexpr int NA = TCO / 32;                         // weight pieces per thread and stage (pixel pieces: 4)
    constexpr int STAGE = (TCO + CONV_PX) * CONV_BK;     // ushorts of one buffer: weight rows, then pixel rows
    constexpr int OUT_LD = TCO + 8;                      // row of the output image in LDS (ushorts): + 16 bytes against conflicts
    static_assert(2 * STAGE >= CONV_PX * OUT_LD, "the output image reuses the operand buffers");
    __shared__ __attribute__((aligned(16))) uint16_t lds_[2 * STAGE];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int r = lane & 31, h = lane >> 5;
    const int wco = wave % WCO, wpx = wave / WCO;
    const int64_t m0 = (int64_t)blockIdx.x * CONV_PX;
    const int co0 = blockIdx.y * TCO;
    const int ks0 = SPLIT ? (int)blockIdx.z * g.per_split : 0;
    int ks1 = SPLIT ? ks0 + g.per_split : g.stages;
    if (ks1 > g.stages) ks1 = g.stages;
    const int nc = g.Ci / CONV_BK;                       // stages per tap

    // this thread's pieces of a stage: column pc (8 channels), rows pr + 32 q of the weight tile and of the pixel tile
    const int pc = t & 7, pr = t >> 3;
    int64_t pix_base[4];                                 // element offset of pixel (b, s * ho, s * wo), channel 0
    int hs[4], ws[4];                                    // s * ho, s * wo; a row beyond M: far outside the image
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int64_t m = m0 + pr + 32 * q;
        const bool in = m < g.M;
        const int64_t mm = in ? m : 0;
        const int64_t qd = mm / g.Wo;
        const int wo = (int)(mm - qd * g.Wo);
        const int b = (int)(qd / g.Ho);
        const int ho = (int)(qd - (int64_t)b * g.Ho);
        hs[q] = in ? ho * g.stride : -(1 << 20);
        ws[q] = wo * g.stride;
        pix_base[q] = (((int64_t)b * g.H + ho * g.stride) * g.W + wo * g.stride) * g.Ci;
    }
    int64_t a_off[NA];                                   // weight row co0 + pr + 32 q: stage ks begins at element 64 * ks of the row
#pragma unroll
    for (int q = 0; q < NA; ++q) a_off[q] = (int64_t)(co0 + pr + 32 * q) * 9 * g.Ci + 8 * pc + (int64_t)CONV_BK * ks0;
    // the tap and channel block of the stage to fetch next: advanced by additions and two carries
    int tap = ks0 / nc, cc = ks0 - tap * nc;
    int kh = tap / 3, kw = tap - 3 * kh;
    int ks_f = ks0;

    u32x4c ra[NA], rb[4];
    uint32_t okm = 0;                                    // bit q: pixel piece q inside the image; bit 4: the stage exists
    auto fetch = [&]() {
        const bool live = ks_f < ks1;
        okm = live ? 16u : 0u;
#pragma unroll
        for (int q = 0; q < NA; ++q) {
            ra[q] = *reinterpret_cast<const u32x4c *>(w + (live ? a_off[q] : (int64_t)(8 * pc)));
            a_off[q] += CONV_BK;
        }
        const int dh = kh - 1, dw = kw - 1;
        const int64_t tap_off = ((int64_t)dh * g.W + dw) * g.Ci + cc * CONV_BK + 8 * pc;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int hi = hs[q] + dh, wi = ws[q] + dw;
            const bool in = live && hi >= 0 && hi < g.H && wi >= 0 && wi < g.W;
            rb[q] = *reinterpret_cast<const u32x4c *>(x + (in ? pix_base[q] + tap_off : (int64_t)(8 * pc)));
            okm |= in ? (1u << q) : 0u;
        }
        ++ks_f;
        const int c1 = ++cc == nc;
        cc = c1 ? 0 : cc;
        kw += c1;
        const int c2 = kw == 3;
        kw = c2 ? 0 : kw;
        kh += c2;
    };
    auto stash = [&](int buf) {
        const u32x4c z = {0u, 0u, 0u, 0u};
        uint16_t *sa = lds_ + buf * STAGE, *sb = sa + TCO * CONV_BK;
        const bool live = (okm & 16u) != 0u;
#pragma unroll
        for (int q = 0; q < NA; ++q) *reinterpret_cast<u32x4c *>(sa + conv_lds_at(pr + 32 * q, pc)) = live ? ra[q] : z;
#pragma unroll
        for (int q = 0; q < 4; ++q) *reinterpret_cast<u32x4c *>(sb + conv_lds_at(pr + 32 * q, pc)) = (okm >> q) & 1u ? rb[q] : z;
    };

    f32x16c acc[2][NJ];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < NJ; ++j)
#pragma unroll
            for (int k = 0; k < 16; ++k) acc[i][j][k] = 0.0f;

    // stage: registers -> LDS buffer, the registers refilled one stage ahead, ONE barrier, multiply.  (The buffer the next
    // stage overwrites was read by the stage before this one; this stage's barrier lies between.)
    fetch();
    int buf = 0;
    for (int ks = ks0; ks < ks1; ++ks) {
        stash(buf);
        fetch();
        __syncthreads();
        const uint16_t *sa = lds_ + buf * STAGE, *sb = sa + TCO * CONV_BK;
#pragma unroll
        for (int kk = 0; kk < CONV_BK / 16; ++kk) {
            bf16x8c fa[2], fb[NJ];
#pragma unroll
            for (int i = 0; i < 2; ++i)
                fa[i] = *reinterpret_cast<const bf16x8c *>(sa + conv_lds_at(wco * 64 + i * 32 + r, 2 * kk + h));
#pragma unroll
            for (int j = 0; j < NJ; ++j)
                fb[j] = *reinterpret_cast<const bf16x8c *>(sb + conv_lds_at(wpx * (32 * NJ) + j * 32 + r, 2 * kk + h));
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < NJ; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[i], fb[j], acc[i][j], 0, 0, 0);
        }
        buf ^= 1;
    }

    // D layout: column (the pixel side) = lane & 31, row (the channel side) = (reg & 3) + 8 * (reg >> 2) + 4 * (lane >> 5)
    if (SPLIT) {
        float *o = part + (int64_t)blockIdx.z * g.M * g.Co;
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
            const int64_t m = m0 + wpx * (32 * NJ) + j * 32 + r;
            if (m < g.M) {
#pragma unroll
                for (int i = 0; i < 2; ++i)
#pragma unroll
                    for (int g4 = 0; g4 < 4; ++g4) {
                        const int c = co0 + wco * 64 + i * 32 + 8 * g4 + 4 * h;
                        const f32x4c v = {acc[i][j][4 * g4], acc[i][j][4 * g4 + 1], acc[i][j][4 * g4 + 2], acc[i][j][4 * g4 + 3]};
                        *reinterpret_cast<f32x4c *>(o + m * g.Co + c) = v;
                    }
            }
        }
        return;
    }
    __syncthreads();                                     // (the last stage's fragment reads are done: the buffers become the image)
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int g4 = 0; g4 < 4; ++g4) {
            const int cl = wco * 64 + i * 32 + 8 * g4 + 4 * h;
            float bv[4] = {0.0f, 0.0f, 0.0f, 0.0f};
            if (bias) {
                const u32x2c bb = *reinterpret_cast<const u32x2c *>(bias + co0 + cl);
                bv[0] = __uint_as_float(bb[0] << 16);
                bv[1] = __uint_as_float(bb[0] & 0xFFFF0000u);
                bv[2] = __uint_as_float(bb[1] << 16);
                bv[3] = __uint_as_float(bb[1] & 0xFFFF0000u);
            }
#pragma unroll
            for (int j = 0; j < NJ; ++j) {
                const int pl = wpx * (32 * NJ) + j * 32 + r;
                u32x2c o;
                o[0] = conv_bf16_rne(acc[i][j][4 * g4] + bv[0]) | (conv_bf16_rne(acc[i][j][4 * g4 + 1] + bv[1]) << 16);
                o[1] = conv_bf16_rne(acc[i][j][4 * g4 + 2] + bv[2]) | (conv_bf16_rne(acc[i][j][4 * g4 + 3] + bv[3]) << 16);
                *reinterpret_cast<u32x2c *>(lds_ + pl * OUT_LD + cl) = o;
            }
        }
    __syncthreads();
    constexpr int PR = TCO / 8;                          // 16-byte pieces per output row
#pragma unroll
    for (int n = 0; n < CONV_PX * PR / 256; ++n) {
        const int idx = t + 256 * n, pl = idx / PR, p8 = idx % PR;
        const int64_t m = m0 + pl;
        if (m < g.M)
            *reinterpret_cast<u32x4c *>(y + m * g.Co + co0 + 8 * p8) = *reinterpret_cast<const u32x4c *>(lds_ + pl * OUT_LD + 8 * p8);
    }
}

// y[m, c] = bf16(bias[c] + sum_s part[s][m][c]), s = 0, 1, ... in order; a thread owns 8 consecutive channels of a pixel
__global__ __launch_bounds__(256) void conv3x3_fold_kernel(const float *__restrict__ part, int splits, int64_t n,
                                                           const uint16_t *__restrict__ bias, int Co, uint16_t *__restrict__ y) {
    const int64_t e = ((int64_t)blockIdx.x * 256 + threadIdx.x) * 8;
    if (e >= n) return;
    float acc[8];
    {
        const f32x4c a = *reinterpret_cast<const f32x4c *>(part + e), b = *reinterpret_cast<const f32x4c *>(part + e + 4);
#pragma unroll
        for (int k = 0; k < 4; ++k) { acc[k] = a[k]; acc[4 + k] = b[k]; }
    }
    for (int s = 1; s < splits; ++s) {
        const float *p = part + (int64_t)s * n + e;
        const f32x4c a = *reinterpret_cast<const f32x4c *>(p), b = *reinterpret_cast<const f32x4c *>(p + 4);
#pragma unroll
        for (int k = 0; k < 4; ++k) { acc[k] += a[k]; acc[4 + k] += b[k]; }
    }
    if (bias) {
        const u32x4c bb = *reinterpret_cast<const u32x4c *>(bias + (int)(e % Co));
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            acc[2 * k] += __uint_as_float(bb[k] << 16);
            acc[2 * k + 1] += __uint_as_float(bb[k] & 0xFFFF0000u);
        }
    }
    u32x4c o;
#pragma unroll
    for (int k = 0; k < 4; ++k) o[k] = conv_bf16_rne(acc[2 * k]) | (conv_bf16_rne(acc[2 * k + 1]) << 16);
    *reinterpret_cast<u32x4c *>(y + e) = o;
}

struct ConvPlan {
    int tco, splits, per_split, stages;
};

// The tile width and the K splits of a problem: from the image's geometry and the widths only, never from the batch (an image's
// bits must not depend on the batch it sits in).  A split runs at least 12 stages (768 of the 9 * ci reduction steps), and the
// splits stop where one image's tiles x splits reach 64 workgroups: layer4 at 255 x 448 (112 pixels, 512 channels: 4 tiles per
// image, 72 stages) takes 6, layer3 (8 tiles, 36 stages) 3, layer1 / layer2 one; a 2048 -> 128 head on 8 x 14 pixels 24.
static ConvPlan conv_plan(int H, int W, int ci, int co, int stride) {
    ConvPlan p;
    p.tco = (co & 127) ? 64 : 128;
    p.stages = 9 * (ci / CONV_BK);
    const int64_t px = (int64_t)((H - 1) / stride + 1) * ((W - 1) / stride + 1);
    const int64_t tiles_img = ((px + CONV_PX - 1) / CONV_PX) * (co / p.tco);
    int64_t s = p.stages / 12;
    const int64_t by_tiles = 64 / tiles_img;
    if (s > by_tiles) s = by_tiles;
    if (s > 64) s = 64;
    if (s < 1) s = 1;
    p.per_split = (int)((p.stages + s - 1) / s);
    p.splits = (p.stages + p.per_split - 1) / p.per_split;
    return p;
}


// ---- the NARROW form: widths that are multiples of 32 (the 32-channel level-2 heads), stride 1 ------------------------------
// Same product, same tile of 128 pixels, same 64-channel stage of 128-byte LDS rows with the same XOR swizzle -- so the
// conflict argument of the header holds unchanged: a ds_read_b128 is served in groups of 16 lanes (rows {0-3, 12-15, 20-27} or
// {4-11, 16-19, 28-31} of a fragment, one piece column), whose (row & 1) * 8 + (piece ^ ((row >> 1) & 7)) are 16 different
// 16-byte columns of the 256-byte bank line; a ds_write_b128 in groups of 8 consecutive lanes = the 8 pieces of ONE row, a
// permutation of the 8 columns of its 128 bytes.
//
// What differs.  (1) TCO = 32 exists: all four waves lie along the pixels, a wave owns ONE 32 x 32 MFMA tile, a thread fetches
// one weight piece per stage.  (2) A tap holds ci / 32 HALF stages of 32 channels, which may be an odd number, so each half of
// the 64-channel stage has its own (tap, channel block): half stage n = 2 * stage + half is tap n / (ci / 32), block
// n % (ci / 32).  A thread's piece column fixes its half (pc >> 2), so it walks its own (kh, kw, block) by two half stages per
// stage -- additions and carries, no branch.  The weight row [kh, kw, ci] is contiguous over ALL half stages: stage ks still
// begins at element 64 * ks of the row.  When 9 * ci / 32 is odd the last stage's second half does not exist: its pieces are
// loaded from a valid address (the tensor's first 64 bytes) and reach LDS as zeros, like a pixel outside the image.
// No split of the reduction: the narrow shapes sit on the stride-4 / stride-8 levels, where the pixel tiles fill the chip.  The
// summation order of an output element is a function of (ci, co) alone.
template <int TCO>
__global__ __launch_bounds__(256) void conv3x3_narrow_kernel(const uint16_t *__restrict__ x, const uint16_t *__restrict__ w,
                                                             const uint16_t *__restrict__ bias, uint16_t *__restrict__ y,
                                                             int H, int W, int Ci, int Co, int64_t M) {
    constexpr int NI = TCO >= 64 ? 2 : 1;                // channel MFMA tiles per wave
    constexpr int WCO = TCO / (32 * NI);                 // waves along the channels; 4 / WCO along the pixels
    constexpr int NJ = WCO;                              // pixel MFMA tiles per wave: 128 / (4 / WCO) / 32
    constexpr int NA = TCO / 32;                         // weight pieces per thread and stage (pixel pieces: 4)
    constexpr int STAGE = (TCO + CONV_PX) * CONV_BK;
    constexpr int OUT_LD = TCO + 8;
    static_assert(2 * STAGE >= CONV_PX * OUT_LD, "the output image reuses the operand buffers");
    __shared__ __attribute__((aligned(16))) uint16_t lds_[2 * STAGE];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int r = lane & 31, h = lane >> 5;
    const int wco = wave % WCO, wpx = wave / WCO;
    const int64_t m0 = (int64_t)blockIdx.x * CONV_PX;
    const int co0 = blockIdx.y * TCO;
    const int nc = Ci / 32;                              // half stages per tap
    const int halves = 9 * nc;
    const int stages = (halves + 1) / 2;

    const int pc = t & 7, pr = t >> 3;
    const int half = pc >> 2, c8 = 8 * (pc & 3);         // this thread's half of a stage, its channels inside the half
    int64_t pix_base[4];
    int hs[4], ws[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int64_t m = m0 + pr + 32 * q;
        const bool in = m < M;
        const int64_t mm = in ? m : 0;
        const int64_t qd = mm / W;
        const int wo = (int)(mm - qd * W);
        const int b = (int)(qd / H);
        const int ho = (int)(qd - (int64_t)b * H);
        hs[q] = in ? ho : -(1 << 20);
        ws[q] = wo;
        pix_base[q] = (((int64_t)b * H + ho) * W + wo) * Ci;
    }
    int64_t a_off[NA];
#pragma unroll
    for (int q = 0; q < NA; ++q) a_off[q] = (int64_t)(co0 + pr + 32 * q) * 9 * Ci + 8 * pc;
    int hn = half;                                       // the half stage to fetch next, its tap and channel block
    int tap = half / nc, cc = half - tap * nc;           // (nc == 1: the second half begins at tap 1)
    int kh = 0, kw = tap;

    u32x4c ra[NA], rb[4];
    uint32_t okm = 0;                                    // bit q: pixel piece q inside the image; bit 4: the half stage exists
    auto fetch = [&]() {
        const bool live = hn < halves;
        okm = live ? 16u : 0u;
#pragma unroll
        for (int q = 0; q < NA; ++q) {
            ra[q] = *reinterpret_cast<const u32x4c *>(w + (live ? a_off[q] : (int64_t)(8 * pc)));
            a_off[q] += CONV_BK;
        }
        const int dh = kh - 1, dw = kw - 1;
        const int64_t tap_off = ((int64_t)dh * W + dw) * Ci + cc * 32 + c8;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int hi = hs[q] + dh, wi = ws[q] + dw;
            const bool in = live && hi >= 0 && hi < H && wi >= 0 && wi < W;
            rb[q] = *reinterpret_cast<const u32x4c *>(x + (in ? pix_base[q] + tap_off : (int64_t)c8));
            okm |= in ? (1u << q) : 0u;
        }
        hn += 2;
#pragma unroll
        for (int s = 0; s < 2; ++s) {                    // two half stages on
            const int c1 = ++cc == nc;
            cc = c1 ? 0 : cc;
            kw += c1;
            const int c2 = kw == 3;
            kw = c2 ? 0 : kw;
            kh += c2;
        }
    };
    auto stash = [&](int buf) {
        const u32x4c z = {0u, 0u, 0u, 0u};
        uint16_t *sa = lds_ + buf * STAGE, *sb = sa + TCO * CONV_BK;
        const bool live = (okm & 16u) != 0u;
#pragma unroll
        for (int q = 0; q < NA; ++q) *reinterpret_cast<u32x4c *>(sa + conv_lds_at(pr + 32 * q, pc)) = live ? ra[q] : z;
#pragma unroll
        for (int q = 0; q < 4; ++q) *reinterpret_cast<u32x4c *>(sb + conv_lds_at(pr + 32 * q, pc)) = (okm >> q) & 1u ? rb[q] : z;
    };

    f32x16c acc[NI][NJ];
#pragma unroll
    for (int i = 0; i < NI; ++i)
#pragma unroll
        for (int j = 0; j < NJ; ++j)
#pragma unroll
            for (int k = 0; k < 16; ++k) acc[i][j][k] = 0.0f;

    fetch();
    int buf = 0;
    for (int ks = 0; ks < stages; ++ks) {
        stash(buf);
        fetch();
        __syncthreads();
        const uint16_t *sa = lds_ + buf * STAGE, *sb = sa + TCO * CONV_BK;
#pragma unroll
        for (int kk = 0; kk < CONV_BK / 16; ++kk) {
            bf16x8c fa[NI], fb[NJ];
#pragma unroll
            for (int i = 0; i < NI; ++i)
                fa[i] = *reinterpret_cast<const bf16x8c *>(sa + conv_lds_at(wco * (32 * NI) + i * 32 + r, 2 * kk + h));
#pragma unroll
            for (int j = 0; j < NJ; ++j)
                fb[j] = *reinterpret_cast<const bf16x8c *>(sb + conv_lds_at(wpx * (32 * NJ) + j * 32 + r, 2 * kk + h));
#pragma unroll
            for (int i = 0; i < NI; ++i)
#pragma unroll
                for (int j = 0; j < NJ; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[i], fb[j], acc[i][j], 0, 0, 0);
        }
        buf ^= 1;
    }

    // D layout: column (the pixel side) = lane & 31, row (the channel side) = (reg & 3) + 8 * (reg >> 2) + 4 * (lane >> 5)
    __syncthreads();                                     // (the last stage's fragment reads are done: the buffers become the image)
#pragma unroll
    for (int i = 0; i < NI; ++i)
#pragma unroll
        for (int g4 = 0; g4 < 4; ++g4) {
            const int cl = wco * (32 * NI) + i * 32 + 8 * g4 + 4 * h;
            float bv[4] = {0.0f, 0.0f, 0.0f, 0.0f};
            if (bias) {
                const u32x2c bb = *reinterpret_cast<const u32x2c *>(bias + co0 + cl);
                bv[0] = __uint_as_float(bb[0] << 16);
                bv[1] = __uint_as_float(bb[0] & 0xFFFF0000u);
                bv[2] = __uint_as_float(bb[1] << 16);
                bv[3] = __uint_as_float(bb[1] & 0xFFFF0000u);
            }
#pragma unroll
            for (int j = 0; j < NJ; ++j) {
                const int pl = wpx * (32 * NJ) + j * 32 + r;
                u32x2c o;
                o[0] = conv_bf16_rne(acc[i][j][4 * g4] + bv[0]) | (conv_bf16_rne(acc[i][j][4 * g4 + 1] + bv[1]) << 16);
                o[1] = conv_bf16_rne(acc[i][j][4 * g4 + 2] + bv[2]) | (conv_bf16_rne(acc[i][j][4 * g4 + 3] + bv[3]) << 16);
                *reinterpret_cast<u32x2c *>(lds_ + pl * OUT_LD + cl) = o;
            }
        }
    __syncthreads();
    constexpr int PR = TCO / 8;                          // 16-byte pieces per output row
#pragma unroll
    for (int n = 0; n < CONV_PX * PR / 256; ++n) {
        const int idx = t + 256 * n, pl = idx / PR, p8 = idx % PR;
        const int64_t m = m0 + pl;
        if (m < M)
            *reinterpret_cast<u32x4c *>(y + m * Co + co0 + 8 * p8) = *reinterpret_cast<const u32x4c *>(lds_ + pl * OUT_LD + 8 * p8);
    }
}

}  // namespace dmm

extern "C" size_t dmm_conv3x3_workspace_bytes(int B, int H, int W, int ci, int co, int stride) {
    if (B <= 0 || H <= 0 || W <= 0 || ci <= 0 || co <= 0 || (ci & 63) || (co & 63) || (stride != 1 && stride != 2)) return 0;
    const dmm::ConvPlan p = dmm::conv_plan(H, W, ci, co, stride);
    if (p.splits == 1) return 0;
    const int64_t M = (int64_t)B * ((H - 1) / stride + 1) * ((W - 1) / stride + 1);
    return sizeof(float) * (size_t)p.splits * (size_t)M * (size_t)co;          // (co % 64 == 0: a multiple of 256 bytes)
}

extern "C" int dmm_conv3x3_bf16(const void *x, const void *w, const void *bias, int B, int H, int W, int ci, int co, int stride,
                                void *y, void *workspace, size_t workspace_bytes, dmm_stream_t stream) {
    if (B < 0 || H <= 0 || W <= 0 || ci <= 0 || co <= 0 || (stride != 1 && stride != 2)) return DMM_ERR_BAD_ARG;
    if ((ci & 63) || (co & 63)) return DMM_ERR_BAD_ARG;
    if (B == 0) return DMM_OK;
    if (!x || !w || !y) return DMM_ERR_BAD_ARG;
    if (((uintptr_t)x & 15) || ((uintptr_t)w & 15) || ((uintptr_t)y & 15) || ((uintptr_t)bias & 15) || ((uintptr_t)workspace & 15))
        return DMM_ERR_BAD_ARG;                            // 16-byte pieces
    const dmm::ConvPlan p = dmm::conv_plan(H, W, ci, co, stride);
    dmm::ConvGeom g;
    g.H = H; g.W = W; g.stride = stride; g.Ci = ci; g.Co = co;
    g.Ho = (H - 1) / stride + 1;
    g.Wo = (W - 1) / stride + 1;
    g.M = (int64_t)B * g.Ho * g.Wo;
    g.stages = p.stages;
    g.per_split = p.per_split;
    const int64_t tiles = (g.M + dmm::CONV_PX - 1) / dmm::CONV_PX;
    if (tiles > 0x7fffffffLL) return DMM_ERR_BAD_ARG;
    const bool split = p.splits > 1;
    if (split && (!workspace || workspace_bytes < sizeof(float) * (size_t)p.splits * (size_t)g.M * (size_t)co)) return DMM_ERR_BAD_ARG;
    const dim3 grid((unsigned)tiles, (unsigned)(co / p.tco), (unsigned)p.splits);
    const uint16_t *xp = (const uint16_t *)x, *wp = (const uint16_t *)w, *bp = (const uint16_t *)bias;
    hipStream_t s = (hipStream_t)stream;
    if (p.tco == 128 && split)
        hipLaunchKernelGGL((dmm::conv3x3_mfma_kernel<128, true>), grid, dim3(256), 0, s, xp, wp, bp, (uint16_t *)y, (float *)workspace, g);
    else if (p.tco == 128)
        hipLaunchKernelGGL((dmm::conv3x3_mfma_kernel<128, false>), grid, dim3(256), 0, s, xp, wp, bp, (uint16_t *)y, (float *)nullptr, g);
    else if (split)
        hipLaunchKernelGGL((dmm::conv3x3_mfma_kernel<64, true>), grid, dim3(256), 0, s, xp, wp, bp, (uint16_t *)y, (float *)workspace, g);
    else
        hipLaunchKernelGGL((dmm::conv3x3_mfma_kernel<64, false>), grid, dim3(256), 0, s, xp, wp, bp, (uint16_t *)y, (float *)nullptr, g);
    int rc = dmm::check_launch();
    if (rc != DMM_OK || !split) return rc;
    const int64_t n = g.M * co;
    hipLaunchKernelGGL(dmm::conv3x3_fold_kernel, dim3((unsigned)((n / 8 + 255) / 256)), dim3(256), 0, s, (const float *)workspace,
                       p.splits, n, bp, co, (uint16_t *)y);
    return dmm::check_launch();
}

extern "C" int dmm_conv3x3_narrow_bf16(const void *x, const void *w, const void *bias, int B, int H, int W, int ci, int co,
                                       void *y, dmm_stream_t stream) {
    if (B < 0 || H <= 0 || W <= 0 || ci <= 0 || co <= 0) return DMM_ERR_BAD_ARG;
    if ((ci & 31) || (co & 31)) return DMM_ERR_BAD_ARG;
    if (B == 0) return DMM_OK;
    if (!x || !w || !y) return DMM_ERR_BAD_ARG;
    if (((uintptr_t)x & 15) || ((uintptr_t)w & 15) || ((uintptr_t)y & 15) || ((uintptr_t)bias & 15)) return DMM_ERR_BAD_ARG;
    const int64_t M = (int64_t)B * H * W;
    const int64_t tiles = (M + dmm::CONV_PX - 1) / dmm::CONV_PX;
    if (tiles > 0x7fffffffLL) return DMM_ERR_BAD_ARG;
    // the channel tile: from co alone (with ci it fixes an element's summation order)
    const int tco = (co & 127) == 0 ? 128 : (co & 63) == 0 ? 64 : 32;
    const dim3 grid((unsigned)tiles, (unsigned)(co / tco));
    const uint16_t *xp = (const uint16_t *)x, *wp = (const uint16_t *)w, *bp = (const uint16_t *)bias;
    hipStream_t s = (hipStream_t)stream;
    if (tco == 128)
        hipLaunchKernelGGL((dmm::conv3x3_narrow_kernel<128>), grid, dim3(256), 0, s, xp, wp, bp, (uint16_t *)y, H, W, ci, co, M);
    else if (tco == 64)
        hipLaunchKernelGGL((dmm::conv3x3_narrow_kernel<64>), grid, dim3(256), 0, s, xp, wp, bp, (uint16_t *)y, H, W, ci, co, M);
    else
        hipLaunchKernelGGL((dmm::conv3x3_narrow_kernel<32>), grid, dim3(256), 0, s, xp, wp, bp, (uint16_t *)y, H, W, ci, co, M);
    return dmm::check_launch();
}
