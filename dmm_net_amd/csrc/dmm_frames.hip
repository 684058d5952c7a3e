// dmm_frames.hip -- (16) frames as the encoders take them, from decoded images: PIL's 8-bit resize (bilinear / bicubic through
// the caller's fixed-point coefficient tables, nearest through the index tables of (14b)), then ToTensor + Normalize as a
// 3 x 256 look-up.  Replaces Image.resize + transforms.ToTensor + transforms.Normalize of dmm/dataloader/dataset.py:202-219.
//   hpass    one workgroup = a tile of output columns (a multiple of 16, one per thread) of up to four source rows of one frame.
//            The span of each row the tile's taps read is pulled into LDS with 16-byte loads (the bytes before the first and
//            after the last aligned chunk one by one: nothing outside the row is read) and the tile's coefficient rows with
//            coalesced loads (a lane's row then starts ksize words after its neighbour's: ksize is odd, no bank is hit twice).
//            Every lane forms the three channel sums of its column for all the rows from LDS, four taps -- twelve consecutive
//            bytes -- at a time: four aligned words per row, shifted to the lane's first byte, instead of twelve byte reads
//            (one byte per read and the coefficients from memory: 91 us for the config-4 clip set; this form:
//            profiles/r14_prepare_frames.md).  The interleaved uint8 results meet in LDS, from where the intermediate goes out
//            in 16-byte stores (its row pitch is 3 W rounded up to 16).  A column whose taps leave the staged window (only a
//            table that is not the rule's can ask for that) reads them from memory, byte by byte.
//   vpass    one workgroup = 256 pixels of one output row; lanes run along the row's BYTES, four per lane, so every tap row is
//            one coalesced read and the pass does not care which channel a byte is.  Without a table it is the copy of the
//            equal-size case.
//   nearest  one workgroup = 256 pixels of one output row, a 3-byte gather per lane.
//   emit     the end of whichever kernel runs last: the row piece, interleaved uint8 in LDS, goes out as it is (out_u8) and
//            through the look-up table (in LDS) into the three fp32 planes, 16 bytes per store where the address allows.
// Everything is integer arithmetic or a look-up: no rounding is made here, and the bytes are the same on every run.
#include "dmm_launchers.h"

namespace dmm {

constexpr int kFrThreads = 256;
constexpr int kFrRows = 4;                                 // source rows of a hpass workgroup (fewer when LDS is short)
constexpr int kFrTileBytes = 3 * kFrThreads;               // a vpass / nearest row piece: 256 pixels
constexpr int kFrLutBytes = 3 * 256 * 4;
constexpr int kFrLdsBudget = 48 * 1024;                    // dynamic LDS a hpass workgroup may ask for

struct FrameOut {
    const float *lut;
    float *f32;
    int64_t fs_out, ps_out;
    uint8_t *u8;
    int64_t fs_u8;
    int H, W;
};

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return min(max(v, lo), hi); }

__device__ __forceinline__ void frames_load_lut(const FrameOut &o, float *lut_s) {
    if (o.f32)
        for (int i = threadIdx.x; i < 3 * 256; i += kFrThreads) lut_s[i] = o.lut[i];
}

// S: 3 * npx interleaved bytes in LDS (16-byte aligned): pixels x0 .. x0 + npx of row y of frame f
__device__ __forceinline__ void frames_emit(const FrameOut &o, const float *lut_s, const uint8_t *S, int f, int y, int x0, int npx) {
    const int tid = threadIdx.x;
    if (o.u8) {
        uint8_t *d = o.u8 + f * o.fs_u8 + ((int64_t)y * o.W + x0) * 3;
        const int nb = 3 * npx;
        const int words = ((uintptr_t)d & 3) == 0 ? nb / 4 : 0;
        for (int i = tid; i < words; i += kFrThreads) reinterpret_cast<uint32_t *>(d)[i] = reinterpret_cast<const uint32_t *>(S)[i];
        for (int i = words * 4 + tid; i < nb; i += kFrThreads) d[i] = S[i];
    }
    if (o.f32) {
        const int groups = (npx + 3) / 4;
        for (int i = tid; i < 3 * groups; i += kFrThreads) {
            const int c = i / groups, x = (i - c * groups) * 4;
            float *p = o.f32 + f * o.fs_out + c * o.ps_out + (int64_t)y * o.W + x0 + x;
            const float *l = lut_s + c * 256;
            if (x + 4 <= npx && ((uintptr_t)p & 15) == 0) {
                *reinterpret_cast<float4 *>(p) = make_float4(l[S[3 * x + c]], l[S[3 * x + 3 + c]], l[S[3 * x + 6 + c]], l[S[3 * x + 9 + c]]);
            } else {
                for (int q = 0; q < 4 && x + q < npx; ++q) p[q] = l[S[3 * (x + q) + c]];
            }
        }
    }
}

__device__ __forceinline__ uint32_t clamp_shift(uint32_t acc) { return (uint32_t)clampi((int32_t)acc >> 22, 0, 255); }

// The tiling of the horizontal pass, decided on the host: tx output columns (a multiple of 16) x rows source rows per workgroup,
// cap_px source pixels of each row staged in LDS.
struct HTile {
    int tx, tiles_x, rows, cap_px, in_pitch, out_pitch, lut_bytes, coef_bytes;
    unsigned lds;
};

static HTile h_tile(int Ws, int W, int ksize, bool final_pass) {
    HTile t;
    const int tiles = (W + kFrThreads - 1) / kFrThreads;
    t.tx = (((W + tiles - 1) / tiles) + 15) / 16 * 16;
    t.rows = kFrRows;
    t.lut_bytes = final_pass ? kFrLutBytes : 0;
    for (;;) {
        // the taps of tx neighbouring columns lie within (tx - 1) * scale + 2 * support + 2 source pixels, and ksize >= 2 * support + 1
        const int64_t span = min((int64_t)Ws, ((int64_t)(t.tx - 1) * Ws + W - 1) / W + ksize + 2);
        t.out_pitch = 3 * t.tx;                            // (a multiple of 48)
        t.coef_bytes = t.tx * ksize * 4;                   // (a multiple of 16)
        // + 16: the row's own misalignment; + 16: the last group of four taps reads up to 15 bytes past the last tap
        const int64_t in_pitch = (3 * span + 15) / 16 * 16 + 32;
        const int64_t lds = t.lut_bytes + t.coef_bytes + (int64_t)t.rows * (in_pitch + t.out_pitch);
        if (lds <= kFrLdsBudget) {
            t.cap_px = (int)span;
            t.in_pitch = (int)in_pitch;
            break;
        }
        if (t.rows > 1) {
            t.rows /= 2;
        } else if (t.tx > 16) {
            t.tx = (t.tx / 2 + 15) / 16 * 16;
        } else {                                           // (tables that are not the rule's: the window is cut, the rest read from memory)
            t.in_pitch = (kFrLdsBudget - t.lut_bytes - t.coef_bytes - t.out_pitch) / 16 * 16;
            t.cap_px = (t.in_pitch - 32) / 3;
            break;
        }
    }
    t.tiles_x = (W + t.tx - 1) / t.tx;
    t.lds = (unsigned)(t.lut_bytes + t.coef_bytes + t.rows * (t.in_pitch + t.out_pitch));
    return t;
}

// grid: column tile fastest, then row group, then frame.  mid != null: the intermediate (row pitch mid_pitch); else the outputs.
__global__ __launch_bounds__(kFrThreads) void frames_hpass_kernel(const uint8_t *__restrict__ src, int64_t fs_src, int64_t rs_src,
                                                                  int Hs, int Ws, int W, const int32_t *__restrict__ bounds,
                                                                  const int32_t *__restrict__ coef, int ksize, HTile t,
                                                                  int row_groups, uint8_t *__restrict__ mid, int64_t mid_pitch,
                                                                  FrameOut o) {
    extern __shared__ uint4 frames_smem[];
    uint8_t *smem = reinterpret_cast<uint8_t *>(frames_smem);
    float *lut_s = reinterpret_cast<float *>(smem);
    int32_t *coef_s = reinterpret_cast<int32_t *>(smem + t.lut_bytes);
    uint8_t *in_s = smem + t.lut_bytes + t.coef_bytes;
    uint8_t *out_s = in_s + t.rows * t.in_pitch;
    unsigned g = blockIdx.x;
    const int tile = g % t.tiles_x; g /= t.tiles_x;
    const int rg = g % row_groups;
    const int f = g / row_groups;
    const int tid = threadIdx.x;
    const int x0 = tile * t.tx, npx = min(t.tx, W - x0);
    const int y0 = rg * t.rows, nrows = min(t.rows, Hs - y0);
    if (!mid) frames_load_lut(o, lut_s);
    {   // the tile's coefficient rows: npx * ksize consecutive words
        const int32_t *cg = coef + (int64_t)x0 * ksize;
        for (int i = tid; i < npx * ksize; i += kFrThreads) coef_s[i] = cg[i];
    }

    // the window of the source rows this tile's taps read: from the first column's first tap
    const int span_lo = clampi(bounds[2 * x0], 0, Ws);
    const int win_px = min(t.cap_px, Ws - span_lo);
    const uint8_t *grow[kFrRows];
    int a0[kFrRows];
#pragma unroll
    for (int r = 0; r < kFrRows; ++r) {
        grow[r] = src + f * fs_src + (int64_t)(y0 + min(r, nrows - 1)) * rs_src;
        const uint8_t *gp = grow[r] + 3 * span_lo;
        a0[r] = (int)((uintptr_t)gp & 15);
        if (r < nrows) {
            uint8_t *L = in_s + r * t.in_pitch + a0[r];     // byte i of the window at L[i]: aligned chunks stay aligned
            const int nbytes = 3 * win_px;
            const int head = min(nbytes, (16 - a0[r]) & 15);
            const int nvec = (nbytes - head) / 16;
            for (int i = tid; i < nvec; i += kFrThreads)
                *reinterpret_cast<uint4 *>(L + head + 16 * i) = *reinterpret_cast<const uint4 *>(gp + head + 16 * i);
            for (int i = tid; i < head; i += kFrThreads) L[i] = gp[i];
            for (int i = head + 16 * nvec + tid; i < nbytes; i += kFrThreads) L[i] = gp[i];
        }
    }
    for (int i = tid; i < t.rows * t.out_pitch / 16; i += kFrThreads) reinterpret_cast<uint4 *>(out_s)[i] = make_uint4(0, 0, 0, 0);
    __syncthreads();

    if (tid < npx) {
        const int x = x0 + tid;
        const int lo = clampi(bounds[2 * x], 0, Ws);
        const int cnt = clampi(bounds[2 * x + 1], 0, min(ksize, Ws - lo));
        const int32_t *cw = coef_s + tid * ksize;
        uint32_t acc[kFrRows][3];
#pragma unroll
        for (int r = 0; r < kFrRows; ++r) acc[r][0] = acc[r][1] = acc[r][2] = 1u << 21;
        if (lo >= span_lo && lo + cnt <= span_lo + win_px) {
            // four taps = twelve consecutive bytes of a row: the four aligned words that hold them, shifted to the first byte.
            // Bytes past the last tap meet a zero weight (they lie inside the row's LDS pitch).
            for (int k0 = 0; k0 < cnt; k0 += 4) {
                const uint32_t w0 = (uint32_t)cw[k0], w1 = k0 + 1 < cnt ? (uint32_t)cw[k0 + 1] : 0u,
                               w2 = k0 + 2 < cnt ? (uint32_t)cw[k0 + 2] : 0u, w3 = k0 + 3 < cnt ? (uint32_t)cw[k0 + 3] : 0u;
#pragma unroll
                for (int r = 0; r < kFrRows; ++r) {
                    if (r < nrows) {
                        const int b = a0[r] + 3 * (lo - span_lo + k0);
                        const uint32_t *q = reinterpret_cast<const uint32_t *>(in_s + r * t.in_pitch) + (b >> 2);
                        const int sh = 8 * (b & 3);
                        const uint32_t d0 = q[0], d1 = q[1], d2 = q[2], d3 = q[3];
                        const uint32_t v0 = (uint32_t)((((uint64_t)d1 << 32) | d0) >> sh), v1 = (uint32_t)((((uint64_t)d2 << 32) | d1) >> sh),
                                       v2 = (uint32_t)((((uint64_t)d3 << 32) | d2) >> sh);
                        acc[r][0] += w0 * (v0 & 255u) + w1 * (v0 >> 24) + w2 * ((v1 >> 16) & 255u) + w3 * ((v2 >> 8) & 255u);
                        acc[r][1] += w0 * ((v0 >> 8) & 255u) + w1 * (v1 & 255u) + w2 * (v1 >> 24) + w3 * ((v2 >> 16) & 255u);
                        acc[r][2] += w0 * ((v0 >> 16) & 255u) + w1 * ((v1 >> 8) & 255u) + w2 * (v2 & 255u) + w3 * (v2 >> 24);
                    }
                }
            }
        } else {
            for (int k = 0; k < cnt; ++k) {
                const uint32_t w = (uint32_t)cw[k];
#pragma unroll
                for (int r = 0; r < kFrRows; ++r) {
                    if (r < nrows) {
                        const uint8_t *q = grow[r] + 3 * (int64_t)(lo + k);
                        acc[r][0] += w * q[0];
                        acc[r][1] += w * q[1];
                        acc[r][2] += w * q[2];
                    }
                }
            }
        }
#pragma unroll
        for (int r = 0; r < kFrRows; ++r) {
            if (r < nrows) {
                uint8_t *d = out_s + r * t.out_pitch + 3 * tid;
                d[0] = (uint8_t)clamp_shift(acc[r][0]);
                d[1] = (uint8_t)clamp_shift(acc[r][1]);
                d[2] = (uint8_t)clamp_shift(acc[r][2]);
            }
        }
    }
    __syncthreads();

    for (int r = 0; r < nrows; ++r) {
        const uint8_t *S = out_s + r * t.out_pitch;
        if (mid) {
            // 3 * x0 is a multiple of 48; the last tile's last chunk ends inside the row's padding (mid_pitch = 3 W rounded up to 16)
            uint8_t *d = mid + ((int64_t)f * Hs + y0 + r) * mid_pitch + 3 * x0;
            for (int i = tid; i < (3 * npx + 15) / 16; i += kFrThreads)
                reinterpret_cast<uint4 *>(d)[i] = reinterpret_cast<const uint4 *>(S)[i];
        } else {
            frames_emit(o, lut_s, S, f, y0 + r, x0, npx);
        }
    }
}

// four bytes of a row from p, of which `valid` (1..4) belong to it; one load where the address is known to be aligned
__device__ __forceinline__ uint32_t frames_load4(const uint8_t *p, int valid, bool aligned4) {
    if (aligned4 && valid == 4) return *reinterpret_cast<const uint32_t *>(p);
    uint32_t v = 0;
    for (int k = 0; k < valid; ++k) v |= (uint32_t)p[k] << (8 * k);
    return v;
}

// grid: column tile fastest, then output row, then frame.  `in`: rows of 3 W bytes (the intermediate, or the source when the
// width keeps its size), Hin of them.  coef == null: the row itself (both axes keep their size).
__global__ __launch_bounds__(kFrThreads) void frames_vpass_kernel(const uint8_t *__restrict__ in, int64_t fs_in, int64_t rs_in,
                                                                  int aligned4, int Hin, int xtiles,
                                                                  const int32_t *__restrict__ bounds,
                                                                  const int32_t *__restrict__ coef, int ksize, FrameOut o) {
    __shared__ float lut_s[3 * 256];
    __shared__ uint4 S4[kFrTileBytes / 16];
    unsigned g = blockIdx.x;
    const int xt = g % xtiles; g /= xtiles;
    const int y = g % o.H;
    const int f = g / o.H;
    const int tid = threadIdx.x;
    const int x0 = xt * kFrThreads, npx = min(kFrThreads, o.W - x0);
    frames_load_lut(o, lut_s);

    const int b0 = 3 * x0 + 4 * tid;                       // this lane's four bytes of the row
    const int valid = clampi(3 * o.W - b0, 0, 4);
    if (4 * tid < kFrTileBytes && valid > 0) {
        const uint8_t *base = in + f * fs_in + b0;
        uint32_t v;
        if (coef) {
            const int lo = clampi(bounds[2 * y], 0, Hin);
            const int cnt = clampi(bounds[2 * y + 1], 0, min(ksize, Hin - lo));
            const int32_t *cw = coef + (int64_t)y * ksize;
            uint32_t acc[4] = {1u << 21, 1u << 21, 1u << 21, 1u << 21};
#pragma unroll 4
            for (int k = 0; k < cnt; ++k) {
                const uint32_t w = (uint32_t)cw[k];
                const uint32_t s = frames_load4(base + (int64_t)(lo + k) * rs_in, valid, aligned4 != 0);
                acc[0] += w * (s & 255u);
                acc[1] += w * ((s >> 8) & 255u);
                acc[2] += w * ((s >> 16) & 255u);
                acc[3] += w * (s >> 24);
            }
            v = clamp_shift(acc[0]) | clamp_shift(acc[1]) << 8 | clamp_shift(acc[2]) << 16 | clamp_shift(acc[3]) << 24;
        } else {
            v = frames_load4(base + (int64_t)y * rs_in, valid, aligned4 != 0);
        }
        reinterpret_cast<uint32_t *>(S4)[tid] = v;
    }
    __syncthreads();
    frames_emit(o, lut_s, reinterpret_cast<const uint8_t *>(S4), f, y, x0, npx);
}

// grid as frames_vpass_kernel.  tables: tab_y [H], then tab_x [W]; any values (an index outside the source reads as 0)
__global__ __launch_bounds__(kFrThreads) void frames_nearest_kernel(const uint8_t *__restrict__ src, int64_t fs_src, int64_t rs_src,
                                                                    int Hs, int Ws, int xtiles, const int32_t *__restrict__ tables,
                                                                    FrameOut o) {
    __shared__ float lut_s[3 * 256];
    __shared__ uint4 S4[kFrTileBytes / 16];
    uint8_t *S = reinterpret_cast<uint8_t *>(S4);
    unsigned g = blockIdx.x;
    const int xt = g % xtiles; g /= xtiles;
    const int y = g % o.H;
    const int f = g / o.H;
    const int tid = threadIdx.x;
    const int x0 = xt * kFrThreads, npx = min(kFrThreads, o.W - x0);
    frames_load_lut(o, lut_s);
    if (tid < npx) {
        const int sy = tables[y], sx = tables[o.H + x0 + tid];
        const bool ok = sy >= 0 && sy < Hs && sx >= 0 && sx < Ws;
        const uint8_t *p = src + f * fs_src + (int64_t)(ok ? sy : 0) * rs_src + 3 * (ok ? sx : 0);
        S[3 * tid + 0] = ok ? p[0] : (uint8_t)0;
        S[3 * tid + 1] = ok ? p[1] : (uint8_t)0;
        S[3 * tid + 2] = ok ? p[2] : (uint8_t)0;
    }
    __syncthreads();
    frames_emit(o, lut_s, S, f, y, x0, npx);
}

static inline int64_t mid_pitch_of(int W) { return ((int64_t)3 * W + 15) / 16 * 16; }

// Answers 1 - 3 of include/dmm_match.h (16) that the two entries share.  *go = true: go on.
static int frames_check(const void *src, int64_t fs_src, int64_t rs_src, int n, int C, int Hs, int Ws, int H, int W,
                        bool src_needed, const void *lut, const void *out_f32, int64_t fs_out, int64_t ps_out, const void *out_u8,
                        int64_t fs_u8, bool *go) {
    *go = false;
    if (n < 0 || C < 0 || Hs < 0 || Ws < 0 || H < 0 || W < 0) return DMM_ERR_BAD_ARG;
    const int64_t HW = (int64_t)H * W;
    if (rs_src < (int64_t)3 * Ws || fs_src < (int64_t)Hs * 3 * Ws) return DMM_ERR_BAD_ARG;
    if (out_f32 && (ps_out < HW || fs_out < HW)) return DMM_ERR_BAD_ARG;
    if (out_u8 && fs_u8 < HW * 3) return DMM_ERR_BAD_ARG;
    if (n == 0 || HW == 0) return DMM_OK;
    if ((src_needed && !src) || (!out_f32 && !out_u8) || (out_f32 && !lut)) return DMM_ERR_BAD_ARG;
    *go = true;
    return DMM_OK;
}

static bool frames_too_large(int C, int Hs, int Ws, int H, int W) {
    const int64_t two31 = (int64_t)1 << 31;
    return C != 3 || Hs > DMM_NEAREST_MAX_AXIS || Ws > DMM_NEAREST_MAX_AXIS || H > DMM_NEAREST_MAX_AXIS ||
           W > DMM_NEAREST_MAX_AXIS || (int64_t)Hs * Ws * 3 >= two31 || (int64_t)H * W * 3 >= two31 ||
           (int64_t)Hs * W * 3 >= two31;
}

}  // namespace dmm

extern "C" size_t dmm_prepare_frames_workspace_bytes(int n, int Hs, int Ws, int H, int W) {
    if (n <= 0 || Hs <= 0 || Ws <= 0 || H <= 0 || W <= 0 || Hs == H || Ws == W) return 0;
    return (size_t)n * (size_t)Hs * (size_t)dmm::mid_pitch_of(W);
}

extern "C" int dmm_prepare_frames_u8(const uint8_t *src, int64_t fs_src, int64_t rs_src, int n, int C, int Hs, int Ws, int H,
                                     int W, const int32_t *bounds_x, const int32_t *coef_x, int ksize_x, const int32_t *bounds_y,
                                     const int32_t *coef_y, int ksize_y, const float *lut, float *out_f32, int64_t fs_out,
                                     int64_t ps_out, uint8_t *out_u8, int64_t fs_u8, void *workspace, size_t workspace_bytes,
                                     dmm_stream_t stream) {
    using namespace dmm;
    if (ksize_x < 0 || ksize_y < 0) return DMM_ERR_BAD_ARG;
    bool go;
    int rc = frames_check(src, fs_src, rs_src, n, C, Hs, Ws, H, W, true, lut, out_f32, fs_out, ps_out, out_u8, fs_u8, &go);
    if (!go) return rc;
    const bool hx = Ws != W, vy = Hs != H;
    if (hx && (!bounds_x || !coef_x || ksize_x == 0)) return DMM_ERR_BAD_ARG;
    if (vy && (!bounds_y || !coef_y || ksize_y == 0)) return DMM_ERR_BAD_ARG;
    if (frames_too_large(C, Hs, Ws, H, W) || Hs == 0 || Ws == 0) return DMM_ERR_UNSUPPORTED;
    if ((hx && ksize_x > DMM_RESAMPLE_MAX_TAPS) || (vy && ksize_y > DMM_RESAMPLE_MAX_TAPS)) return DMM_ERR_UNSUPPORTED;
    const HTile t = hx ? h_tile(Ws, W, ksize_x, !vy) : HTile{};
    const int row_groups = hx ? (Hs + t.rows - 1) / t.rows : 0;
    const int xtiles = (W + kFrThreads - 1) / kFrThreads;
    // (a grid stays below 2^32 threads, as in (14d))
    if ((hx && (int64_t)n * row_groups * t.tiles_x >= DMM_RESIZE_MAX_WORKGROUPS) || (int64_t)n * H * xtiles >= DMM_RESIZE_MAX_WORKGROUPS)
        return DMM_ERR_UNSUPPORTED;
    const size_t need = dmm_prepare_frames_workspace_bytes(n, Hs, Ws, H, W);
    if (need && (!workspace || workspace_bytes < need || ((uintptr_t)workspace & 15) != 0)) return DMM_ERR_WORKSPACE;

    const hipStream_t s = (hipStream_t)stream;
    const FrameOut o{lut, out_f32, fs_out, ps_out, out_u8, fs_u8, H, W};
    uint8_t *mid = hx && vy ? (uint8_t *)workspace : nullptr;
    const int64_t pitch = mid_pitch_of(W);
    if (hx) {
        hipLaunchKernelGGL(frames_hpass_kernel, dim3((unsigned)((int64_t)n * row_groups * t.tiles_x)), dim3(kFrThreads), t.lds, s,
                           src, fs_src, rs_src, Hs, Ws, W, bounds_x, coef_x, ksize_x, t, row_groups, mid, pitch, o);
        rc = check_launch();
        if (rc != DMM_OK || !vy) return rc;
    }
    const uint8_t *in = mid ? mid : src;
    const int64_t fs_in = mid ? (int64_t)Hs * pitch : fs_src, rs_in = mid ? pitch : rs_src;
    const int aligned4 = ((uintptr_t)in & 3) == 0 && fs_in % 4 == 0 && rs_in % 4 == 0;
    hipLaunchKernelGGL(frames_vpass_kernel, dim3((unsigned)((int64_t)n * H * xtiles)), dim3(kFrThreads), 0, s, in, fs_in, rs_in,
                       aligned4, Hs, xtiles, vy ? bounds_y : nullptr, vy ? coef_y : nullptr, ksize_y, o);
    return check_launch();
}

extern "C" int dmm_prepare_frames_nearest_u8(const uint8_t *src, int64_t fs_src, int64_t rs_src, int n, int C, int Hs, int Ws,
                                             int H, int W, const int32_t *tables, const float *lut, float *out_f32, int64_t fs_out,
                                             int64_t ps_out, uint8_t *out_u8, int64_t fs_u8, dmm_stream_t stream) {
    using namespace dmm;
    bool go;
    const int rc = frames_check(src, fs_src, rs_src, n, C, Hs, Ws, H, W, (int64_t)Hs * Ws != 0, lut, out_f32, fs_out, ps_out,
                                out_u8, fs_u8, &go);
    if (!go) return rc;
    if (!tables) return DMM_ERR_BAD_ARG;
    const int xtiles = (W + kFrThreads - 1) / kFrThreads;
    if (frames_too_large(C, Hs, Ws, H, W) || (int64_t)n * H * xtiles >= DMM_RESIZE_MAX_WORKGROUPS)
        return DMM_ERR_UNSUPPORTED;
    const FrameOut o{lut, out_f32, fs_out, ps_out, out_u8, fs_u8, H, W};
    hipLaunchKernelGGL(frames_nearest_kernel, dim3((unsigned)((int64_t)n * H * xtiles)), dim3(kFrThreads), 0, (hipStream_t)stream,
                       src, fs_src, rs_src, Hs, Ws, xtiles, tables, o);
    return check_launch();
}
