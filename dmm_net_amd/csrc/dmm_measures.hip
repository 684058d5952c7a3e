// dmm_measures.hip -- (14) the integer counts under the DAVIS region similarity J and boundary measure F of a clip:
// db_eval_iou (dmm/measures/jaccard.py:15-37) and db_eval_boundary with seg2bmap (dmm/measures/f_boundary.py:14-78, :80-140)
// as db_eval_sequence calls them per object and frame (dmm/dataloader/evaluation.py:44-46: an == obj_id, sg == obj_id).
// One kernel, one read of the two label maps per (frame, object) tile, everything else on 64-bit words in LDS:
//   1. ballot    label == id -> row-major 1-bit words of S (prediction) and A (annotation); popcounts of S & A and S | A
//   2. boundary  seg2bmap by word shifts with the carry bit of the next word; popcounts of the two boundary planes
//   3. dilate    only where the OTHER boundary has a bit in the word: the disk dilation of that word, AND, popcount
// The disk {dx^2 + dy^2 <= r^2} column by column: out = OR over dx of shift(U_v(dx), dx), U_m[y] = OR of the rows y - m .. y + m,
// v(dx) = floor(sqrt(r^2 - dx^2)).  v grows as |dx| falls from r to 0, so one walk adds each row to U once and shifts U once
// per dx: 2 r + 1 rows and r + 1 shifted pairs per word instead of a full footprint.  All outputs are integers and integer
// addition commutes: the atomics below give the same bytes on every run.
// (14b), (14d): the reference's nearest resize of a prediction whose size is not the annotation's (jaccard.py:28-32,
// f_boundary.py:34-38; PIL's ImagingScaleAffine) as two index tables walked by sequential double additions and one gather
// pass into a frame of the annotation's size, which (14) then scores.  (A gather inside stage 1 instead -- (14c) -- was built
// and measured slower than these two steps: every object's workgroups repeat it.  profiles/r13_davis_resized.md.)
#include "dmm_launchers.h"

namespace dmm {

constexpr int kMeasThreads = 256;                          // four waves
constexpr int kMeasWaves = kMeasThreads / kWave;
constexpr int kMeasBatch = 8;                             // region words a wave loads before it ballots the first
constexpr int kMeasCap = 1280;                             // 64-bit words per LDS plane; four planes = 40 KiB
constexpr int kMeasMaxRadius = DMM_DAVIS_MAX_RADIUS;
typedef unsigned long long word_t;

// The tile of one workgroup: `bh` rows x `tw` words of output.  Its region is `bh + 2 r + 1` mask rows (r above, r + 1 below:
// a boundary row reads the mask row under it) by `tw + 2` words (one word either side: r <= 63 crosses one word boundary).
struct MeasTile {
    int bh, tw, bands, xtiles;
};
static inline MeasTile meas_tile(int H, int W, int radius) {
    MeasTile t;
    t.bh = DMM_DAVIS_BAND_ROWS(radius);
    if (t.bh > H) t.bh = H;
    const int rows = t.bh + 2 * radius + 1, wpr = (W + 63) / 64;
    t.tw = kMeasCap / rows - 2;                            // rows <= 64 + 127: at least 4
    if (t.tw > wpr) t.tw = wpr;
    t.bands = (H + t.bh - 1) / t.bh;
    t.xtiles = (wpr + t.tw - 1) / t.tw;
    return t;
}

__device__ __forceinline__ int wave_sum_i32(int v) {
#pragma unroll
    for (int m = 1; m < kWave; m <<= 1) v += __shfl_xor(v, m, kWave);
    return v;
}

// grid: xtile fastest, then band, object, frame -- the objects of a frame run side by side and share its lines in L2.
__global__ __launch_bounds__(kMeasThreads) void davis_counts_kernel(
    const uint8_t *__restrict__ pred, const uint8_t *__restrict__ gt, int n_obj, int H, int W, int64_t fs_pred, int64_t fs_gt,
    int radius, int bh, int tw, int bands, int xtiles, int32_t *__restrict__ counts) {
    __shared__ word_t plane_s[4][kMeasCap];                // mask S | mask A | boundary of S | boundary of A
    __shared__ int cnt_s[6];
    unsigned g = blockIdx.x;
    const int xt = g % xtiles; g /= xtiles;
    const int band = g % bands; g /= bands;
    const int o = g % n_obj;
    const int f = g / n_obj;
    const int id = o + 1;
    const int twh = tw + 2, rows = bh + 2 * radius + 1, wpr = (W + 63) / 64;
    const int y_top = band * bh - radius;                  // image row of region row 0
    const int w_left = xt * tw - 1;                        // image word of region word 0
    const int lane = threadIdx.x % kWave, wave = threadIdx.x / kWave;
    const uint8_t *p = pred + (int64_t)f * fs_pred, *a = gt + (int64_t)f * fs_gt;
    word_t *mS = plane_s[0], *mA = plane_s[1], *bS = plane_s[2], *bA = plane_s[3];
    if (threadIdx.x < 6) cnt_s[threadIdx.x] = 0;
    int cnt[6] = {0, 0, 0, 0, 0, 0};

    // 1. one wave ballot per region word; words off the image are zero ("zero where the shift leaves the image").  A wave takes
    // kMeasBatch consecutive words at a time and issues all their loads before the first ballot: one word per round trip to
    // memory made this stage the whole kernel's time.
    const int n_words = rows * twh;
    for (int i0 = wave * kMeasBatch; i0 < n_words; i0 += kMeasWaves * kMeasBatch) {
        int lp[kMeasBatch], la[kMeasBatch];
#pragma unroll
        for (int u = 0; u < kMeasBatch; ++u) {
            const int i = i0 + u, ry = i / twh, cw = i - ry * twh;
            const int y = y_top + ry, xw = w_left + cw, x = xw * 64 + lane;
            const bool in = i < n_words && y >= 0 && y < H && xw >= 0 && x < W;
            const int64_t at = (int64_t)y * W + x;
            lp[u] = in ? p[at] : 0;                        // (0 is no object's label)
            la[u] = in ? a[at] : 0;
        }
#pragma unroll
        for (int u = 0; u < kMeasBatch; ++u) {
            const int i = i0 + u, ry = i / twh, cw = i - ry * twh;
            if (i >= n_words) break;
            const word_t S = __ballot(lp[u] == id), A = __ballot(la[u] == id);
            if (ry >= radius && ry < radius + bh && cw >= 1 && cw <= tw) {
                cnt[0] += __popcll(S & A);                 // (wave-uniform: lane 0's copy is the one that is added)
                cnt[1] += __popcll(S | A);
            }
            if (lane == 0) {
                mS[i] = S;
                mA[i] = A;
            }
        }
    }
    if (lane != 0) cnt[0] = cnt[1] = 0;
    __syncthreads();

    // 2. seg2bmap, one thread per word of the rows - 1 boundary rows.  e / s / se: the mask shifted towards the origin from
    // the east / south / south-east.  The order of f_boundary.py:117-122: all three inside, the last row m ^ e, then the last
    // column m ^ s, then the corner 0.  (The word right of the region is not there: its carry reaches bit 63 of the right
    // halo word only, and a shift of at most 63 does not bring that bit into the tile.)
    for (int i = threadIdx.x; i < (rows - 1) * twh; i += kMeasThreads) {
        const int ry = i / twh, cw = i - ry * twh;
        const int y = y_top + ry, xw = w_left + cw;
        word_t b[2] = {0, 0};
        if (y >= 0 && y < H && xw >= 0 && xw < wpr) {
            const bool carry = cw + 1 < twh;
            const word_t last = (W - 1) / 64 == xw ? (word_t)1 << ((W - 1) & 63) : 0;
#pragma unroll
            for (int k = 0; k < 2; ++k) {
                const word_t *m_ = k ? mA : mS;
                const word_t m = m_[i], mn = carry ? m_[i + 1] : 0;
                const word_t s = m_[i + twh], sn = carry ? m_[i + twh + 1] : 0;       // (zeros under the image)
                const word_t e = (m >> 1) | (mn << 63), se = (s >> 1) | (sn << 63);
                word_t v = y == H - 1 ? (m ^ e) : ((m ^ e) | (m ^ s) | (m ^ se));
                v = (v & ~last) | ((m ^ s) & last);
                if (y == H - 1) v &= ~last;
                b[k] = v;
            }
            if (ry >= radius && ry < radius + bh && cw >= 1 && cw <= tw) {
                cnt[2] += __popcll(b[0]);
                cnt[3] += __popcll(b[1]);
            }
        }
        bS[i] = b[0];
        bA[i] = b[1];
    }
    __syncthreads();

    // 3. one thread per (tile word, side): side 0 = boundary of S against the dilated boundary of A (slot 4), side 1 the
    // reverse (slot 5).  Rows ry - m .. ry + m stay inside the boundary planes: the halo is `radius` rows on both sides.
    const int r2 = radius * radius;
    for (int j = threadIdx.x; j < 2 * bh * tw; j += kMeasThreads) {
        const int side = j & 1, jj = j >> 1;
        const int by = jj / tw, cw = jj - by * tw + 1;
        const int ry = by + radius;
        const word_t *tgt_ = side ? bA : bS, *src = side ? bS : bA;
        const word_t tgt = tgt_[ry * twh + cw];
        if (tgt == 0) continue;
        const word_t *c = src + ry * twh + cw;
        word_t u0 = c[-1], u1 = c[0], u2 = c[1], acc = 0;
        int v = 0;
        for (int k = radius; k >= 1; --k) {
            while ((v + 1) * (v + 1) + k * k <= r2) {
                ++v;
                const word_t *up = c - v * twh, *dn = c + v * twh;
                u0 |= up[-1] | dn[-1];
                u1 |= up[0] | dn[0];
                u2 |= up[1] | dn[1];
            }
            acc |= (u1 << k) | (u0 >> (64 - k)) | (u1 >> k) | (u2 << (64 - k));
            if ((acc & tgt) == tgt) break;
        }
        if ((acc & tgt) != tgt) {
            for (; v < radius;) {                          // dx = 0: the whole column
                ++v;
                u1 |= c[-v * twh] | c[v * twh];
            }
            acc |= u1;
        }
        cnt[4 + side] += __popcll(acc & tgt);
    }

    // the workgroup's six partials: lanes, then waves (LDS), then one global atomic per slot
#pragma unroll
    for (int s = 0; s < 6; ++s) {
        const int t = wave_sum_i32(cnt[s]);
        if (lane == 0 && t) atomicAdd(&cnt_s[s], t);
    }
    __syncthreads();
    if (threadIdx.x < 6 && cnt_s[threadIdx.x]) atomicAdd(&counts[((int64_t)f * n_obj + o) * 6 + threadIdx.x], cnt_s[threadIdx.x]);
}

// (14b) one lane per axis walks the source coordinate by the sequential double additions of the rule; block 0 the rows,
// block 1 the columns.  `a` comes from the launcher's own division.
__global__ __launch_bounds__(kWave) void nearest_tables_kernel(int H, int W, double ay, double ax, int32_t *__restrict__ tab) {
    if (threadIdx.x != 0) return;
    const int n = blockIdx.x ? W : H;
    const double a = blockIdx.x ? ax : ay;
    int32_t *t = tab + (blockIdx.x ? H : 0);
    double o = a * 0.5;
    for (int i = 0; i < n; ++i) {
        t[i] = o < 0 ? -1 : (int)o;
        o += a;
    }
}

// (14d) four consecutive bytes of a frame per thread, counted from the 4-byte boundary at or below the frame's first byte,
// so that every full group is one aligned 32-bit store whatever W and the frame stride are.
constexpr int kResizeThreads = 256;
__global__ __launch_bounds__(kResizeThreads) void resize_labels_kernel(
    const uint8_t *__restrict__ srcp, int Hs, int Ws, int64_t fs_src, uint8_t *__restrict__ dst, int H, int W, int64_t fs_dst,
    const int32_t *__restrict__ tab, unsigned blocks_per_frame) {
    const int f = blockIdx.x / blocks_per_frame;
    const int64_t HW = (int64_t)H * W;
    const uint8_t *s = srcp + (int64_t)f * fs_src;
    uint8_t *d = dst + (int64_t)f * fs_dst;
    const int lead = (int)((uintptr_t)d & 3);
    const int64_t i0 = ((int64_t)(blockIdx.x % blocks_per_frame) * kResizeThreads + threadIdx.x) * 4 - lead;
    if (i0 >= HW) return;
    int y = (int)((i0 < 0 ? 0 : i0) / W), x = (int)((i0 < 0 ? 0 : i0) - (int64_t)y * W);
    uint32_t v = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int64_t i = i0 + k;
        if (i < 0 || i >= HW) continue;
        const int ty = tab[y], tx = tab[H + x];
        const uint32_t l = ty >= 0 && ty < Hs && tx >= 0 && tx < Ws ? s[(int64_t)ty * Ws + tx] : 0;
        v |= l << (8 * k);
        if (++x == W) {
            x = 0;
            ++y;
        }
    }
    if (i0 >= 0 && i0 + 4 <= HW) {
        *(uint32_t *)(d + i0) = v;
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (i0 + k >= 0 && i0 + k < HW) d[i0 + k] = (uint8_t)(v >> (8 * k));
    }
}

// The answers of the entry, in the order include/dmm_match.h (14) lists.  *go = true: launch.
static int davis_counts_check(const void *pred, const void *gt, int frames, int n_obj, int H, int W, int64_t fs_pred,
                              int64_t fs_gt, int radius, const void *counts, const void *workspace, size_t workspace_bytes,
                              bool *go) {
    *go = false;
    if (frames < 0 || n_obj < 0 || H < 0 || W < 0 || radius < 0) return DMM_ERR_BAD_ARG;
    const int64_t HW = (int64_t)H * W;
    if (fs_pred < HW || fs_gt < HW) return DMM_ERR_BAD_ARG;
    if (frames == 0 || n_obj == 0) return DMM_OK;
    if (!pred || !gt || !counts) return DMM_ERR_BAD_ARG;
    if (radius > kMeasMaxRadius || n_obj > 255 || HW >= ((int64_t)1 << 31)) return DMM_ERR_UNSUPPORTED;
    if ((int64_t)frames * n_obj * 6 >= ((int64_t)1 << 31)) return DMM_ERR_UNSUPPORTED;
    if (HW > 0) {
        const MeasTile t = meas_tile(H, W, radius);
        if ((int64_t)frames * n_obj * t.bands * t.xtiles >= ((int64_t)1 << 31)) return DMM_ERR_UNSUPPORTED;   // (the grid)
    }
    const size_t need = dmm_davis_counts_workspace_bytes(frames, n_obj, H, W, radius);
    if (need && (!workspace || workspace_bytes < need)) return DMM_ERR_WORKSPACE;
    *go = true;
    return DMM_OK;
}

}  // namespace dmm

extern "C" size_t dmm_davis_counts_workspace_bytes(int frames, int n_obj, int H, int W, int radius) {
    (void)frames; (void)n_obj; (void)H; (void)W; (void)radius;
    return 0;                                              // the band partials meet in `counts` itself
}

extern "C" int dmm_davis_counts_u8(const uint8_t *pred, const uint8_t *gt, int frames, int n_obj, int H, int W,
                                   int64_t frame_stride_pred, int64_t frame_stride_gt, int radius, int32_t *counts,
                                   void *workspace, size_t workspace_bytes, dmm_stream_t stream) {
    using namespace dmm;
    bool go;
    const int rc = davis_counts_check(pred, gt, frames, n_obj, H, W, frame_stride_pred, frame_stride_gt, radius, counts,
                                      workspace, workspace_bytes, &go);
    if (!go) return rc;
    DMM_HIP_TRY(zero_async(counts, (size_t)frames * n_obj * 6 * 4, (hipStream_t)stream));
    if (H == 0 || W == 0) return DMM_OK;
    const MeasTile t = meas_tile(H, W, radius);
    const unsigned grid = (unsigned)((int64_t)frames * n_obj * t.bands * t.xtiles);
    hipLaunchKernelGGL(davis_counts_kernel, dim3(grid), dim3(kMeasThreads), 0, (hipStream_t)stream, pred, gt, n_obj, H, W,
                       frame_stride_pred, frame_stride_gt, radius, t.bh, t.tw, t.bands, t.xtiles, counts);
    return check_launch();
}

extern "C" int dmm_nearest_index_tables_i32(int Hs, int Ws, int H, int W, int32_t *tables, dmm_stream_t stream) {
    using namespace dmm;
    if (Hs < 0 || Ws < 0 || H < 0 || W < 0) return DMM_ERR_BAD_ARG;
    if (H + W == 0) return DMM_OK;
    if (!tables) return DMM_ERR_BAD_ARG;
    if (Hs > DMM_NEAREST_MAX_AXIS || Ws > DMM_NEAREST_MAX_AXIS || H > DMM_NEAREST_MAX_AXIS || W > DMM_NEAREST_MAX_AXIS)
        return DMM_ERR_UNSUPPORTED;
    const double ay = H ? (double)Hs / (double)H : 0.0, ax = W ? (double)Ws / (double)W : 0.0;    // the rule's plain division
    hipLaunchKernelGGL(nearest_tables_kernel, dim3(2), dim3(kWave), 0, (hipStream_t)stream, H, W, ay, ax, tables);
    return check_launch();
}

extern "C" int dmm_resize_labels_nearest_u8(const uint8_t *src, int Hs, int Ws, int64_t frame_stride_src, uint8_t *dst, int H,
                                            int W, int64_t frame_stride_dst, const int32_t *tables, int frames,
                                            dmm_stream_t stream) {
    using namespace dmm;
    if (frames < 0 || Hs < 0 || Ws < 0 || H < 0 || W < 0) return DMM_ERR_BAD_ARG;
    const int64_t HW = (int64_t)H * W, HWs = (int64_t)Hs * Ws;
    if (frame_stride_src < HWs || frame_stride_dst < HW) return DMM_ERR_BAD_ARG;
    if (frames == 0 || HW == 0) return DMM_OK;
    if (!src || !dst || !tables || (const void *)src == (const void *)dst) return DMM_ERR_BAD_ARG;
    if (HW >= ((int64_t)1 << 31) || HWs >= ((int64_t)1 << 31)) return DMM_ERR_UNSUPPORTED;
    const int64_t per_frame = ((HW + 3) / 4 + 1 + kResizeThreads - 1) / kResizeThreads;      // (+ 1: the group the lead splits)
    // the grid stays below 2^32 THREADS (HIP runtimes have refused gridDim.x * blockDim.x past 32 bits): 2^24 workgroups,
    // 16 GiB of output in one call
    if (per_frame * frames >= DMM_RESIZE_MAX_WORKGROUPS) return DMM_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(resize_labels_kernel, dim3((unsigned)(per_frame * frames)), dim3(kResizeThreads), 0, (hipStream_t)stream,
                       src, Hs, Ws, frame_stride_src, dst, H, W, frame_stride_dst, tables, (unsigned)per_frame);
    return check_launch();
}
