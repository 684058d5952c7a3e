// dmm_augment.hip -- (15) the clip augmentation of a training step: one nearest-neighbour affine warp per frame, applied to the
// image planes, the annotation and every pasted proposal mask, with the proposals' boxes and the target planes out of the same
// pass.  Replaces dmm/dataloader/dataset.py:222-258 (flip, Affine(tf_matrix, interp='nearest') on img, annot and each mask,
// binmask_to_bbox_xyxy_pt of (mask > 0.5)) and sequence_from_masks (:300-338) on the warped annotation; the warp itself is
// th_affine2d(center=True) + th_nearest_interp2d (dmm/dataloader/transforms/utils.py:67-148).
//   warp    one workgroup = one tile of output pixels of one frame, one pixel per thread.  The source index of the pixel is
//           computed ONCE (fp32, one rounding per operation, the order of include/dmm_match.h (15)) and reused over all planes:
//           a 4-byte gather per plane, a coalesced store.  The mask gathers go out kAugBatch at a time before the first is
//           waited for: one plane per round trip took 202 us for the config-4 clip set, batches of eight 145 us.
//   boxes   a wave covers whole tile rows (or a 64-pixel piece of one), so the ballot of (value > 0.5) IS the wave's reduction:
//           first / last set bit give the columns and rows.  Waves meet in LDS (integer max), workgroups in the table (integer
//           max), which lives in boxes_out itself until the finish launch turns it into floats.  All four sides are kept as
//           maxima (W - xmin, H - ymin, xmax + 1, ymax + 1) so that the table clears to ZERO = "empty".
//   targets (label == o + 1) as 1.0 / 0.0 per plane; the plane's ballot popcount is the wave's share of sizes[f, o].
// Integer max and integer add commute: the bytes are the same on every run.
#include "dmm_launchers.h"

#ifndef DMM_AUG_TILE_W
#define DMM_AUG_TILE_W 64                                  // columns of a workgroup's tile (profiles/r10_augment.md)
#endif
#ifndef DMM_AUG_BATCH
#define DMM_AUG_BATCH 8                                    // mask gathers a thread has in flight (same file)
#endif

namespace dmm {

constexpr int kAugThreads = 256;                           // four waves, one output pixel per thread
constexpr int kAugTileW = DMM_AUG_TILE_W;
constexpr int kAugTileH = kAugThreads / kAugTileW;
constexpr int kAugBoxChunk = 64;                           // mask planes whose boxes meet in LDS before they go to the table
constexpr int kAugBatch = DMM_AUG_BATCH;                   // mask planes whose gathers a thread has in flight
constexpr int kAugMaxF = DMM_AUGMENT_MAX_TARGETS;
static_assert(kAugTileW >= 1 && kAugTileW <= kAugThreads && (kAugTileW & (kAugTileW - 1)) == 0, "the tile width is a power of two");

__global__ __launch_bounds__(256) void augment_clear_kernel(int32_t *__restrict__ a, int64_t na, int32_t *__restrict__ b,
                                                            int64_t nb) {
    const int64_t step = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < na + nb; i += step) {
        if (i < na) a[i] = 0;
        else b[i - na] = 0;
    }
}

struct AugPlanes {
    const float *frames_in;
    float *frames_out;
    const uint8_t *labels_in;
    uint8_t *labels_out;
    const float *masks_in;
    float *masks_out;
    int64_t fs_fin, ps_fin, fs_fout, ps_fout, fs_lin, fs_lout, fs_min, ps_min, fs_mout, ps_mout;
};

// grid: tile column fastest, then tile row, then frame
__global__ __launch_bounds__(kAugThreads) void augment_warp_kernel(AugPlanes a, const float *__restrict__ matrices,
                                                                   const int32_t *__restrict__ flips, int C, int P, int F,
                                                                   int H, int W, float cr, float cc, int tiles_x, int tiles_y,
                                                                   int32_t *__restrict__ box_table, float *__restrict__ targets,
                                                                   int32_t *__restrict__ sizes) {
    __shared__ int box_s[kAugBoxChunk * 4];
    __shared__ int size_s[kAugMaxF];
    unsigned g = blockIdx.x;
    const int tx = g % tiles_x; g /= tiles_x;
    const int ty = g % tiles_y;
    const int f = g / tiles_y;
    const int lane = threadIdx.x % kWave, wave = threadIdx.x / kWave;
    const int r = ty * kAugTileH + (int)threadIdx.x / kAugTileW, c = tx * kAugTileW + (int)threadIdx.x % kAugTileW;
    const bool in = r < H && c < W;
    const int64_t HW = (int64_t)H * W;

    for (int i = threadIdx.x; i < kAugBoxChunk * 4; i += kAugThreads) box_s[i] = 0;
    for (int i = threadIdx.x; i < F; i += kAugThreads) size_s[i] = 0;

    // the source pixel: include/dmm_match.h (15), one fp32 rounding per operation (the library is built without contraction)
    const float *m = matrices + (int64_t)f * 9;
    const float x = (float)r - cr, y = (float)c - cc;
    const float sr = (((m[0] * x) + (m[1] * y)) + m[2]) + cr;
    const float sc = (((m[3] * x) + (m[4] * y)) + m[5]) + cc;
    int ri = (int)rintf(fminf(fmaxf(sr, 0.0f), (float)(H - 1)));
    int ci = (int)rintf(fminf(fmaxf(sc, 0.0f), (float)(W - 1)));
    ri = min(max(ri, 0), H - 1);                           // (no-ops while H - 1 and W - 1 are exact in fp32; a NaN lands on 0)
    ci = min(max(ci, 0), W - 1);
    if (flips && flips[f]) ci = W - 1 - ci;
    const int64_t src = in ? (int64_t)ri * W + ci : 0, dst = (int64_t)r * W + c;
    __syncthreads();

    {   // the image planes
        const float *pi = a.frames_in + f * a.fs_fin;
        float *po = a.frames_out + f * a.fs_fout;
#pragma unroll 4
        for (int ch = 0; ch < C; ++ch)
            if (in) po[ch * a.ps_fout + dst] = pi[ch * a.ps_fin + src];
    }

    {   // the annotation, its target planes and their sizes
        const int lab = in ? a.labels_in[f * a.fs_lin + src] : 0;
        if (in) a.labels_out[f * a.fs_lout + dst] = (uint8_t)lab;
        float *tg = targets + (int64_t)f * F * HW;
        for (int o = 0; o < F; ++o) {
            const bool hit = in && lab == o + 1;
            if (in) tg[o * HW + dst] = hit ? 1.0f : 0.0f;
            const unsigned long long b = __ballot(hit);
            if (lane == 0 && b) atomicAdd(&size_s[o], __popcll(b));
        }
    }

    // the proposal masks and their boxes.  The wave's pixels: rows r_w .. r_w + rows - 1 of the tile, `seg` columns from c_w
    constexpr int seg = kAugTileW < kWave ? kAugTileW : kWave;
    const int r_w = ty * kAugTileH + wave * kWave / kAugTileW, c_w = tx * kAugTileW + wave * kWave % kAugTileW;
    const float *mi = a.masks_in + f * a.fs_min;
    float *mo = a.masks_out + f * a.fs_mout;
    for (int p0 = 0; p0 < P; p0 += kAugBoxChunk) {
        const int np = min(kAugBoxChunk, P - p0);
        // kAugBatch planes at a time: all their gathers are issued before the first ballot waits for one
        for (int k0 = 0; k0 < np; k0 += kAugBatch) {
            float v[kAugBatch];
#pragma unroll
            for (int u = 0; u < kAugBatch; ++u) v[u] = in && k0 + u < np ? mi[(p0 + k0 + u) * a.ps_min + src] : 0.0f;
#pragma unroll
            for (int u = 0; u < kAugBatch; ++u) {
                const int k = k0 + u;
                if (k >= np) break;
                if (in) mo[(p0 + k) * a.ps_mout + dst] = v[u];
                const unsigned long long b = __ballot(v[u] > 0.5f);
                if (b) {                                   // (wave-uniform)
                    const int lo = __ffsll(b) - 1, hi = 63 - __clzll(b);
                    unsigned long long cols = b;
                    if (seg < kWave) {
                        cols = 0;
#pragma unroll
                        for (int s = 0; s < kWave / seg; ++s) cols |= b >> (s * seg);
                        cols &= (1ull << (seg % 64)) - 1;
                    }
                    const int xmin = c_w + __ffsll(cols) - 1, xmax = c_w + 63 - __clzll(cols);
                    const int ymin = r_w + lo / seg, ymax = r_w + hi / seg;
                    if (lane == 0) {
                        atomicMax(&box_s[k * 4 + 0], W - xmin);
                        atomicMax(&box_s[k * 4 + 1], H - ymin);
                        atomicMax(&box_s[k * 4 + 2], xmax + 1);
                        atomicMax(&box_s[k * 4 + 3], ymax + 1);
                    }
                }
            }
        }
        __syncthreads();
        for (int i = threadIdx.x; i < np * 4; i += kAugThreads) {
            const int v = box_s[i];
            if (v) {
                atomicMax(&box_table[((int64_t)f * P + p0) * 4 + i], v);
                box_s[i] = 0;
            }
        }
        __syncthreads();
    }

    __syncthreads();
    for (int o = threadIdx.x; o < F; o += kAugThreads)
        if (size_s[o]) atomicAdd(&sizes[(int64_t)f * F + o], size_s[o]);
}

// the table (W - xmin, H - ymin, xmax + 1, ymax + 1; all zero = empty) -> xyxy floats in place, or the caller's box
__global__ __launch_bounds__(256) void augment_box_finish_kernel(float *__restrict__ boxes_out, const float *__restrict__ boxes_in,
                                                                 int32_t *__restrict__ box_valid, int64_t n_boxes, int H, int W) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_boxes) return;
    const int32_t *t = reinterpret_cast<const int32_t *>(boxes_out) + i * 4;
    const int t0 = t[0], t1 = t[1], t2 = t[2], t3 = t[3];
    const bool any = t2 != 0;
    float *o = boxes_out + i * 4;
    const float *bi = boxes_in + i * 4;
    o[0] = any ? (float)(W - t0) : bi[0];
    o[1] = any ? (float)(H - t1) : bi[1];
    o[2] = any ? (float)(t2 - 1) : bi[2];
    o[3] = any ? (float)(t3 - 1) : bi[3];
    box_valid[i] = any ? 1 : 0;
}

struct AugTiles {
    int tiles_x, tiles_y;
};
static inline AugTiles aug_tiles(int H, int W) {
    return {(W + kAugTileW - 1) / kAugTileW, (H + kAugTileH - 1) / kAugTileH};
}

}  // namespace dmm

extern "C" size_t dmm_augment_clip_workspace_bytes(int n, int C, int P, int F, int H, int W) {
    (void)n; (void)C; (void)P; (void)F; (void)H; (void)W;
    return 0;                                              // the box table lives in boxes_out until the finish launch
}

extern "C" int dmm_augment_clip_f32(const float *frames_in, int64_t fs_frames_in, int64_t ps_frames_in, float *frames_out,
                                    int64_t fs_frames_out, int64_t ps_frames_out, const uint8_t *labels_in, int64_t fs_labels_in,
                                    uint8_t *labels_out, int64_t fs_labels_out, const float *masks_in, int64_t fs_masks_in,
                                    int64_t ps_masks_in, float *masks_out, int64_t fs_masks_out, int64_t ps_masks_out,
                                    const float *boxes_in, float *boxes_out, int32_t *box_valid, float *targets, int32_t *sizes,
                                    const float *matrices, const int32_t *flips, int n, int C, int P, int F, int H, int W,
                                    void *workspace, size_t workspace_bytes, dmm_stream_t stream) {
    using namespace dmm;
    // 1. sizes and strides
    if (n < 0 || C < 0 || P < 0 || F < 0 || H < 0 || W < 0) return DMM_ERR_BAD_ARG;
    const int64_t HW = (int64_t)H * W;
    if (C > 0 && (ps_frames_in < HW || ps_frames_out < HW || fs_frames_in < HW || fs_frames_out < HW)) return DMM_ERR_BAD_ARG;
    if (fs_labels_in < HW || fs_labels_out < HW) return DMM_ERR_BAD_ARG;
    if (P > 0 && (ps_masks_in < HW || ps_masks_out < HW || fs_masks_in < HW || fs_masks_out < HW)) return DMM_ERR_BAD_ARG;
    // 2. nothing to do
    if (n == 0 || HW == 0) return DMM_OK;
    // 3. pointers
    if (!labels_in || !labels_out || !matrices) return DMM_ERR_BAD_ARG;
    if (C > 0 && (!frames_in || !frames_out)) return DMM_ERR_BAD_ARG;
    if (P > 0 && (!masks_in || !masks_out || !boxes_in || !boxes_out || !box_valid)) return DMM_ERR_BAD_ARG;
    if (F > 0 && (!targets || !sizes)) return DMM_ERR_BAD_ARG;
    if ((const void *)labels_in == (const void *)labels_out || (C > 0 && frames_in == frames_out) ||
        (P > 0 && (masks_in == masks_out || boxes_in == boxes_out)))
        return DMM_ERR_BAD_ARG;                            // a gather cannot run in place
    // 4. the envelope
    const AugTiles t = aug_tiles(H, W);
    const int64_t two31 = (int64_t)1 << 31;
    if (HW >= two31 || F > kAugMaxF || (int64_t)n * t.tiles_x * t.tiles_y >= two31 || (int64_t)n * P * 4 >= two31 ||
        (int64_t)n * F >= two31)
        return DMM_ERR_UNSUPPORTED;
    // 5. workspace
    const size_t need = dmm_augment_clip_workspace_bytes(n, C, P, F, H, W);
    if (need && (!workspace || workspace_bytes < need)) return DMM_ERR_WORKSPACE;

    const hipStream_t s = (hipStream_t)stream;
    const int64_t n_table = (int64_t)n * P * 4, n_sizes = (int64_t)n * F;
    if (n_table + n_sizes > 0) {
        int64_t blocks = (n_table + n_sizes + 255) / 256;
        if (blocks > 1024) blocks = 1024;
        hipLaunchKernelGGL(augment_clear_kernel, dim3((unsigned)blocks), dim3(256), 0, s, reinterpret_cast<int32_t *>(boxes_out),
                           n_table, sizes, n_sizes);
        const int rc = check_launch();
        if (rc != DMM_OK) return rc;
    }
    AugPlanes a{frames_in, frames_out, labels_in, labels_out, masks_in, masks_out, fs_frames_in, ps_frames_in, fs_frames_out,
                ps_frames_out, fs_labels_in, fs_labels_out, fs_masks_in, ps_masks_in, fs_masks_out, ps_masks_out};
    const float cr = (float)(H / 2.0 - 0.5), cc = (float)(W / 2.0 - 0.5);
    hipLaunchKernelGGL(augment_warp_kernel, dim3((unsigned)((int64_t)n * t.tiles_x * t.tiles_y)), dim3(kAugThreads), 0, s, a,
                       matrices, flips, C, P, F, H, W, cr, cc, t.tiles_x, t.tiles_y, reinterpret_cast<int32_t *>(boxes_out),
                       targets, sizes);
    int rc = check_launch();
    if (rc != DMM_OK || P == 0) return rc;
    const int64_t n_boxes = (int64_t)n * P;
    hipLaunchKernelGGL(augment_box_finish_kernel, dim3((unsigned)((n_boxes + 255) / 256)), dim3(256), 0, s, boxes_out, boxes_in,
                       box_valid, n_boxes, H, W);
    return check_launch();
}
