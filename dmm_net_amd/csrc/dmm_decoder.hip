// dmm_decoder.hip -- everything between the convolutions of the ConvLSTM refine decoder (include/dmm_match.h (12)).
// Reference: dmm/modules/base.py:115-188 (RSISMask.forward), dmm/modules/clstm.py:80-131 (ConvLSTMCellMask.forward),
// dmm/modules/evaluator.py:179-212 (the per-object loop of inference_timestep).
//
// Four streaming / pointwise kernels, plain C++ (fp32 arithmetic; the cell, the upsample and the finish are templates over
// the storage type of the activations, fp32 or bf16: include/dmm_match.h (12i)-(12k)): the mask pyramid (nested ceil-mode 2x2 max pools as clipped
// 2^k windows, all levels and objects in one pass over the image-size planes), the fused LSTM cell (the three
// evaluations of a level share one pre-activation; each mask plane's share is a 36-weight stencil per hidden channel),
// the align-corners bilinear upsample written into a channel range of the next level's convolution input, and the
// finish (upsample to image size, sigmoid, the valid-gated history write and the zero rows of the padded output).
// For training on the fused form: the backward of the cell (12e), which recomputes the gates, and its fixed-order fold; and
// what the refine step of training (dmm/modules/trainer.py:236-306) runs around the decoder: the backward of the pyramid (12f),
// the backward of the upsample in 'write' mode (12g), the trainer's nearest / sigmoid / pad finish and its backward (12h).
// The backward of the cell, of the upsample and the trainer's finish are templates over the activations' storage type as well:
// their bf16 instantiations are (12l)-(12o), the bf16 training form.  The pyramid and its backward are fp32 only.
#include "dmm_common.h"

#include <math.h>

namespace dmm {

// ---- (12a) mask pyramid ------------------------------------------------------------------------------------------
// One workgroup = one 32 x 32 tile of one plane (video b, object t, source c): 256 lanes x one 16-byte load (rows are
// only 4-byte aligned: float4u).  Lane l holds row l / 8, columns 4 * (l % 8) .. + 3 of the tile: its 4-wide maximum,
// folded over the 4 rows of a 4 x 4 window by two lane exchanges (lanes l ^ 8, l ^ 16 -- one wave holds 8 rows), over
// the 8 x 8 window by two more (l ^ 32, l ^ 1); the 16 x 16 and 32 x 32 windows combine the four waves through 16
// floats of LDS.  Pixels outside the plane count as -inf (the clipped window of a ceil-mode pool without padding).
__device__ __forceinline__ float fmax2(float a, float b) { return a > b ? a : b; }

__global__ __launch_bounds__(256) void mask_pyramid_kernel(
    const float *__restrict__ prev, const float *__restrict__ ymask, const float *__restrict__ init, int64_t sb_prev,
    int64_t so_prev, int64_t sb_y, int64_t so_y, int64_t sb_i, int64_t so_i, int B, int H, int W, int tiles_x,
    float *__restrict__ out5, float *__restrict__ out4, float *__restrict__ out3, float *__restrict__ out2) {
    __shared__ float s8[16];
    const int plane = blockIdx.y;                      // (t * B + b) * 3 + c : the layout of the outputs
    const int c = plane % 3, tb = plane / 3, b = tb % B, t = tb / B;
    const float *src = c == 0 ? prev + (int64_t)b * sb_prev + (int64_t)t * so_prev
                     : c == 1 ? ymask + (int64_t)b * sb_y + (int64_t)t * so_y
                              : init + (int64_t)b * sb_i + (int64_t)t * so_i;
    const int ty = blockIdx.x / tiles_x, tx = blockIdx.x - ty * tiles_x;
    const int l = threadIdx.x;
    const int row = ty * 32 + (l >> 3), col = tx * 32 + 4 * (l & 7);
    const float ninf = -INFINITY;
    float m = ninf;
    if (row < H && col < W) {
        const float *p = src + (int64_t)row * W + col;
        if (col + 3 < W) {
            const float4u v = __builtin_nontemporal_load(reinterpret_cast<const float4u *>(p));
            m = fmax2(fmax2(v.x, v.y), fmax2(v.z, v.w));
        } else {
            for (int k = 0; col + k < W; ++k) m = fmax2(m, p[k]);
        }
    }
    const int h2 = (H + 3) >> 2, w2 = (W + 3) >> 2, h3 = (H + 7) >> 3, w3 = (W + 7) >> 3;
    const int h4 = (H + 15) >> 4, w4 = (W + 15) >> 4, h5 = (H + 31) >> 5, w5 = (W + 31) >> 5;
    // 4 x 4 windows: rows l>>3 = 4r .. 4r+3 of this wave
    m = fmax2(m, __shfl_xor(m, 8));
    m = fmax2(m, __shfl_xor(m, 16));
    if ((l & 24) == 0) {                               // lanes of window-row 2 * wave (l < 8) and 2 * wave + 1 (32 <= l < 40)
        const int y = ty * 8 + (l >> 5), x = tx * 8 + (l & 7);
        if (y < h2 && x < w2) out2[((int64_t)plane * h2 + y) * w2 + x] = m;
    }
    // 8 x 8 windows: the wave's two window-rows, two neighbouring columns
    m = fmax2(m, __shfl_xor(m, 32));
    m = fmax2(m, __shfl_xor(m, 1));
    const int wave = l >> 6, ll = l & 63;
    if ((ll & 57) == 0) {                              // ll in {0, 2, 4, 6}
        const int y = ty * 4 + wave, x = tx * 4 + (ll >> 1);
        if (y < h3 && x < w3) out3[((int64_t)plane * h3 + y) * w3 + x] = m;
        s8[wave * 4 + (ll >> 1)] = m;
    }
    __syncthreads();
    if (l < 4) {                                       // 16 x 16 windows (2 x 2 of them)
        const int r = l >> 1, q = l & 1;
        const float a = fmax2(fmax2(s8[(2 * r) * 4 + 2 * q], s8[(2 * r) * 4 + 2 * q + 1]),
                              fmax2(s8[(2 * r + 1) * 4 + 2 * q], s8[(2 * r + 1) * 4 + 2 * q + 1]));
        const int y = ty * 2 + r, x = tx * 2 + q;
        if (y < h4 && x < w4) out4[((int64_t)plane * h4 + y) * w4 + x] = a;
    }
    if (l == 0) {                                      // the 32 x 32 window (the tile starts inside the plane)
        float a = s8[0];
#pragma unroll
        for (int k = 1; k < 16; ++k) a = fmax2(a, s8[k]);
        if (ty < h5 && tx < w5) out5[((int64_t)plane * h5 + ty) * w5 + tx] = a;
    }
}

// ---- storage of the activations (the convolutions' inputs and outputs): fp32, or bf16 for (12i)-(12k) -----------------------
// A value is widened on load (exact) and rounded ONCE, to nearest even, at the store (torch's rule: a NaN becomes 0x7FC0), so
// a bf16 instantiation gives its fp32 twin's result on the widened inputs, rounded.  A lane owns one position: 2-byte loads
// and stores, coalesced over the wave like the dwords of the fp32 form, and right for every alignment a bf16 tensor can have.
__device__ __forceinline__ float act_load(const float *p) { return *p; }
__device__ __forceinline__ float act_load(const bf16_t *p) { return MaskIO<bf16_t>::load1(p); }
__device__ __forceinline__ void act_store(float *p, float v) { *p = v; }
__device__ __forceinline__ void act_store(bf16_t *p, float v) {
    const uint32_t u = __float_as_uint(v);
    p->v = v != v ? (uint16_t)0x7FC0u : (uint16_t)((u + 0x7FFFu + ((u >> 16) & 1u)) >> 16);
}

// ---- (12b) / (12i) fused LSTM cell ---------------------------------------------------------------------------------
// A lane owns one position (b, y, x) and CH consecutive hidden channels: the 27 stencil inputs (3 planes x 3 x 3,
// zero padded) are loaded once, the 36 weights of a channel are wave-uniform, every gate / state access is coalesced
// over the positions.  T: the storage of the pre-activation's addends and of the hidden (both copies); the mask planes, the
// stencil and the cell state are fp32 in either form.
constexpr int kGateCh = 4;

__device__ __forceinline__ float sigmoid_f32(float x) { return 1.0f / (1.0f + expf(-x)); }

template <typename T>
__global__ __launch_bounds__(256) void clstm_gates_kernel(
    const T *__restrict__ pre0, const T *__restrict__ pre1, const T *__restrict__ pre2, int64_t sb0, int64_t sb1,
    int64_t sb2, const float *__restrict__ masks, int64_t sb_m, const float *__restrict__ wm, const float *__restrict__ c_prev,
    int B, int Hd, int h, int w, T *__restrict__ hidden, float *__restrict__ cell, T *__restrict__ hidden2,
    int64_t sb_h2) {
    const int hw = h * w;
    const int pos = blockIdx.x * 256 + threadIdx.x;
    if (pos >= B * hw) return;
    const int b = pos / hw, p = pos - b * hw, y = p / w, x = p - y * w;
    float mk[3][9];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const float *mp = masks + (int64_t)b * sb_m + (int64_t)k * hw;
#pragma unroll
        for (int dy = 0; dy < 3; ++dy)
#pragma unroll
            for (int dx = 0; dx < 3; ++dx) {
                const int yy = y + dy - 1, xx = x + dx - 1;
                mk[k][dy * 3 + dx] = (yy >= 0 && yy < h && xx >= 0 && xx < w) ? mp[yy * w + xx] : 0.0f;
            }
    }
    const int ch0 = blockIdx.y * kGateCh;
    for (int ch = ch0; ch < ch0 + kGateCh && ch < Hd; ++ch) {
        float g[4];                                    // in, remember, out, cell: the reference's chunk(4, 1)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int64_t off = (int64_t)(q * Hd + ch) * hw + p;
            float v = act_load(pre0 + (int64_t)b * sb0 + off);
            if (pre1) v = v + act_load(pre1 + (int64_t)b * sb1 + off);
            if (pre2) v = v + act_load(pre2 + (int64_t)b * sb2 + off);
            g[q] = v;
        }
        const int64_t so = ((int64_t)b * Hd + ch) * hw + p;
        const float cp = c_prev ? c_prev[so] : 0.0f;
        float hk[3], ck[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            float s[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const float *wq = wm + (int64_t)(q * Hd + ch) * 9;
                float a = 0.0f;
#pragma unroll
                for (int j = 0; j < 9; ++j) a = __builtin_fmaf(wq[j], mk[k][j], a);
                s[q] = g[q] + a;
            }
            const float gi = sigmoid_f32(s[0]), gr = sigmoid_f32(s[1]), go = sigmoid_f32(s[2]), gc = tanhf(s[3]);
            ck[k] = (gr * cp) + (gi * gc);
            hk[k] = go * tanhf(ck[k]);
        }
        // the reference's order: prev_mask (plane 0), init_pred (plane 2), y_mask (plane 1); (a + b + c) / 3
        const float hv = ((hk[0] + hk[2]) + hk[1]) / 3.0f;
        const float cv = ((ck[0] + ck[2]) + ck[1]) / 3.0f;
        act_store(hidden + so, hv);
        cell[so] = cv;
        if (hidden2) act_store(hidden2 + (int64_t)b * sb_h2 + (int64_t)ch * hw + p, hv);
    }
}

// ---- (12e) backward of the fused LSTM cell -----------------------------------------------------------------------------
// The forward's geometry: a lane owns one position and the kGateCh channels of its group.  Nothing of the forward is saved:
// the gates are recomputed with the forward's expressions in the forward's order.  ds[e][q] is the gradient of the gate
// pre-activation q of evaluation e = 0, 1, 2 (mask planes 0, 2, 1).  d_pre and d_cell_prev are per lane.  The two reductions
// go through the workspace and are folded in a fixed order by clstm_gates_bwd_fold_kernel (no atomics):
//   d_masks   each lane leaves its 27 tap sums  tap[k][j] = sum over (q, channels of the group) ds_{q,k} * w_mask[q, ch, j]
//             in ws_m [groups][B][3][9][h * w]; the fold gathers them from the nine source positions, groups ascending;
//   d_w_mask  36 sums per channel over the workgroup's 256 positions (planes in evaluation order inside the lane, the
//             64-lane tree of wave_sum_rows, the four waves in order through LDS) go to ws_w [position blocks][4 * Hd * 9];
//             the fold adds the position blocks in ascending order.
// Lanes past the last position hold ds = 0 and take part in the wave sums.  T: the storage of the addends, of d_hidden and of
// d_pre (12l), as in the forward; the gradient arithmetic, the tap sums and both reductions are fp32 in either form, so the
// fold kernel is shared.
__device__ __forceinline__ int eval_plane(int e) { return e == 0 ? 0 : (e == 1 ? 2 : 1); }

template <typename T, bool WANT_M, bool WANT_W>
__global__ __launch_bounds__(256) void clstm_gates_bwd_kernel(
    const T *__restrict__ pre0, const T *__restrict__ pre1, const T *__restrict__ pre2, int64_t sb0, int64_t sb1,
    int64_t sb2, const float *__restrict__ masks, int64_t sb_m, const float *__restrict__ wm, const float *__restrict__ c_prev,
    const T *__restrict__ d_hidden, const float *__restrict__ d_cell, int B, int Hd, int h, int w,
    T *__restrict__ d_pre, float *__restrict__ d_cprev, float *__restrict__ ws_m, float *__restrict__ ws_w) {
    __shared__ float s_w[WANT_W ? kGateCh * 4 * 36 : 1];
    __shared__ float s_wm[kGateCh * 36];               // the group's stencil weights: read as vector operands (36 wave-uniform
    const int hw = h * w;                              // scalars per channel, on top of twelve pointers, do not fit the SGPRs)
    const int ch0 = blockIdx.y * kGateCh;
    if (threadIdx.x < kGateCh * 36) {
        const int c = threadIdx.x / 36, i = threadIdx.x - c * 36;
        s_wm[threadIdx.x] = ch0 + c < Hd ? wm[(int64_t)((i / 9) * Hd + ch0 + c) * 9 + (i % 9)] : 0.0f;
    }
    __syncthreads();
    const int pos = blockIdx.x * 256 + threadIdx.x;
    const bool valid = pos < B * hw;
    const int b = valid ? pos / hw : 0, p = valid ? pos - b * hw : 0, y = p / w, x = p - y * w;
    float mk[3][9];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const float *mp = masks + (int64_t)b * sb_m + (int64_t)k * hw;
#pragma unroll
        for (int dy = 0; dy < 3; ++dy)
#pragma unroll
            for (int dx = 0; dx < 3; ++dx) {
                const int yy = y + dy - 1, xx = x + dx - 1;
                mk[k][dy * 3 + dx] = (valid && yy >= 0 && yy < h && xx >= 0 && xx < w) ? mp[yy * w + xx] : 0.0f;
            }
    }
    float tap[3][9];
#pragma unroll
    for (int k = 0; k < 3; ++k)
#pragma unroll
        for (int j = 0; j < 9; ++j) tap[k][j] = 0.0f;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int c = 0; c < kGateCh && ch0 + c < Hd; ++c) {
        const int ch = ch0 + c;
        float ds[3][4];
#pragma unroll
        for (int e = 0; e < 3; ++e)
#pragma unroll
            for (int q = 0; q < 4; ++q) ds[e][q] = 0.0f;
        if (valid) {
            float g[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int64_t off = (int64_t)(q * Hd + ch) * hw + p;
                float v = act_load(pre0 + (int64_t)b * sb0 + off);
                if (pre1) v = v + act_load(pre1 + (int64_t)b * sb1 + off);
                if (pre2) v = v + act_load(pre2 + (int64_t)b * sb2 + off);
                g[q] = v;
            }
            const int64_t so = ((int64_t)b * Hd + ch) * hw + p;
            const float cp = c_prev ? c_prev[so] : 0.0f;
            const float u = d_hidden ? act_load(d_hidden + so) / 3.0f : 0.0f;
            const float v = d_cell ? d_cell[so] / 3.0f : 0.0f;
            float dcr[3];
#pragma unroll
            for (int e = 0; e < 3; ++e) {
                const int k = eval_plane(e);
                float s[4];
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const float *wq = s_wm + c * 36 + q * 9;
                    float a = 0.0f;
#pragma unroll
                    for (int j = 0; j < 9; ++j) a = __builtin_fmaf(wq[j], mk[k][j], a);
                    s[q] = g[q] + a;
                }
                const float gi = sigmoid_f32(s[0]), gr = sigmoid_f32(s[1]), go = sigmoid_f32(s[2]), gc = tanhf(s[3]);
                const float ck = (gr * cp) + (gi * gc);
                const float tk = tanhf(ck);
                const float dc = v + (u * go) * (1.0f - tk * tk);
                ds[e][0] = ((dc * gc) * gi) * (1.0f - gi);
                ds[e][1] = c_prev ? ((dc * cp) * gr) * (1.0f - gr) : 0.0f;
                ds[e][2] = ((u * tk) * go) * (1.0f - go);
                ds[e][3] = (dc * gi) * (1.0f - gc * gc);
                dcr[e] = dc * gr;
            }
#pragma unroll
            for (int q = 0; q < 4; ++q)
                act_store(d_pre + ((int64_t)b * 4 * Hd + (int64_t)(q * Hd + ch)) * hw + p, (ds[0][q] + ds[1][q]) + ds[2][q]);
            if (d_cprev) d_cprev[so] = (dcr[0] + dcr[1]) + dcr[2];
        }
        if (WANT_M) {
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const float *wq = s_wm + c * 36 + q * 9;
#pragma unroll
                for (int e = 0; e < 3; ++e)
#pragma unroll
                    for (int j = 0; j < 9; ++j) tap[eval_plane(e)][j] = __builtin_fmaf(ds[e][q], wq[j], tap[eval_plane(e)][j]);
            }
        }
        if (WANT_W) {
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                float r[9];
#pragma unroll
                for (int j = 0; j < 9; ++j) {
                    float a = ds[0][q] * mk[0][j];
                    a = __builtin_fmaf(ds[1][q], mk[2][j], a);
                    r[j] = __builtin_fmaf(ds[2][q], mk[1][j], a);
                }
                wave_sum_rows<9>(r);
                if (lane == 0) {
#pragma unroll
                    for (int j = 0; j < 9; ++j) s_w[(c * 4 + wave) * 36 + q * 9 + j] = r[j];
                }
            }
        }
    }
    if (WANT_M && valid) {
        float *t = ws_m + ((int64_t)blockIdx.y * B + b) * 27 * hw + p;
#pragma unroll
        for (int k = 0; k < 3; ++k)
#pragma unroll
            for (int j = 0; j < 9; ++j) t[(int64_t)(k * 9 + j) * hw] = tap[k][j];
    }
    if (WANT_W) {
        __syncthreads();
        const int c = threadIdx.x / 36, i = threadIdx.x - c * 36;
        if (c < kGateCh && ch0 + c < Hd) {
            const float *sp = s_w + c * 4 * 36 + i;
            const float a = ((sp[0] + sp[36]) + sp[72]) + sp[108];
            ws_w[(int64_t)blockIdx.x * 36 * Hd + (int64_t)((i / 9) * Hd + ch0 + c) * 9 + (i % 9)] = a;
        }
    }
}

// Workgroups 0 .. blocks_m - 1: one lane per element of d_masks; the rest: one lane per element of d_w_mask.
__global__ __launch_bounds__(256) void clstm_gates_bwd_fold_kernel(const float *__restrict__ ws_m, const float *__restrict__ ws_w,
                                                                   int B, int Hd, int h, int w, int groups, int pos_blocks,
                                                                   unsigned blocks_m, float *__restrict__ d_masks,
                                                                   float *__restrict__ d_wm) {
    const int hw = h * w;
    if (blockIdx.x < blocks_m) {
        const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
        if (i >= (int64_t)B * 3 * hw) return;
        const int p = (int)(i % hw), y = p / w, x = p - y * w;
        const int64_t bk = i / hw;                     // b * 3 + k
        // tap j's source position; a tap whose source lies outside the plane reads the lane's own position and counts as 0,
        // so the loads of a group do not hang on a branch and the next group's are issued under this group's adds
        int off[9];
        bool in[9];
#pragma unroll
        for (int j = 0; j < 9; ++j) {
            const int yy = y - j / 3 + 1, xx = x - j % 3 + 1;
            in[j] = yy >= 0 && yy < h && xx >= 0 && xx < w;
            off[j] = j * hw + (in[j] ? yy * w + xx : p);
        }
        float acc = 0.0f;
#pragma unroll 2
        for (int g = 0; g < groups; ++g) {
            const float *t = ws_m + (((int64_t)g * B * 3 + bk) * 9) * hw;
            float v[9];
#pragma unroll
            for (int j = 0; j < 9; ++j) v[j] = t[off[j]];
#pragma unroll
            for (int j = 0; j < 9; ++j) acc = acc + (in[j] ? v[j] : 0.0f);
        }
        d_masks[i] = acc;
    } else {
        const int i = (int)(blockIdx.x - blocks_m) * 256 + threadIdx.x;
        const int n = 36 * Hd;
        if (i >= n) return;
        float acc = 0.0f;
        int k = 0;
        for (; k + 8 <= pos_blocks; k += 8) {          // eight loads in flight, added in ascending order
            float v[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) v[j] = ws_w[(int64_t)(k + j) * n + i];
#pragma unroll
            for (int j = 0; j < 8; ++j) acc = acc + v[j];
        }
        for (; k < pos_blocks; ++k) acc = acc + ws_w[(int64_t)k * n + i];
        d_wm[i] = acc;
    }
}

// ---- (12c) / (12d), (12j) / (12k) align-corners bilinear ---------------------------------------------------------------
// ATen's upsample_bilinear2d with align_corners = True: scale = (in - 1) / (out - 1) (0 for out == 1), src = scale * dst,
// lower index by truncation, lambda1 = src - lower, lambda0 = 1 - lambda1.
struct Lerp { int i0, step; float l0, l1; };
__device__ __forceinline__ Lerp lerp_of(int dst, float scale, int in) {
    const float s = scale * (float)dst;
    Lerp r;
    r.i0 = (int)s;
    if (r.i0 > in - 1) r.i0 = in - 1;                  // (never taken for exact arithmetic; keeps every read in bounds)
    r.step = r.i0 < in - 1 ? 1 : 0;
    r.l1 = s - (float)r.i0;
    r.l0 = 1.0f - r.l1;
    return r;
}
template <typename T>
__device__ __forceinline__ float bilerp(const T *__restrict__ p, int w, const Lerp &ly, const Lerp &lx) {
    const T *r0 = p + (int64_t)ly.i0 * w + lx.i0, *r1 = r0 + (int64_t)ly.step * w;
    return ly.l0 * (lx.l0 * act_load(r0) + lx.l1 * act_load(r0 + lx.step)) +
           ly.l1 * (lx.l0 * act_load(r1) + lx.l1 * act_load(r1 + lx.step));
}
__host__ __device__ __forceinline__ float ac_scale(int in, int out) { return out > 1 ? (float)(in - 1) / (float)(out - 1) : 0.0f; }

template <int MODE, typename T>   // 0 write, 1 add, 2 mul; T: the storage of src and dst
__global__ __launch_bounds__(256) void upsample_into_kernel(const T *__restrict__ src, int64_t sb_src, int C, int h, int w,
                                                            T *__restrict__ dst, int64_t sb_dst, int c0, int H, int W,
                                                            float sy, float sx, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int X = (int)(i % W);
    int64_t r = i / W;
    const int Y = (int)(r % H);
    r /= H;
    const int c = (int)(r % C), b = (int)(r / C);
    const float v = bilerp(src + (int64_t)b * sb_src + (int64_t)c * h * w, w, lerp_of(Y, sy, h), lerp_of(X, sx, w));
    T *d = dst + (int64_t)b * sb_dst + ((int64_t)(c0 + c) * H + Y) * W + X;
    if (MODE == 0) act_store(d, v);
    else if (MODE == 1) act_store(d, act_load(d) + v);
    else act_store(d, act_load(d) * v);
}

// One lane = 4 consecutive pixels of a row of outs[b, t] (rows are 4-byte aligned: float4u stores).  T: the storage of the
// logits, which are gathered element by element; outs and hist are fp32 in either form.
template <typename T>
__global__ __launch_bounds__(256) void refine_finish_kernel(const T *__restrict__ logits, int64_t sb_l, int64_t so_l, int h,
                                                            int w, const int *__restrict__ valid, int B, int O, int n_obj, int H,
                                                            int W, int Wq, float sy, float sx, float *__restrict__ outs,
                                                            float *__restrict__ hist, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int X = 4 * (int)(i % Wq);
    int64_t r = i / Wq;
    const int Y = (int)(r % H);
    r /= H;
    const int t = (int)(r % O), b = (int)(r / O);
    const int64_t o = (((int64_t)b * O + t) * H + Y) * W + X;
    float v[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    const bool live = t < n_obj;
    if (live) {
        const T *p = logits + (int64_t)b * sb_l + (int64_t)t * so_l;
        const Lerp ly = lerp_of(Y, sy, h);
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (X + k < W) v[k] = sigmoid_f32(bilerp(p, w, ly, lerp_of(X + k, sx, w)));
    }
    const bool keep = live && hist && valid[b * O + t] != 0;
    if (X + 3 < W) {
        float4u q;
        q.x = v[0]; q.y = v[1]; q.z = v[2]; q.w = v[3];
        __builtin_nontemporal_store(q, reinterpret_cast<float4u *>(outs + o));
        if (keep) __builtin_nontemporal_store(q, reinterpret_cast<float4u *>(hist + o));
    } else {
        for (int k = 0; X + k < W; ++k) {
            outs[o + k] = v[k];
            if (keep) hist[o + k] = v[k];
        }
    }
}

// ---- (12f) backward of the mask pyramid -------------------------------------------------------------------------------
// One workgroup = one 32 x 32 tile of one wanted plane (video b, object t, prev_mask or init_pred), as in the forward.  The
// chain of 2x2 pools is replayed on (value, position) pairs in LDS: 16 x 16 winners of the first pool, then 8 x 8, 4 x 4,
// 2 x 2 and 1 (the outputs' levels 2 .. 5).  Every pool scans its four children in row-major order and replaces the winner
// on a strict '>' only -- ATen's rule, so among equal maxima of a composite window the smallest Z-order code wins.  Pixels
// outside the plane count as -inf and never win (inputs are finite; the tile's first pixel lies inside the plane).  The
// gradients then descend into an LDS tile of 1024 floats, level 2, 3, 4, 5 in this order, a barrier between two levels
// (windows of one level are disjoint, so no two lanes meet), and the whole tile is stored: every pixel is written.
__device__ __forceinline__ void pool_winner(const float *__restrict__ cv, const short *__restrict__ cp, int n, int i,
                                            float *__restrict__ pv, short *__restrict__ pp) {
    const int half = n >> 1, py = i / half, px = i - py * half;
    const int c = (2 * py) * n + 2 * px;
    float v = cv[c];
    short p = cp[c];
    if (cv[c + 1] > v) { v = cv[c + 1]; p = cp[c + 1]; }
    if (cv[c + n] > v) { v = cv[c + n]; p = cp[c + n]; }
    if (cv[c + n + 1] > v) { v = cv[c + n + 1]; p = cp[c + n + 1]; }
    pv[i] = v;
    pp[i] = p;
}

__global__ __launch_bounds__(256) void mask_pyramid_bwd_kernel(
    const float *__restrict__ prev, const float *__restrict__ init, int64_t sb_prev, int64_t so_prev, int64_t sb_i, int64_t so_i,
    int B, int H, int W, int tiles_x, const float *__restrict__ d5, const float *__restrict__ d4, const float *__restrict__ d3,
    const float *__restrict__ d2, float *__restrict__ d_prev, int64_t sb_dp, int64_t so_dp, float *__restrict__ d_init,
    int64_t sb_di, int64_t so_di) {
    __shared__ float s_v[1024];                        // the tile's values, then its gradients
    __shared__ float v1[256], v2[64], v3[16], v4[4], v5[1];
    __shared__ short p1[256], p2[64], p3[16], p4[4], p5[1];
    const int wanted = (d_prev ? 1 : 0) + (d_init ? 1 : 0);
    const int which = blockIdx.y % wanted, tb = blockIdx.y / wanted, b = tb % B, t = tb / B;
    const bool is_prev = d_prev && which == 0;
    const float *src = is_prev ? prev + (int64_t)b * sb_prev + (int64_t)t * so_prev : init + (int64_t)b * sb_i + (int64_t)t * so_i;
    float *dst = is_prev ? d_prev + (int64_t)b * sb_dp + (int64_t)t * so_dp : d_init + (int64_t)b * sb_di + (int64_t)t * so_di;
    const int c = is_prev ? 0 : 2;                     // the plane's channel in the forward's outputs
    const int64_t plane = ((int64_t)t * B + b) * 3 + c;
    const int ty = blockIdx.x / tiles_x, tx = blockIdx.x - ty * tiles_x;
    const int l = threadIdx.x;
    const int y0 = ty * 32, x0 = tx * 32;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int i = k * 256 + l, row = y0 + (i >> 5), col = x0 + (i & 31);
        s_v[i] = (row < H && col < W) ? src[(int64_t)row * W + col] : -INFINITY;
    }
    __syncthreads();
    {                                                  // the first pool: 2 x 2 pixels, positions = indices into the tile
        const int py = l >> 4, px = l & 15, q = (2 * py) * 32 + 2 * px;
        float v = s_v[q];
        int p = q;
        if (s_v[q + 1] > v) { v = s_v[q + 1]; p = q + 1; }
        if (s_v[q + 32] > v) { v = s_v[q + 32]; p = q + 32; }
        if (s_v[q + 33] > v) { v = s_v[q + 33]; p = q + 33; }
        v1[l] = v;
        p1[l] = (short)p;
    }
    __syncthreads();
    if (l < 64) pool_winner(v1, p1, 16, l, v2, p2);
    __syncthreads();
    if (l < 16) pool_winner(v2, p2, 8, l, v3, p3);
    __syncthreads();
    if (l < 4) pool_winner(v3, p3, 4, l, v4, p4);
    __syncthreads();
    if (l == 0) pool_winner(v4, p4, 2, 0, v5, p5);
#pragma unroll
    for (int k = 0; k < 4; ++k) s_v[k * 256 + l] = 0.0f;   // (the values were last read by the first pool)
    __syncthreads();
    const int h2 = (H + 3) >> 2, w2 = (W + 3) >> 2, h3 = (H + 7) >> 3, w3 = (W + 7) >> 3;
    const int h4 = (H + 15) >> 4, w4 = (W + 15) >> 4, h5 = (H + 31) >> 5, w5 = (W + 31) >> 5;
    if (d2 && l < 64) {
        const int y = ty * 8 + (l >> 3), x = tx * 8 + (l & 7);
        if (y < h2 && x < w2) s_v[p2[l]] = s_v[p2[l]] + d2[(plane * h2 + y) * w2 + x];
    }
    __syncthreads();
    if (d3 && l < 16) {
        const int y = ty * 4 + (l >> 2), x = tx * 4 + (l & 3);
        if (y < h3 && x < w3) s_v[p3[l]] = s_v[p3[l]] + d3[(plane * h3 + y) * w3 + x];
    }
    __syncthreads();
    if (d4 && l < 4) {
        const int y = ty * 2 + (l >> 1), x = tx * 2 + (l & 1);
        if (y < h4 && x < w4) s_v[p4[l]] = s_v[p4[l]] + d4[(plane * h4 + y) * w4 + x];
    }
    __syncthreads();
    if (d5 && l == 0 && ty < h5 && tx < w5) s_v[p5[0]] = s_v[p5[0]] + d5[(plane * h5 + ty) * w5 + tx];
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int i = k * 256 + l, row = y0 + (i >> 5), col = x0 + (i & 31);
        if (row < H && col < W) dst[(int64_t)row * W + col] = s_v[i];
    }
}

// ---- (12g) backward of the bilinear upsample ('write' mode) ------------------------------------------------------------
// Gather form: one lane per source element.  The destination rows (columns) whose lerp_of can touch source row y lie in
// [(y - 1) / scale, (y + 1) / scale); that range is widened by one and clipped, and every candidate is then classified with
// the forward's own lerp_of, so the indices and weights are the forward's, bit for bit.  Y ascending, then X ascending.
__device__ __forceinline__ void touch_range(int i, float scale, int out, int &lo, int &hi) {
    lo = 0;
    hi = out - 1;
    if (scale > 0.0f) {                                // (scale == 0: in == 1, every destination index reads source 0)
        const float a = floorf((float)(i - 1) / scale) - 1.0f, b = ceilf((float)(i + 1) / scale) + 1.0f;
        if (a > 0.0f) lo = a < (float)(out - 1) ? (int)a : out - 1;
        if (b < (float)(out - 1)) hi = b > 0.0f ? (int)b : 0;
    }
}
__device__ __forceinline__ float touch_weight(const Lerp &r, int i) {
    float wgt = r.i0 == i ? r.l0 : 0.0f;
    if (r.i0 + r.step == i) wgt = r.i0 == i ? wgt + r.l1 : r.l1;   // (step == 0: the forward reads the row twice)
    return wgt;
}

template <typename T>   // the storage of d_dst and d_src (12m): the gather accumulates in fp32 and rounds once, at the store
__global__ __launch_bounds__(256) void upsample_bwd_kernel(const T *__restrict__ d_dst, int64_t sb_dst, int C, int H, int W,
                                                           int c0, T *__restrict__ d_src, int64_t sb_src, int h, int w,
                                                           float sy, float sx, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int x = (int)(i % w);
    int64_t r = i / w;
    const int y = (int)(r % h);
    r /= h;
    const int c = (int)(r % C), b = (int)(r / C);
    int Y0, Y1, X0, X1;
    touch_range(y, sy, H, Y0, Y1);
    touch_range(x, sx, W, X0, X1);
    const T *g = d_dst + (int64_t)b * sb_dst + (int64_t)(c0 + c) * H * W;
    float acc = 0.0f;
    for (int Y = Y0; Y <= Y1; ++Y) {
        const Lerp ly = lerp_of(Y, sy, h);
        if (ly.i0 != y && ly.i0 + ly.step != y) continue;
        const float wy = touch_weight(ly, y);
        const T *row = g + (int64_t)Y * W;
        for (int X = X0; X <= X1; ++X) {
            const Lerp lx = lerp_of(X, sx, w);
            if (lx.i0 != x && lx.i0 + lx.step != x) continue;
            acc = acc + (wy * touch_weight(lx, x)) * act_load(row + X);
        }
    }
    act_store(d_src + (int64_t)b * sb_src + ((int64_t)c * h + y) * w + x, acc);
}

// ---- (12h) the finish of the training step -------------------------------------------------------------------------------
// torch's default NEAREST interpolation: source index = min((int)floorf(dst * scale), in - 1), scale = (float)in / out.
__host__ __device__ __forceinline__ float nn_scale(int in, int out) { return (float)in / (float)out; }
__device__ __forceinline__ int nn_index(int dst, float scale, int in) {
    const int i = (int)floorf((float)dst * scale);
    return i < in - 1 ? i : in - 1;
}

template <typename T>   // the storage of the logits (12n); outs is fp32 in either form
__global__ __launch_bounds__(256) void refine_train_finish_kernel(const T *__restrict__ logits, int64_t sb_l, int64_t so_l,
                                                                  int h, int w, int O, int n_obj, int H, int W, float sy, float sx,
                                                                  float *__restrict__ outs, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int X = (int)(i % W);
    int64_t r = i / W;
    const int Y = (int)(r % H);
    r /= H;
    const int t = (int)(r % O), b = (int)(r / O);
    float v = 0.0f;
    if (t < n_obj) {
        const T *p = logits + (int64_t)b * sb_l + (int64_t)t * so_l;
        v = sigmoid_f32(act_load(p + (int64_t)nn_index(Y, sy, h) * w + nn_index(X, sx, w)));
    }
    outs[i] = v;
}

// The destination indices that read source index i form a contiguous block inside [i * out / in - 1, (i + 1) * out / in + 1]
// (integer arithmetic, one index of room each way); the block is found by classifying with nn_index itself.
__device__ __forceinline__ void nn_block(int i, float scale, int in, int out, int &lo, int &hi) {
    int64_t a = ((int64_t)i * out) / in - 1, z = ((int64_t)(i + 1) * out + in - 1) / in + 1;
    if (a < 0) a = 0;
    if (z > out - 1) z = out - 1;
    lo = (int)a;
    hi = (int)z;
    while (lo <= hi && nn_index(lo, scale, in) != i) ++lo;
    while (hi >= lo && nn_index(hi, scale, in) != i) --hi;
}

template <typename T>   // the storage of the logits and of d_logits (12o); d_outs is fp32, the block sum and the product too
__global__ __launch_bounds__(256) void refine_train_finish_bwd_kernel(const T *__restrict__ logits, int64_t sb_l, int64_t so_l,
                                                                      int h, int w, const float *__restrict__ d_outs, int O,
                                                                      int n_obj, int H, int W, float sy, float sx,
                                                                      T *__restrict__ d_logits, int64_t sb_d, int64_t so_d,
                                                                      int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int x = (int)(i % w);
    int64_t r = i / w;
    const int y = (int)(r % h);
    r /= h;
    const int t = (int)(r % n_obj), b = (int)(r / n_obj);
    int Y0, Y1, X0, X1;
    nn_block(y, sy, h, H, Y0, Y1);
    nn_block(x, sx, w, W, X0, X1);
    const float *g = d_outs + ((int64_t)b * O + t) * H * W;
    float acc = 0.0f;
    for (int Y = Y0; Y <= Y1; ++Y)
        for (int X = X0; X <= X1; ++X) acc = acc + g[(int64_t)Y * W + X];
    const float p = sigmoid_f32(act_load(logits + (int64_t)b * sb_l + (int64_t)t * so_l + (int64_t)y * w + x));
    act_store(d_logits + (int64_t)b * sb_d + (int64_t)t * so_d + (int64_t)y * w + x, (p * (1.0f - p)) * acc);
}

// ---- the entries of the three templated kernels: one check and one launch for both storage types --------------------------
template <typename T>
static int clstm_gates_entry(const T *pre0, const T *pre1, const T *pre2, int64_t sb0, int64_t sb1, int64_t sb2, const float *masks,
                             int64_t sb_masks, const float *w_mask, const float *cell_prev, int B, int hidden_size, int h, int w,
                             T *hidden, float *cell, T *hidden_copy, int64_t sb_copy, dmm_stream_t stream) {
    if (B < 0 || hidden_size <= 0 || h <= 0 || w <= 0) return DMM_ERR_BAD_ARG;
    if (B == 0) return DMM_OK;
    if (!pre0 || !masks || !w_mask || !hidden || !cell) return DMM_ERR_BAD_ARG;
    const int64_t hw = (int64_t)h * w;
    if (sb0 < 0 || sb1 < 0 || sb2 < 0 || sb_masks < 3 * hw || (hidden_copy && sb_copy < (int64_t)hidden_size * hw))
        return DMM_ERR_BAD_ARG;
    const int64_t blocks = ((int64_t)B * hw + 255) / 256, groups = (hidden_size + kGateCh - 1) / kGateCh;
    if ((int64_t)B * hw > 0x7fffffffLL || groups > 65535) return DMM_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(clstm_gates_kernel<T>, dim3((unsigned)blocks, (unsigned)groups), dim3(256), 0, (hipStream_t)stream, pre0,
                       pre1, pre2, sb0, sb1, sb2, masks, sb_masks, w_mask, cell_prev, B, hidden_size, h, w, hidden, cell,
                       hidden_copy, sb_copy);
    return check_launch();
}

template <typename T>
static int upsample_into_entry(const T *src, int64_t sb_src, int B, int C, int h, int w, T *dst, int64_t sb_dst, int C_dst, int c0,
                               int H, int W, int mode, dmm_stream_t stream) {
    if (B < 0 || C <= 0 || h <= 0 || w <= 0 || H <= 0 || W <= 0 || C_dst <= 0) return DMM_ERR_BAD_ARG;
    if (c0 < 0 || c0 + C > C_dst || mode < 0 || mode > 2) return DMM_ERR_BAD_ARG;   // the channel range lies inside dst
    if (B == 0) return DMM_OK;
    if (!src || !dst) return DMM_ERR_BAD_ARG;
    if (sb_src < (int64_t)C * h * w || sb_dst < (int64_t)C_dst * H * W) return DMM_ERR_BAD_ARG;
    const int64_t n = (int64_t)B * C * H * W, blocks = (n + 255) / 256;
    if (blocks > 0x7fffffffLL) return DMM_ERR_UNSUPPORTED;
    const float sy = ac_scale(h, H), sx = ac_scale(w, W);
#define DMM_UP(MODE_)                                                                                                     \
    hipLaunchKernelGGL((upsample_into_kernel<MODE_, T>), dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, src,    \
                       sb_src, C, h, w, dst, sb_dst, c0, H, W, sy, sx, n)
    if (mode == 0) DMM_UP(0);
    else if (mode == 1) DMM_UP(1);
    else DMM_UP(2);
#undef DMM_UP
    return check_launch();
}

template <typename T>
static int refine_finish_entry(const T *logits, int64_t sb_logits, int64_t so_logits, int h, int w, const int *valid, int B, int O,
                               int n_obj, int H, int W, float *outs, float *mask_hist, dmm_stream_t stream) {
    if (B < 0 || O < 0 || n_obj < 0 || n_obj > O || h <= 0 || w <= 0 || H <= 0 || W <= 0) return DMM_ERR_BAD_ARG;
    if (B == 0 || O == 0) return DMM_OK;
    if (!outs || (n_obj > 0 && !logits) || (mask_hist && !valid)) return DMM_ERR_BAD_ARG;
    if (sb_logits < 0 || so_logits < 0) return DMM_ERR_BAD_ARG;
    const int Wq = (W + 3) / 4;
    const int64_t n = (int64_t)B * O * H * Wq, blocks = (n + 255) / 256;
    if (blocks > 0x7fffffffLL) return DMM_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(refine_finish_kernel<T>, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, logits, sb_logits,
                       so_logits, h, w, valid, B, O, n_obj, H, W, Wq, ac_scale(h, H), ac_scale(w, W), outs, mask_hist, n);
    return check_launch();
}

template <typename T>
static int clstm_gates_bwd_entry(const T *pre0, const T *pre1, const T *pre2, int64_t sb0, int64_t sb1, int64_t sb2,
                                 const float *masks, int64_t sb_masks, const float *w_mask, const float *cell_prev, int B,
                                 int hidden_size, int h, int w, const T *d_hidden, const float *d_cell, T *d_pre,
                                 float *d_cell_prev, float *d_masks, float *d_w_mask, void *ws, size_t ws_bytes,
                                 dmm_stream_t stream) {
    if (B < 0 || hidden_size <= 0 || h <= 0 || w <= 0) return DMM_ERR_BAD_ARG;
    if (B == 0) return DMM_OK;
    if (!pre0 || !masks || !w_mask || !d_pre || (!d_hidden && !d_cell) || (d_cell_prev && !cell_prev)) return DMM_ERR_BAD_ARG;
    const int64_t hw = (int64_t)h * w;
    if (sb0 < 0 || sb1 < 0 || sb2 < 0 || sb_masks < 3 * hw) return DMM_ERR_BAD_ARG;
    const bool reduce = d_masks || d_w_mask;
    if (reduce && !ws) return DMM_ERR_BAD_ARG;
    const int64_t blocks = ((int64_t)B * hw + 255) / 256, groups = (hidden_size + kGateCh - 1) / kGateCh;
    if ((int64_t)B * hw > 0x7fffffffLL || groups > 65535) return DMM_ERR_UNSUPPORTED;
    if (reduce && ws_bytes < dmm_clstm_gates_bwd_workspace_bytes(B, hidden_size, h, w)) return DMM_ERR_WORKSPACE;
    float *ws_m = (float *)ws, *ws_w = reduce ? ws_m + groups * B * 27 * hw : nullptr;
#define DMM_GATES_BWD(M_, W_)                                                                                              \
    hipLaunchKernelGGL((clstm_gates_bwd_kernel<T, M_, W_>), dim3((unsigned)blocks, (unsigned)groups), dim3(256), 0,        \
                       (hipStream_t)stream, pre0, pre1, pre2, sb0, sb1, sb2, masks, sb_masks, w_mask, cell_prev, d_hidden, \
                       d_cell, B, hidden_size, h, w, d_pre, d_cell_prev, ws_m, ws_w)
    if (d_masks && d_w_mask) DMM_GATES_BWD(true, true);
    else if (d_masks) DMM_GATES_BWD(true, false);
    else if (d_w_mask) DMM_GATES_BWD(false, true);
    else DMM_GATES_BWD(false, false);
#undef DMM_GATES_BWD
    int rc = check_launch();
    if (rc != DMM_OK || !reduce) return rc;
    const unsigned blocks_m = d_masks ? (unsigned)(((int64_t)B * 3 * hw + 255) / 256) : 0u;
    const unsigned blocks_w = d_w_mask ? (unsigned)((36 * hidden_size + 255) / 256) : 0u;
    hipLaunchKernelGGL(clstm_gates_bwd_fold_kernel, dim3(blocks_m + blocks_w), dim3(256), 0, (hipStream_t)stream, ws_m, ws_w,
                       B, hidden_size, h, w, (int)groups, (int)blocks, blocks_m, d_masks, d_w_mask);
    return check_launch();
}

template <typename T>
static int upsample_bwd_entry(const T *d_dst, int64_t sb_dst, int B, int C, int H, int W, int C_dst, int c0, T *d_src,
                              int64_t sb_src, int h, int w, dmm_stream_t stream) {
    if (B < 0 || C <= 0 || h <= 0 || w <= 0 || H <= 0 || W <= 0 || C_dst <= 0) return DMM_ERR_BAD_ARG;
    if (c0 < 0 || c0 + C > C_dst) return DMM_ERR_BAD_ARG;                            // the channel range lies inside d_dst
    if (H < h || W < w) return DMM_ERR_UNSUPPORTED;                                  // the gather ranges assume out >= in
    if (B == 0) return DMM_OK;
    if (!d_dst || !d_src) return DMM_ERR_BAD_ARG;
    if (sb_src < (int64_t)C * h * w || sb_dst < (int64_t)C_dst * H * W) return DMM_ERR_BAD_ARG;
    const int64_t n = (int64_t)B * C * h * w, blocks = (n + 255) / 256;
    if (blocks > 0x7fffffffLL) return DMM_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(upsample_bwd_kernel<T>, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, d_dst, sb_dst, C, H, W,
                       c0, d_src, sb_src, h, w, ac_scale(h, H), ac_scale(w, W), n);
    return check_launch();
}

template <typename T>
static int refine_train_finish_entry(const T *logits, int64_t sb_logits, int64_t so_logits, int h, int w, int B, int O, int n_obj,
                                     int H, int W, float *outs, dmm_stream_t stream) {
    if (B < 0 || O < 0 || n_obj < 0 || n_obj > O || h <= 0 || w <= 0 || H <= 0 || W <= 0) return DMM_ERR_BAD_ARG;
    if (B == 0 || O == 0) return DMM_OK;
    if (!outs || (n_obj > 0 && !logits)) return DMM_ERR_BAD_ARG;
    if (sb_logits < 0 || so_logits < 0) return DMM_ERR_BAD_ARG;
    const int64_t n = (int64_t)B * O * H * W, blocks = (n + 255) / 256;
    if (blocks > 0x7fffffffLL) return DMM_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(refine_train_finish_kernel<T>, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, logits,
                       sb_logits, so_logits, h, w, O, n_obj, H, W, nn_scale(h, H), nn_scale(w, W), outs, n);
    return check_launch();
}

template <typename T>
static int refine_train_finish_bwd_entry(const T *logits, int64_t sb_logits, int64_t so_logits, int h, int w, const float *d_outs,
                                         int B, int O, int n_obj, int H, int W, T *d_logits, int64_t sb_d, int64_t so_d,
                                         dmm_stream_t stream) {
    if (B < 0 || O < 0 || n_obj < 0 || n_obj > O || h <= 0 || w <= 0 || H <= 0 || W <= 0) return DMM_ERR_BAD_ARG;
    if (B == 0 || n_obj == 0) return DMM_OK;
    if (!logits || !d_outs || !d_logits) return DMM_ERR_BAD_ARG;
    if (sb_logits < 0 || so_logits < 0 || sb_d < 0 || so_d < (int64_t)h * w) return DMM_ERR_BAD_ARG;
    const int64_t n = (int64_t)B * n_obj * h * w, blocks = (n + 255) / 256;
    if (blocks > 0x7fffffffLL) return DMM_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(refine_train_finish_bwd_kernel<T>, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, logits,
                       sb_logits, so_logits, h, w, d_outs, O, n_obj, H, W, nn_scale(h, H), nn_scale(w, W), d_logits,
                       sb_d, so_d, n);
    return check_launch();
}

}  // namespace dmm

extern "C" int dmm_mask_pyramid_f32(const float *prev_mask, const float *y_mask, const float *init_pred, int64_t sb_prev,
                                    int64_t so_prev, int64_t sb_y, int64_t so_y, int64_t sb_init, int64_t so_init, int B,
                                    int n_obj, int H, int W, float *out5, float *out4, float *out3, float *out2,
                                    dmm_stream_t stream) {
    if (B < 0 || n_obj < 0 || H <= 0 || W <= 0) return DMM_ERR_BAD_ARG;
    if (B == 0 || n_obj == 0) return DMM_OK;
    if (!prev_mask || !y_mask || !init_pred || !out5 || !out4 || !out3 || !out2) return DMM_ERR_BAD_ARG;
    if (sb_prev < 0 || so_prev < 0 || sb_y < 0 || so_y < 0 || sb_init < 0 || so_init < 0) return DMM_ERR_BAD_ARG;
    const int tiles_x = (W + 31) / 32, tiles_y = (H + 31) / 32;
    const int64_t planes = (int64_t)B * n_obj * 3;
    if (planes > 65535 || (int64_t)tiles_x * tiles_y > 0x7fffffffLL) return DMM_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(dmm::mask_pyramid_kernel, dim3((unsigned)(tiles_x * tiles_y), (unsigned)planes), dim3(256), 0,
                       (hipStream_t)stream, prev_mask, y_mask, init_pred, sb_prev, so_prev, sb_y, so_y, sb_init, so_init, B, H, W,
                       tiles_x, out5, out4, out3, out2);
    return dmm::check_launch();
}

extern "C" int dmm_clstm_gates_f32(const float *pre0, const float *pre1, const float *pre2, int64_t sb0, int64_t sb1, int64_t sb2,
                                   const float *masks, int64_t sb_masks, const float *w_mask, const float *cell_prev, int B,
                                   int hidden_size, int h, int w, float *hidden, float *cell, float *hidden_copy,
                                   int64_t sb_copy, dmm_stream_t stream) {
    return dmm::clstm_gates_entry<float>(pre0, pre1, pre2, sb0, sb1, sb2, masks, sb_masks, w_mask, cell_prev, B, hidden_size, h, w,
                                         hidden, cell, hidden_copy, sb_copy, stream);
}

extern "C" int dmm_clstm_gates_bf16(const void *pre0, const void *pre1, const void *pre2, int64_t sb0, int64_t sb1, int64_t sb2,
                                    const float *masks, int64_t sb_masks, const float *w_mask, const float *cell_prev, int B,
                                    int hidden_size, int h, int w, void *hidden, float *cell, void *hidden_copy, int64_t sb_copy,
                                    dmm_stream_t stream) {
    typedef dmm::bf16_t T;
    return dmm::clstm_gates_entry<T>((const T *)pre0, (const T *)pre1, (const T *)pre2, sb0, sb1, sb2, masks, sb_masks, w_mask,
                                     cell_prev, B, hidden_size, h, w, (T *)hidden, cell, (T *)hidden_copy, sb_copy, stream);
}

// ws_m [groups][B][27][h * w] then ws_w [position blocks][36 * hidden_size]; 0 for sizes the entry refuses or has no work for
extern "C" size_t dmm_clstm_gates_bwd_workspace_bytes(int B, int hidden_size, int h, int w) {
    if (B <= 0 || hidden_size <= 0 || h <= 0 || w <= 0) return 0;
    const int64_t hw = (int64_t)h * w, groups = (hidden_size + dmm::kGateCh - 1) / dmm::kGateCh;
    if ((int64_t)B * hw > 0x7fffffffLL || groups > 65535) return 0;
    const int64_t blocks = ((int64_t)B * hw + 255) / 256;
    return (size_t)(groups * B * 27 * hw + blocks * 36 * hidden_size) * sizeof(float);
}

extern "C" int dmm_clstm_gates_bwd_f32(const float *pre0, const float *pre1, const float *pre2, int64_t sb0, int64_t sb1,
                                       int64_t sb2, const float *masks, int64_t sb_masks, const float *w_mask,
                                       const float *cell_prev, int B, int hidden_size, int h, int w, const float *d_hidden,
                                       const float *d_cell, float *d_pre, float *d_cell_prev, float *d_masks, float *d_w_mask,
                                       void *ws, size_t ws_bytes, dmm_stream_t stream) {
    return dmm::clstm_gates_bwd_entry<float>(pre0, pre1, pre2, sb0, sb1, sb2, masks, sb_masks, w_mask, cell_prev, B, hidden_size, h,
                                             w, d_hidden, d_cell, d_pre, d_cell_prev, d_masks, d_w_mask, ws, ws_bytes, stream);
}

extern "C" int dmm_clstm_gates_bwd_bf16(const void *pre0, const void *pre1, const void *pre2, int64_t sb0, int64_t sb1,
                                        int64_t sb2, const float *masks, int64_t sb_masks, const float *w_mask,
                                        const float *cell_prev, int B, int hidden_size, int h, int w, const void *d_hidden,
                                        const float *d_cell, void *d_pre, float *d_cell_prev, float *d_masks, float *d_w_mask,
                                        void *ws, size_t ws_bytes, dmm_stream_t stream) {
    typedef dmm::bf16_t T;
    return dmm::clstm_gates_bwd_entry<T>((const T *)pre0, (const T *)pre1, (const T *)pre2, sb0, sb1, sb2, masks, sb_masks, w_mask,
                                         cell_prev, B, hidden_size, h, w, (const T *)d_hidden, d_cell, (T *)d_pre, d_cell_prev,
                                         d_masks, d_w_mask, ws, ws_bytes, stream);
}

extern "C" int dmm_upsample_bilinear_into_f32(const float *src, int64_t sb_src, int B, int C, int h, int w, float *dst,
                                              int64_t sb_dst, int C_dst, int c0, int H, int W, int mode, dmm_stream_t stream) {
    return dmm::upsample_into_entry<float>(src, sb_src, B, C, h, w, dst, sb_dst, C_dst, c0, H, W, mode, stream);
}

extern "C" int dmm_upsample_bilinear_into_bf16(const void *src, int64_t sb_src, int B, int C, int h, int w, void *dst,
                                               int64_t sb_dst, int C_dst, int c0, int H, int W, int mode, dmm_stream_t stream) {
    typedef dmm::bf16_t T;
    return dmm::upsample_into_entry<T>((const T *)src, sb_src, B, C, h, w, (T *)dst, sb_dst, C_dst, c0, H, W, mode, stream);
}

extern "C" int dmm_refine_finish_f32(const float *logits, int64_t sb_logits, int64_t so_logits, int h, int w, const int *valid,
                                     int B, int O, int n_obj, int H, int W, float *outs, float *mask_hist,
                                     dmm_stream_t stream) {
    return dmm::refine_finish_entry<float>(logits, sb_logits, so_logits, h, w, valid, B, O, n_obj, H, W, outs, mask_hist, stream);
}

extern "C" int dmm_refine_finish_bf16(const void *logits, int64_t sb_logits, int64_t so_logits, int h, int w, const int *valid,
                                      int B, int O, int n_obj, int H, int W, float *outs, float *mask_hist,
                                      dmm_stream_t stream) {
    return dmm::refine_finish_entry<dmm::bf16_t>((const dmm::bf16_t *)logits, sb_logits, so_logits, h, w, valid, B, O, n_obj, H, W,
                                                 outs, mask_hist, stream);
}

extern "C" int dmm_mask_pyramid_bwd_f32(const float *prev_mask, const float *init_pred, int64_t sb_prev, int64_t so_prev,
                                        int64_t sb_init, int64_t so_init, int B, int n_obj, int H, int W, const float *d_out5,
                                        const float *d_out4, const float *d_out3, const float *d_out2, float *d_prev,
                                        int64_t sb_dprev, int64_t so_dprev, float *d_init, int64_t sb_dinit, int64_t so_dinit,
                                        dmm_stream_t stream) {
    if (B < 0 || n_obj < 0 || H <= 0 || W <= 0) return DMM_ERR_BAD_ARG;
    if (B == 0 || n_obj == 0 || (!d_prev && !d_init)) return DMM_OK;
    if ((d_prev && !prev_mask) || (d_init && !init_pred)) return DMM_ERR_BAD_ARG;
    if (sb_prev < 0 || so_prev < 0 || sb_init < 0 || so_init < 0) return DMM_ERR_BAD_ARG;
    const int64_t hw = (int64_t)H * W;
    if ((d_prev && (so_dprev < hw || sb_dprev < 0)) || (d_init && (so_dinit < hw || sb_dinit < 0))) return DMM_ERR_BAD_ARG;
    const int tiles_x = (W + 31) / 32, tiles_y = (H + 31) / 32;
    const int64_t planes = (int64_t)B * n_obj * ((d_prev ? 1 : 0) + (d_init ? 1 : 0));
    if ((int64_t)B * n_obj * 3 > 65535 || (int64_t)tiles_x * tiles_y > 0x7fffffffLL) return DMM_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(dmm::mask_pyramid_bwd_kernel, dim3((unsigned)(tiles_x * tiles_y), (unsigned)planes), dim3(256), 0,
                       (hipStream_t)stream, prev_mask, init_pred, sb_prev, so_prev, sb_init, so_init, B, H, W, tiles_x, d_out5,
                       d_out4, d_out3, d_out2, d_prev, sb_dprev, so_dprev, d_init, sb_dinit, so_dinit);
    return dmm::check_launch();
}

extern "C" int dmm_upsample_bilinear_bwd_f32(const float *d_dst, int64_t sb_dst, int B, int C, int H, int W, int C_dst, int c0,
                                             float *d_src, int64_t sb_src, int h, int w, dmm_stream_t stream) {
    return dmm::upsample_bwd_entry<float>(d_dst, sb_dst, B, C, H, W, C_dst, c0, d_src, sb_src, h, w, stream);
}

extern "C" int dmm_upsample_bilinear_bwd_bf16(const void *d_dst, int64_t sb_dst, int B, int C, int H, int W, int C_dst, int c0,
                                              void *d_src, int64_t sb_src, int h, int w, dmm_stream_t stream) {
    typedef dmm::bf16_t T;
    return dmm::upsample_bwd_entry<T>((const T *)d_dst, sb_dst, B, C, H, W, C_dst, c0, (T *)d_src, sb_src, h, w, stream);
}

extern "C" int dmm_refine_train_finish_f32(const float *logits, int64_t sb_logits, int64_t so_logits, int h, int w, int B, int O,
                                           int n_obj, int H, int W, float *outs, dmm_stream_t stream) {
    return dmm::refine_train_finish_entry<float>(logits, sb_logits, so_logits, h, w, B, O, n_obj, H, W, outs, stream);
}

extern "C" int dmm_refine_train_finish_bf16(const void *logits, int64_t sb_logits, int64_t so_logits, int h, int w, int B, int O,
                                            int n_obj, int H, int W, float *outs, dmm_stream_t stream) {
    return dmm::refine_train_finish_entry<dmm::bf16_t>((const dmm::bf16_t *)logits, sb_logits, so_logits, h, w, B, O, n_obj, H, W,
                                                       outs, stream);
}

extern "C" int dmm_refine_train_finish_bwd_f32(const float *logits, int64_t sb_logits, int64_t so_logits, int h, int w,
                                               const float *d_outs, int B, int O, int n_obj, int H, int W, float *d_logits,
                                               int64_t sb_d, int64_t so_d, dmm_stream_t stream) {
    return dmm::refine_train_finish_bwd_entry<float>(logits, sb_logits, so_logits, h, w, d_outs, B, O, n_obj, H, W, d_logits, sb_d,
                                                     so_d, stream);
}

extern "C" int dmm_refine_train_finish_bwd_bf16(const void *logits, int64_t sb_logits, int64_t so_logits, int h, int w,
                                                const float *d_outs, int B, int O, int n_obj, int H, int W, void *d_logits,
                                                int64_t sb_d, int64_t so_d, dmm_stream_t stream) {
    typedef dmm::bf16_t T;
    return dmm::refine_train_finish_bwd_entry<T>((const T *)logits, sb_logits, so_logits, h, w, d_outs, B, O, n_obj, H, W,
                                                 (T *)d_logits, sb_d, so_d, stream);
}
