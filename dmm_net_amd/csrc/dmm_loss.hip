// dmm_loss.hip -- (13) the soft-IoU mask loss of the trainer's frame step: softIoU under softIoULoss
// (dmm/utils/hungarian.py:62-86, dmm/utils/objectives.py:25-35) as called on the matching layer's output
// (dmm/modules/trainer.py:205-206) and on the refine decoder's (trainer.py:281-293), with the hard IoU logged beside each
// (dmm/utils/match_helper.py:9-28 from trainer.py:188-196 and :296-300).  Three kernels:
//   mask_loss_partials_kernel  one read of pred and target: per (row, chunk) the two fp32 sums and the two integer counts
//   mask_loss_finish_kernel    one workgroup: rows, selection, the three scalars, the backward's coefficient pairs
//   mask_loss_bwd_kernel       one read of target, one write of dpred
// No float atomics: every sum has one order (written at each fold), so there is no _det twin.  Memory bound without reuse;
// at the trainer's 20 rows of 255 x 448 the three launches are a few microseconds of traffic each and sit on launch latency.
#include "dmm_launchers.h"

namespace dmm {

constexpr int kLossThreads = 256;                                        // four waves
constexpr int kLossChunk = DMM_MASK_LOSS_CHUNK;                           // pixels of one row per workgroup
constexpr int kLossLoads = kLossChunk / (kLossThreads * 4);               // 16-byte loads of pred in flight per lane
static_assert(kLossLoads * kLossThreads * 4 == kLossChunk && kLossLoads >= 1, "a chunk is whole 16-byte loads per lane");
typedef uint32_t uint4w __attribute__((ext_vector_type(4), aligned(4)));  // a slab slot: sum p y | sum p + y - p y | #and | #or

// the workspace: the coefficient pairs [rows][2] fp32 (what the backward reads), then the slab [rows][chunks] of 16 bytes
static inline int64_t loss_chunks(int HW) { return ((int64_t)HW + kLossChunk - 1) / kLossChunk; }
static inline size_t loss_slab_offset(int64_t rows) { return (size_t)((rows * 8 + 15) / 16 * 16); }

// 4 pixels of a row from pixel i on: one 16-byte (fp32) / 8-byte (16-bit) non-temporal load, or the row's tail one by one
// with zeros behind it (a zero pixel adds nothing to either sum and is in neither count)
template <typename T>
__device__ __forceinline__ void loss_load4(const T *row, int64_t i, int HW, float (&v)[4]) {
    if (i + 4 <= HW) {
        MaskIO<T>::load4(row + i, v);
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) v[k] = i + k < HW ? MaskIO<T>::load1(row + i + k) : 0.0f;
    }
}

// grid (chunks, rows).  Lane l of the workgroup takes pixels chunk * kLossChunk + (j * 256 + l) * 4 .. + 3, j < kLossLoads: all
// loads are issued before the first use.  Sums: the lane's 16 pixels in ascending order, wave_sum's tree, waves 0..3.
template <typename T>
__global__ __launch_bounds__(kLossThreads) void mask_loss_partials_kernel(
    const float *__restrict__ pred, int64_t sb_pred, int64_t so_pred, const T *__restrict__ target, int64_t sb_tgt,
    int64_t so_tgt, int n_obj, int HW, int chunks, uint4w *__restrict__ slab) {
    const int r = blockIdx.y, c = blockIdx.x;
    const int b = r / n_obj, t = r - b * n_obj;
    const float *p = pred + (int64_t)b * sb_pred + (int64_t)t * so_pred;
    const T *y = target + (int64_t)b * sb_tgt + (int64_t)t * so_tgt;
    const int64_t i0 = (int64_t)c * kLossChunk + (int64_t)threadIdx.x * 4;
    float pv[kLossLoads][4], yv[kLossLoads][4];
#pragma unroll
    for (int j = 0; j < kLossLoads; ++j) {
        loss_load4<float>(p, i0 + j * kLossThreads * 4, HW, pv[j]);
        loss_load4<T>(y, i0 + j * kLossThreads * 4, HW, yv[j]);
    }
    float si = 0.0f, su = 0.0f;
    int n_and = 0, n_or = 0;                               // wave-uniform: a ballot per pixel column
#pragma unroll
    for (int j = 0; j < kLossLoads; ++j) {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const float py = pv[j][k] * yv[j][k];
            si = si + py;
            su = su + ((pv[j][k] + yv[j][k]) - py);        // out + target - out * target, hungarian.py:81
            const bool hp = pv[j][k] > 0.5f, hy = yv[j][k] > 0.5f;
            n_and += __builtin_popcountll(__ballot(hp && hy));
            n_or += __builtin_popcountll(__ballot(hp || hy));
        }
    }
    si = wave_sum(si);
    su = wave_sum(su);
    __shared__ float sum_s[kLossThreads / kWave][2];
    __shared__ int cnt_s[kLossThreads / kWave][2];
    const int wave = threadIdx.x / kWave;
    if (threadIdx.x % kWave == 0) {
        sum_s[wave][0] = si;
        sum_s[wave][1] = su;
        cnt_s[wave][0] = n_and;
        cnt_s[wave][1] = n_or;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        float fi = sum_s[0][0], fu = sum_s[0][1];
        int ca = cnt_s[0][0], co = cnt_s[0][1];
#pragma unroll
        for (int w = 1; w < kLossThreads / kWave; ++w) {
            fi = fi + sum_s[w][0];
            fu = fu + sum_s[w][1];
            ca += cnt_s[w][0];
            co += cnt_s[w][1];
        }
        uint4w q;
        q.x = __float_as_uint(fi); q.y = __float_as_uint(fu); q.z = (uint32_t)ca; q.w = (uint32_t)co;
        slab[(int64_t)r * chunks + c] = q;
    }
}

// sw.byte() != 0 (objectives.py:32): the float truncated to an integer, its low 8 bits
__device__ __forceinline__ bool loss_selected(float w) { return (((int)w) & 0xff) != 0; }

// One workgroup; thread l owns rows l, l + 256, ...  Block folds: the thread's rows in ascending order, wave_sum's tree,
// waves 0..3.  coef: [rows][2], first (I_r, U_r) parked by the row's own thread, then the pair the backward reads.
__global__ __launch_bounds__(kLossThreads) void mask_loss_finish_kernel(
    const uint4w *__restrict__ slab, int chunks, const float *__restrict__ sw, int64_t sb_sw, const int32_t *__restrict__ valid,
    int B, int O, int n_obj, float *__restrict__ cost, float *__restrict__ hard, float *__restrict__ scalars,
    float *__restrict__ coef) {
    const int R = B * n_obj;
    int any = 0;                                           // (sw.data > 0).any(), objectives.py:31
    for (int r = threadIdx.x; r < R; r += kLossThreads) {
        const int b = r / n_obj, t = r - b * n_obj;
        any |= sw[(int64_t)b * sb_sw + t] > 0.0f;
    }
    any = __syncthreads_or(any);
    // sum of the selected costs | sum hard * valid | sum hard | K | nv   (the two counts stay exact in fp32: < 2^24)
    float acc[5] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
    for (int r = threadIdx.x; r < R; r += kLossThreads) {
        const int b = r / n_obj, t = r - b * n_obj;
        float fi = 0.0f, fu = 0.0f;
        int ca = 0, co = 0;
        for (int c = 0; c < chunks; ++c) {
            const uint4w q = slab[(int64_t)r * chunks + c];
            fi = fi + __uint_as_float(q.x);
            fu = fu + __uint_as_float(q.y);
            ca += (int)q.z;
            co += (int)q.w;
        }
        const float U = fu + 1e-6f;
        const float cost_r = 1.0f - fi / U;
        const float hard_r = (float)ca / ((float)co + 1e-6f);
        cost[r] = cost_r;
        hard[r] = hard_r;
        coef[2 * r] = fi;
        coef[2 * r + 1] = U;
        if (!any || loss_selected(sw[(int64_t)b * sb_sw + t])) {
            acc[0] = acc[0] + cost_r;
            acc[3] = acc[3] + 1.0f;
        }
        if (valid) acc[1] = acc[1] + hard_r * (float)valid[b * O + t];
        acc[2] = acc[2] + hard_r;
    }
    if (valid)
        for (int i = threadIdx.x; i < B * O; i += kLossThreads) acc[4] = acc[4] + (float)valid[i];
    wave_sum_rows<5>(acc);
    __shared__ float fold_s[kLossThreads / kWave][5];
    if (threadIdx.x % kWave == 0) {
#pragma unroll
        for (int i = 0; i < 5; ++i) fold_s[threadIdx.x / kWave][i] = acc[i];
    }
    __syncthreads();
    float tot[5];
#pragma unroll
    for (int i = 0; i < 5; ++i) {
        tot[i] = fold_s[0][i];
#pragma unroll
        for (int w = 1; w < kLossThreads / kWave; ++w) tot[i] = tot[i] + fold_s[w][i];
    }
    const float K = tot[3], nv = tot[4];
    if (threadIdx.x == 0) {
        scalars[0] = tot[0] / K;                                                  // torch.mean of the selection
        scalars[1] = nv > 0.0f ? tot[1] / (nv + 1e-6f) : 0.0f;                    // trainer.py:195-196
        scalars[2] = nv > 0.0f ? tot[2] / (nv + 1e-6f) : 0.0f;                    // trainer.py:299-300
    }
    for (int r = threadIdx.x; r < R; r += kLossThreads) {
        const int b = r / n_obj, t = r - b * n_obj;
        const float fi = coef[2 * r], U = coef[2 * r + 1];
        const bool sel = !any || loss_selected(sw[(int64_t)b * sb_sw + t]);
        const float den = K * U;
        coef[2 * r] = sel ? -1.0f / den : 0.0f;                                   // a_r = -sel / (K U)
        coef[2 * r + 1] = sel ? (fi / U) / den : 0.0f;                            // b_r = sel I / (K U^2)
    }
}

// grid (chunks, B * O).  dpred[b, t, i] = d_loss * (a_r y + b_r (1 - y)) for t < n_obj, zeros for the padded planes.
template <typename T>
__global__ __launch_bounds__(kLossThreads) void mask_loss_bwd_kernel(
    const T *__restrict__ target, int64_t sb_tgt, int64_t so_tgt, const float *__restrict__ coef,
    const float *__restrict__ d_loss, int O, int n_obj, int HW, float *__restrict__ dpred, int64_t sb_dpred, int64_t so_dpred) {
    const int b = blockIdx.y / O, t = blockIdx.y - b * O;
    const bool live = t < n_obj;
    float *d = dpred + (int64_t)b * sb_dpred + (int64_t)t * so_dpred;
    const int64_t i0 = (int64_t)blockIdx.x * kLossChunk + (int64_t)threadIdx.x * 4;
    float yv[kLossLoads][4];
    float ga = 0.0f, gb = 0.0f;
    if (live) {
        const T *y = target + (int64_t)b * sb_tgt + (int64_t)t * so_tgt;
#pragma unroll
        for (int j = 0; j < kLossLoads; ++j) loss_load4<T>(y, i0 + j * kLossThreads * 4, HW, yv[j]);
        const int r = b * n_obj + t;
        const float g = *d_loss;
        ga = g * coef[2 * r];
        gb = g * coef[2 * r + 1];
    }
#pragma unroll
    for (int j = 0; j < kLossLoads; ++j) {
        const int64_t i = i0 + j * kLossThreads * 4;
        float v[4] = {0.0f, 0.0f, 0.0f, 0.0f};
        if (live) {
#pragma unroll
            for (int k = 0; k < 4; ++k) v[k] = ga * yv[j][k] + gb * (1.0f - yv[j][k]);
        }
        if (i + 4 <= HW) {
            float4u q;
            q.x = v[0]; q.y = v[1]; q.z = v[2]; q.w = v[3];
            *reinterpret_cast<float4u *>(d + i) = q;
        } else {
            for (int k = 0; i + k < HW; ++k) d[i + k] = v[k];
        }
    }
}

// ---- host side: one argument bundle, one check -------------------------------------------------------------------
struct MaskLossArgs {
    const float *pred;                   // forward only
    int64_t sb_pred, so_pred;
    const void *target;
    int target_dtype;
    int64_t sb_tgt, so_tgt;
    const float *sw;                     // forward only
    int64_t sb_sw;
    const int32_t *valid;                // may be null
    int B, O, n_obj, HW;
    float *cost, *hard, *scalars;        // forward only
    void *workspace;
    size_t workspace_bytes;
    const float *d_loss;                 // backward only
    float *dpred;
    int64_t sb_dpred, so_dpred;
};

static size_t mask_loss_workspace_bytes(int B, int n_obj, int HW) {
    if (B <= 0 || n_obj <= 0 || HW <= 0) return 0;
    const int64_t rows = (int64_t)B * n_obj;
    return loss_slab_offset(rows) + (size_t)rows * (size_t)loss_chunks(HW) * 16;
}

// The answers of both entries, in the order include/dmm_match.h (13) lists.  *go = true: launch.
static int mask_loss_check(const MaskLossArgs &a, bool backward, bool *go) {
    *go = false;
    if (a.B < 0 || a.O < 0 || a.n_obj < 0 || a.HW < 0 || a.n_obj > a.O) return DMM_ERR_BAD_ARG;
    if (a.so_tgt < a.HW || a.sb_tgt < 0) return DMM_ERR_BAD_ARG;
    if (backward ? (a.so_dpred < a.HW || a.sb_dpred < 0) : (a.so_pred < a.HW || a.sb_pred < 0 || a.sb_sw < 0))
        return DMM_ERR_BAD_ARG;
    if (a.B == 0 || a.HW == 0 || (backward ? a.O : a.n_obj) == 0) return DMM_OK;
    if (!a.target) return DMM_ERR_BAD_ARG;
    if (backward ? (!a.d_loss || !a.dpred) : (!a.pred || !a.sw || !a.cost || !a.hard || !a.scalars)) return DMM_ERR_BAD_ARG;
    if (!soft_planes(a.target_dtype)) return DMM_ERR_UNSUPPORTED;
    if ((int64_t)a.B * a.O > 65535) return DMM_ERR_UNSUPPORTED;               // (a grid axis; b * O + t stays an int)
    const size_t need = mask_loss_workspace_bytes(a.B, a.n_obj, a.HW);        // (0: a backward that only writes zero planes)
    if (need && (!a.workspace || a.workspace_bytes < need)) return DMM_ERR_WORKSPACE;
    *go = true;
    return DMM_OK;
}

}  // namespace dmm

extern "C" size_t dmm_mask_iou_loss_workspace_bytes(int B, int n_obj, int HW) {
    return dmm::mask_loss_workspace_bytes(B, n_obj, HW);
}

extern "C" int dmm_mask_iou_loss_fwd(const float *pred, int64_t sb_pred, int64_t so_pred, const void *target, int target_dtype,
                                     int64_t sb_tgt, int64_t so_tgt, const float *sw, int64_t sb_sw, const int *valid, int B,
                                     int O, int n_obj, int HW, float *cost, float *hard, float scalars[3], void *workspace,
                                     size_t workspace_bytes, dmm_stream_t stream) {
    using namespace dmm;
    const MaskLossArgs a = {pred, sb_pred, so_pred, target, target_dtype, sb_tgt, so_tgt, sw, sb_sw, valid, B, O, n_obj, HW,
                            cost, hard, scalars, workspace, workspace_bytes, nullptr, nullptr, 0, 0};
    bool go;
    const int rc = mask_loss_check(a, false, &go);
    if (!go) return rc;
    const int rows = B * n_obj, chunks = (int)loss_chunks(HW);
    float *coef = (float *)workspace;
    uint4w *slab = (uint4w *)((char *)workspace + loss_slab_offset(rows));
    const int launched = with_plane_type(target_dtype, target, DMM_ERR_UNSUPPORTED, [&](auto tgt) {
        typedef plane_type_of<decltype(tgt)> T;
        hipLaunchKernelGGL((mask_loss_partials_kernel<T>), dim3((unsigned)chunks, (unsigned)rows), dim3(kLossThreads), 0,
                           (hipStream_t)stream, pred, sb_pred, so_pred, tgt, sb_tgt, so_tgt, n_obj, HW, chunks, slab);
        return check_launch();
    });
    if (launched != DMM_OK) return launched;
    hipLaunchKernelGGL(mask_loss_finish_kernel, dim3(1), dim3(kLossThreads), 0, (hipStream_t)stream, slab, chunks, sw, sb_sw,
                       (const int32_t *)valid, B, O, n_obj, cost, hard, scalars, coef);
    return check_launch();
}

extern "C" int dmm_mask_iou_loss_bwd(const void *target, int target_dtype, int64_t sb_tgt, int64_t so_tgt, const float *d_loss,
                                     int B, int O, int n_obj, int HW, const void *workspace, size_t workspace_bytes,
                                     float *dpred, int64_t sb_dpred, int64_t so_dpred, dmm_stream_t stream) {
    using namespace dmm;
    const MaskLossArgs a = {nullptr, 0, 0, target, target_dtype, sb_tgt, so_tgt, nullptr, 0, nullptr, B, O, n_obj, HW,
                            nullptr, nullptr, nullptr, const_cast<void *>(workspace), workspace_bytes, d_loss, dpred, sb_dpred,
                            so_dpred};
    bool go;
    const int rc = mask_loss_check(a, true, &go);
    if (!go) return rc;
    const int chunks = (int)loss_chunks(HW);
    const float *coef = (const float *)workspace;
    return with_plane_type(target_dtype, target, DMM_ERR_UNSUPPORTED, [&](auto tgt) {
        typedef plane_type_of<decltype(tgt)> T;
        hipLaunchKernelGGL((mask_loss_bwd_kernel<T>), dim3((unsigned)chunks, (unsigned)(B * O)), dim3(kLossThreads), 0,
                           (hipStream_t)stream, tgt, sb_tgt, so_tgt, coef, d_loss, O, n_obj, HW, dpred, sb_dpred, so_dpred);
        return check_launch();
    });
}
