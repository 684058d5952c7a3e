// dmm_launchers.h -- every dmm:: launcher that one .hip defines and another calls, declared ONCE (the solver's are in
// dmm_solve.h).  The defining file includes this header too, so a definition that drifts from its declaration does not
// compile; default arguments are given here and nowhere else.
#pragma once
#include "dmm_common.h"

namespace dmm {

// dmm_cosine_lanes.hip: the one-launch feature similarity; DMM_ERR_UNSUPPORTED (nothing launched) outside D in
// {256, 512, 1024}.  zero_ptr / zero_words: a buffer the launch clears on the side; n_valid: live proposals per frame.
int cosine_lanes_launch(const float *feat_t, const float *feat_p, int B, int N, int M, int D, float *cos_out,
                        hipStream_t stream, int32_t *zero_ptr = nullptr, int64_t zero_words = 0,
                        const int32_t *n_valid = nullptr);
// dmm_cosine.hip: dmm_feature_normalize_f32 on two row sets with one launch, which can also clear a buffer on the side
int feature_normalize2_launch(const float *in_a, int64_t rows_a, float *out_a, float *norms_a, const float *in_b,
                              int64_t rows_b, float *out_b, float *norms_b, int D, hipStream_t stream,
                              void *zero_ptr = nullptr, size_t zero_bytes = 0);

// dmm_cost.hip: similarity and counts of a handful of dense frames in one launch (DMM_ERR_UNSUPPORTED: nothing launched)
int front_small_launch(const void *masks_p, const void *masks_t, const void *masks_t2, int dtype, const float *feat_t,
                       const float *feat_p, int B, int N, int M, int HW, int D, int64_t sp_b, int64_t sp_n, int64_t st_b,
                       int64_t st_m, int64_t st2_b, int64_t st2_m, float *cos_out, int32_t *inter, int32_t *area_p,
                       int32_t *area_t, int32_t *inter2, int32_t *area_t2, bool tables_zero, hipStream_t stream);
// dmm_cost.hip: dmm_iou_counts / dmm_iou_counts_dual on tables the caller has already cleared on this stream (the
// dispatch behind every count entry with tables_zeroed = true)
int iou_counts_prezeroed(const void *masks_p, const void *masks_t, int dtype, int B, int N, int M, int HW, int64_t sp_b,
                         int64_t sp_n, int64_t st_b, int64_t st_m, const int32_t *n_valid, const int32_t *m_valid,
                         int32_t *inter, int32_t *area_p, int32_t *area_t, dmm_stream_t stream);
int iou_counts_dual_prezeroed(const void *masks_p, const void *masks_t, const void *masks_t2, int dtype, int B, int N, int M,
                              int HW, int64_t sp_b, int64_t sp_n, int64_t st_b, int64_t st_m, int64_t st2_b, int64_t st2_m,
                              const int32_t *n_valid, const int32_t *m_valid, int32_t *inter, int32_t *area_p,
                              int32_t *area_t, int32_t *inter2, int32_t *area_t2, dmm_stream_t stream);
// dmm_mix.hip: dmm_mask_mix_bwd into a dRb the caller has already cleared (the backward behind every mix entry with
// MixBwd::drb_zeroed set)
int mask_mix_bwd_prezeroed(const float *Rb, const void *masks_p, int dtype, const float *dout, int B, int N, int M, int Pp,
                           int HW, int64_t sp_b, int64_t sp_n, const int32_t *n_valid, const int32_t *m_valid, float *dRb,
                           dmm_stream_t stream);

// The checks every one-call entry starts with.  *go = true: go on; otherwise the return value is the entry's answer
// (DMM_OK: nothing to do).  have_pointers: none of the entry's mandatory pointers is null.
static inline int one_call_check(int B, int N, int M, int HW, int D, bool have_pointers, bool *go) {
    *go = false;
    if (B < 0 || N < 0 || M < 0 || HW < 0 || D < 0) return DMM_ERR_BAD_ARG;
    if (B == 0 || M == 0) return DMM_OK;
    if (N == 0 || !have_pointers) return DMM_ERR_BAD_ARG;
    *go = true;
    return DMM_OK;
}
// the mix needs the pixel values: 1-bit planes are an input format of the counts only
static inline bool soft_planes(int dtype) { return dtype == DMM_F32 || dtype == DMM_F16 || dtype == DMM_BF16; }

// ---- dmm_front.hip: the front and the tail of the one-call entries (dmm_match_forward*, dmm_match_solve_packed*,
// dmm_match_train_forward) ---------------------------------------------------------------------------------------------
// Feature similarity into `cos` and the IoU counts into the tables, down this chain (the first link that takes the
// shape):
//   1. dense frames, a handful of them: similarity and counts in ONE launch (front_small_launch)
//   2. the lanes kernel, which clears the tables on the side, then the counts on the cleared tables
//   3. a clearing launch, the counts, then the dense tile similarity (dmm_cosine_features_f32)
//   4. ... or both feature sets normalised and dmm_cosine_f32
// COSINE_KERNEL = 1 skips 1 and 2.  The last four fields are where the entries differ on purpose.
struct Front {
    const void *masks_p, *masks_t;       // the planes the counts read (DMM_PACKED1: words) and their element strides
    int dtype;
    int64_t sp_b, sp_n, st_b, st_m;
    const void *targets;                 // training: a second template set counted in the same pass (null: none)
    int64_t sg_b, sg_m;
    const float *feat_p, *feat_t;
    int B, N, M, HW, D;
    const int32_t *n_valid, *m_valid;
    float *cos;                          // out [B, M, N]
    int32_t *inter, *area_p, *area_t;    // out; with inter2 | area_t2 one block of table_words words from `inter`
    int32_t *inter2, *area_t2;           // the targets' tables (null without targets)
    size_t table_words;
    float *featn_p, *featn_t;            // room for the normalised rows of link 4
    bool tables_zero;                    // the caller vouches the tables are zero already (link 1 skips its clear)
    bool ragged_lanes;                   // ragged batches take link 2 (dmm_match_forward_ws keeps them on link 4)
    bool dense_tile;                     // dense batches may take link 3's tile kernel (the packed entries go on to 4)
    bool split_norm;                     // link 4 normalises with two launches (dmm_match_forward_ws), not one
};
// *fused (may be null): link 1 ran -- its tables are the ones the solver may be asked to leave zero
int match_front(const Front &f, hipStream_t stream, bool *fused = nullptr);
// full_outmask [B, M, HW] from Rb: train mode keeps every R > 0.01, so the rows share planes and the union of their
// supports is streamed once (dmm_mask_mix_shared_to); test mode keeps one proposal per row (dmm_mask_mix)
int match_mix(const float *Rb, const void *masks_p, int dtype, int B, int N, int M, int HW, int64_t sp_b, int64_t sp_n,
              const int32_t *n_valid, const int32_t *m_valid, int is_test, float *full_outmask, dmm_stream_t stream);

}  // namespace dmm
