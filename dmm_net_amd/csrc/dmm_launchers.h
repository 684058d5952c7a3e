// dmm_launchers.h -- every dmm:: launcher that one .hip defines and another calls, declared ONCE (the solver's are in
// dmm_solve.h).  The defining file includes this header too, so a definition that drifts from its declaration does not
// compile; default arguments are given here and nowhere else.  The host-side argument bundles that cross files live here
// too: CountArgs (the IoU counts) and Front (the one-call entries' front), which derives from it.
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

// The arguments of the IoU counts, for every caller and for dmm_cost.hip itself: the planes, the live counts, the tables.
struct CountArgs {
    const void *masks_p, *masks_t;       // the planes the counts read (DMM_PACKED1: words)
    const void *masks_t2;                // a second template set counted in the same pass (training: the targets); null: none
    int dtype;
    int B, N, M, HW;
    int64_t sp_b, sp_n, st_b, st_m;      // element strides; sp_b = kFrameTable: masks_p is the device table of the frames
    int64_t st2_b, st2_m;
    const int32_t *n_valid, *m_valid;
    int32_t *inter, *area_p, *area_t;    // out [B, M, N], [B, N], [B, M]
    int32_t *inter2, *area_t2;           // the second set's tables (null without masks_t2)
};
// dmm_cost.hip: the dispatch behind every count entry.  tables_zeroed: the caller has already cleared every table on this
// stream (the front: the launch before this one did) -- otherwise the counts clear them first
int iou_counts_launch(const CountArgs &a, bool tables_zeroed, hipStream_t stream);

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
struct Front : CountArgs {
    const float *feat_p, *feat_t;
    int D;
    float *cos;                          // out [B, M, N]
    size_t table_words;                  // inter | area_p | area_t (| inter2 | area_t2) are one block of so many words
    float *featn_p, *featn_t;            // room for the normalised rows of link 4
    bool tables_zero;                    // the caller vouches the tables are zero already (link 1 skips its clear)
    bool ragged_lanes;                   // ragged batches take link 2 (dmm_match_forward_ws keeps them on link 4)
    bool dense_tile;                     // dense batches may take link 3's tile kernel (the packed entries go on to 4)
    bool split_norm;                     // link 4 normalises with two launches (dmm_match_forward_ws), not one
};
// dmm_cost.hip: link 1 -- similarity and counts of a handful of dense frames in one launch (DMM_ERR_UNSUPPORTED: nothing
// launched)
int front_small_launch(const Front &f, hipStream_t stream);
// *fused (may be null): link 1 ran -- its tables are the ones the solver may be asked to leave zero
int match_front(const Front &f, hipStream_t stream, bool *fused = nullptr);
// full_outmask [B, M, HW] from Rb: train mode keeps every R > 0.01, so the rows share planes and the union of their
// supports is streamed once (dmm_mask_mix_shared_to); test mode keeps one proposal per row (dmm_mask_mix)
int match_mix(const float *Rb, const void *masks_p, int dtype, int B, int N, int M, int HW, int64_t sp_b, int64_t sp_n,
              const int32_t *n_valid, const int32_t *m_valid, int is_test, float *full_outmask, dmm_stream_t stream);

}  // namespace dmm
