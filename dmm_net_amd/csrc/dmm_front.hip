// dmm_front.hip -- what the one-call entries (dmm_api.hip, dmm_train.hip) share in front of and behind the solver:
// match_front (feature similarity + IoU counts, with their fallback chain) and match_mix.  See dmm_launchers.h: a Front IS
// the counts' bundle (CountArgs) plus the similarity's arguments, so the count launchers take it as it stands.
#include "dmm_launchers.h"

namespace dmm {

int match_front(const Front &f, hipStream_t stream, bool *fused) {
    if (fused) *fused = false;
    const bool dense = !f.n_valid && !f.m_valid;
    const bool lanes = opt(DMM_OPT_COSINE_KERNEL) != 1;
    int rc = DMM_ERR_UNSUPPORTED;
    // 1. a handful of dense frames: table clear, then similarity and counts beside each other in ONE launch
    if (dense && lanes) {
        rc = front_small_launch(f, stream);
        if (rc == DMM_OK && fused) *fused = true;
        if (rc != DMM_ERR_UNSUPPORTED) return rc;
    }
    // 2. the one-launch similarity, which also clears the count tables (no clearing launch in front of the counts): every
    // frame in the summation order of ITS live proposal count; template rows past m_valid are computed and never read
    // (every consumer masks them) -- bit identical to link 4 on every live entry
    if (lanes && (dense || f.ragged_lanes))
        rc = cosine_lanes_launch(f.feat_t, f.feat_p, f.B, f.N, f.M, f.D, f.cos, stream, f.inter, (int64_t)f.table_words,
                                 f.n_valid);
    if (rc == DMM_OK) return iou_counts_launch(f, /*tables_zeroed=*/true, stream);
    if (rc != DMM_ERR_UNSUPPORTED) return rc;
    // 3. a D the lanes kernel does not take (or COSINE_KERNEL = 1): clear, count, then the tile kernel on dense batches
    DMM_HIP_TRY(zero_async(f.inter, sizeof(int32_t) * f.table_words, stream));
    rc = iou_counts_launch(f, /*tables_zeroed=*/true, stream);
    if (rc != DMM_OK) return rc;
    if (dense && f.dense_tile) {
        rc = dmm_cosine_features_f32(f.feat_t, f.feat_p, f.B, f.N, f.M, f.D, f.cos, stream);
        if (rc != DMM_ERR_UNSUPPORTED) return rc;
    }
    // 4. any D, ragged or not: the rows normalised, then their products summed (D = 0: nothing to normalise)
    if (f.split_norm) {
        rc = dmm_feature_normalize_f32(f.feat_p, (int64_t)f.B * f.N, f.D, f.featn_p, nullptr, stream);
        if (rc != DMM_OK) return rc;
        rc = dmm_feature_normalize_f32(f.feat_t, (int64_t)f.B * f.M, f.D, f.featn_t, nullptr, stream);
    } else {
        rc = f.D == 0 ? DMM_OK
                      : feature_normalize2_launch(f.feat_p, (int64_t)f.B * f.N, f.featn_p, nullptr, f.feat_t,
                                                  (int64_t)f.B * f.M, f.featn_t, nullptr, f.D, stream);
    }
    if (rc != DMM_OK) return rc;
    return dmm_cosine_f32(f.featn_t, f.featn_p, f.B, f.N, f.M, f.D, f.n_valid, f.m_valid, f.cos, stream);
}

int match_mix(const float *Rb, const void *masks_p, int dtype, int B, int N, int M, int HW, int64_t sp_b, int64_t sp_n,
              const int32_t *n_valid, const int32_t *m_valid, int is_test, float *full_outmask, dmm_stream_t stream) {
    const int Pp = N > M ? N : M + 1;
    if (is_test)
        return dmm_mask_mix(Rb, masks_p, dtype, B, N, M, Pp, HW, sp_b, sp_n, n_valid, m_valid, full_outmask, (int64_t)M * HW,
                            HW, stream);
    return dmm_mask_mix_shared_to(Rb, masks_p, dtype, B, N, M, Pp, HW, sp_b, sp_n, n_valid, m_valid, full_outmask, DMM_F32,
                                  (int64_t)M * HW, HW, stream);
}

}  // namespace dmm
