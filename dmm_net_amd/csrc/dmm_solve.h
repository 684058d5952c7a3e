// dmm_solve.h -- shared between the two mappings of the relaxed-assignment solver:
//   dmm_solve.hip     thread = column, one wave(-group) per frame   (throughput form: thousands of frames in flight)
//   dmm_solve_rs.hip  row-split, RG x CG waves per frame            (latency form / wide tables)
// Both issue the same fp32 operations in the same order (reference relax_match.py:36-105): bit-identical results.
#pragma once
#include <stdlib.h>

#include "dmm_torch_order.h"

namespace dmm {

struct RelaxParams {
    int max_iter, proj_iter;
    float lr;
};

// ---- host-side argument bundles of the layer solvers (the kernels' own signatures spell the lists out) ----
struct SolveIn {
    const float *cos;                                  // [B, M, N] feature similarity
    const int32_t *inter, *area_p, *area_t;            // the IoU count tables
    const float *score_p;
    int B, N, M;
    const int32_t *n_valid, *m_valid;                  // live proposals / templates per frame (null: all)
};
struct SolveOut {
    float *sim, *R, *Rb, *match_score, *det_score;     // R may be null
    int32_t *iters;                                    // may be null
    float *X_final;                                    // may be null
};
// ... as the leading arguments of a solver kernel launch (X_final or the tape's pointers follow)
#define DMM_SOLVE_KARGS(in, w_feat, w_iou, prm, is_test, out)                                                          \
    (in).cos, (in).inter, (in).area_p, (in).area_t, (in).score_p, (in).N, (in).M, (in).n_valid, (in).m_valid, w_feat,    \
        w_iou, prm, is_test, (out).sim, (out).R, (out).Rb, (out).match_score, (out).det_score, (out).iters

// solver width of an [M, N] table: the proposals, or one dummy column more than the templates
static inline int padded_width(int N, int M) { return N > M ? N : M + 1; }
static inline bool in_fast_envelope(int N, int M) {
    return M <= DMM_MAX_TEMPLATES && padded_width(N, M) <= DMM_MAX_PROPOSALS;
}

// The checks every solver entry starts with.  *go = true: launch; otherwise the return value is the entry's answer
// (DMM_OK: nothing to solve).  envelope: the entry serves the compiled fast kernels only.  is_test is reduced to 0 / 1:
// the upper bits of the kernels' argument are the library's own.
static inline int solve_entry_check(const SolveIn &in, const SolveOut &out, int max_iter, int proj_iter, bool envelope,
                                    int *is_test, bool *go) {
    *go = false;
    *is_test = *is_test != 0;
    if (in.B < 0 || in.N < 0 || in.M < 0 || max_iter < 0 || proj_iter < 0) return DMM_ERR_BAD_ARG;
    if (in.B == 0 || in.M == 0) return DMM_OK;
    if (in.N == 0) return DMM_ERR_BAD_ARG;
    if (!in.cos || !in.inter || !in.area_p || !in.area_t || !in.score_p || !out.sim || !out.Rb || !out.match_score ||
        !out.det_score)
        return DMM_ERR_BAD_ARG;
    if (envelope && !in_fast_envelope(in.N, in.M)) return DMM_ERR_UNSUPPORTED;
    *go = true;
    return DMM_OK;
}

// python: sim*(1-w) + iou*w with w a python float -> both scalars rounded to fp32 once
static inline void sim_weights(float score_weight, float &w_feat, float &w_iou) {
    w_feat = (float)(1.0 - (double)score_weight);
    w_iou = score_weight;
}

// Which mapping serves a launch of B frames with M template rows and solver width Pp.  The row-split form was built
// to cut the latency of a single frame's dependent chain.  Since round 3 the one-wave form is the
// default everywhere (dmm_solve.hip has the figures): row-split runs only where DMM_OPT_SOLVER_KERNEL = 1 asks for it
// and it is compiled (Pp <= 64); 0 forces thread-per-column.  The tests run every solver golden through both.
bool use_row_split(int B, int M, int Pp);

int launch_relax_match_rs(const SolveIn &in, float w_feat, float w_iou, RelaxParams prm, int is_test, const SolveOut &out,
                          hipStream_t stream);
int launch_relax_solve_rs(const float *C, int B, int n, int m, const int32_t *rows_valid, const int32_t *cols_valid,
                          RelaxParams prm, float *X_final, float *R_out, float *cost_out, int32_t *iters_out,
                          hipStream_t stream);

// dmm_relax_match_f32 with the table-clearing request of dmm_match_forward_ws and the training call's tape (dmm_solve.hip)
int relax_match_launch(const SolveIn &in, float score_weight, RelaxParams prm, int is_test, const SolveOut &out,
                       int clear_tables, int *cleared, dmm_stream_t stream, void *tape = nullptr, int *taped = nullptr);
// the training call's solver tape (dmm_solve.hip): bytes (0 = not taped), and the backward that walks it
size_t relax_tape_bytes(int B, int N, int M, int max_iter, int proj_iter);
int relax_match_bwd_launch(const float *sim, const float *score_p, int B, int N, int M, const int32_t *n_valid,
                           const int32_t *m_valid, int max_iter, int proj_iter, float lr, int is_test, const float *dRb,
                           const float *d_match_score, const float *d_det_score, float *dsim_out, void *workspace,
                           size_t workspace_bytes, const void *fwd_tape, const float *R_saved, const int32_t *iters_saved,
                           dmm_stream_t stream);

// General forms for tables outside the compiled envelope (dmm_wide.hip): any N, M; the solver keeps its state in
// `scratch` (B x wide_scratch_floats(M, max(N, M + 1)) floats).
size_t wide_scratch_floats(int M, int PpS);
int launch_cosine_wide(const float *featn_t, const float *featn_p, int B, int N, int M, int D, const int32_t *n_valid,
                       const int32_t *m_valid, float *cos_out, hipStream_t stream);
int launch_relax_match_wide(const SolveIn &in, float w_feat, float w_iou, RelaxParams prm, int is_test, const SolveOut &out,
                            float *scratch, hipStream_t stream);

// backward of the solver at any table size (dmm_wide.hip): workspace bytes PER FRAME, and the launch
size_t wide_bwd_bytes(int N, int M, int max_iter, int proj_iter);
int launch_relax_match_bwd_wide(const float *sim, const float *score_p, int B, int N, int M, const int32_t *n_valid,
                                const int32_t *m_valid, RelaxParams prm, int is_test, const float *dRb, const float *dms,
                                const float *dds, float *dsim_out, void *workspace, hipStream_t stream);

// dmm_lsap.hip: dmm_hungarian_match_f32 on the bundles, and status [B] = 0 on `stream` (the Hungarian entries' answer for
// a call without templates)
int hungarian_match_launch(const SolveIn &in, float score_weight, const SolveOut &out, int32_t *status, dmm_stream_t stream);
int lsap_zero_status(int32_t *status, int B, dmm_stream_t stream);

// Threads per workgroup: the one-wave solver gets a second wave (the cost-norm helper, norm_helper_wave) while few frames
// are in flight -- two waves per frame then still sit on different SIMDs; DMM_OPT_SOLVER_HELPER_MAX (default 512 frames,
// 0 = never) moves the switch.
static inline int solver_block(int ng, int B) {
    if (ng != 1) return 64 * ng;
    const int helper_max = opt(DMM_OPT_SOLVER_HELPER_MAX);
    return B <= helper_max ? 128 : 64;
}

}  // namespace dmm

// Kernel selection: exact-row-count instantiations for the common small problems (one wave per
// frame), guarded generic ones (MT in {8,16,32}) otherwise.
#define DMM_DISPATCH_SOLVER(M_, W_, EXACT_OK, CALL)                                                          \
    do {                                                                                                     \
        const int ng_ = ((W_) + 63) / 64;                                                                    \
        if (ng_ <= 1 && (EXACT_OK)) {                                                                        \
            switch (M_) {                                                                                    \
                case 1: CALL(1, 1, true); break;   case 2: CALL(2, 1, true); break;                          \
                case 3: CALL(3, 1, true); break;   case 4: CALL(4, 1, true); break;                          \
                case 5: CALL(5, 1, true); break;   case 6: CALL(6, 1, true); break;                          \
                case 7: CALL(7, 1, true); break;   case 8: CALL(8, 1, true); break;                          \
                case 9: CALL(9, 1, true); break;   case 10: CALL(10, 1, true); break;                        \
                case 11: CALL(11, 1, true); break; case 12: CALL(12, 1, true); break;                        \
                case 13: CALL(13, 1, true); break; case 14: CALL(14, 1, true); break;                        \
                case 15: CALL(15, 1, true); break; case 16: CALL(16, 1, true); break;                        \
                default: CALL(32, 1, false); break;                                                          \
            }                                                                                                \
        } else if (ng_ <= 1) {                                                                               \
            if ((M_) <= 8) CALL(8, 1, false); else if ((M_) <= 16) CALL(16, 1, false); else CALL(32, 1, false); \
        } else if (ng_ == 2) {                                                                               \
            if ((M_) <= 8) CALL(8, 2, false); else if ((M_) <= 16) CALL(16, 2, false); else CALL(32, 2, false); \
        } else {                                                                                             \
            if ((M_) <= 8) CALL(8, 4, false); else if ((M_) <= 16) CALL(16, 4, false);                       \
            else if ((M_) == 20 && (EXACT_OK)) CALL(20, 4, true); else CALL(32, 4, false);                   \
        }                                                                                                    \
    } while (0)

