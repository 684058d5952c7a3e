/*
 * dmm_match.h -- C ABI of libdmm_match.so: the MI355X (gfx950) implementation of DMM-Net's
 * differentiable mask-matching layer.
 *
 * Drop-in boundary.  The reference (ZENGXH/DMM_Net) is pure Python; its matching layer is
 *   dmm/modules/match_model.py:13-152   class MatchModel (forward :24-47)
 *   dmm/utils/match_helper.py:9-64      pairwise mask IoU, cosine, matching loss
 *   dmm/modules/submodules/relax_match.py:9-105   relax_matching (PGD + Dykstra projections)
 * and it reaches native code only through torch ops.  The entry points below are what a
 * ctypes / cpp_extension binding of that layer calls instead of those torch ops; each one
 * names the reference lines it replaces.  See INTEGRATION.md for the reference-side stub.
 *
 * Conventions
 *  - plain C: raw DEVICE pointers, sizes, element strides, a hipStream_t passed as void*;
 *    no torch types, no exceptions; every function returns a dmm_status (0 = ok);
 *  - nothing is allocated: outputs and workspace are caller provided (dmm_workspace_bytes);
 *  - everything is enqueued on `stream` and is hipGraph-capturable (no host syncs);
 *  - batched: B independent frames per call.  B = 1 reproduces one reference call;
 *    N = proposals (reference "P"), M = templates (reference "O"), Pp = max(N, M+1) is the
 *    padded solver width (match_model.py:109-113), HW = H*W pixels of one mask plane;
 *  - ragged batches: n_valid[B] / m_valid[B] (device int32, may be NULL) give the number of
 *    live proposals / templates of each frame (<= N, <= M); tables keep the N/M/Pp strides;
 *    frames with m_valid == 0 or n_valid == 0 produce zeros (dmm_model.py:118-122);
 *  - a mask plane is H*W contiguous elements; planes / frames may be strided (in elements);
 *  - integer results are bit exact w.r.t. the reference; fp32 results follow the reference's
 *    op order with fp contraction disabled (sums use a fixed tree order).
 */
#ifndef DMM_MATCH_H
#define DMM_MATCH_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DMM_ABI_VERSION 2

typedef enum dmm_status {
    DMM_OK = 0,
    DMM_ERR_BAD_ARG = 1,      /* null pointer / negative size / inconsistent shape */
    DMM_ERR_UNSUPPORTED = 2,  /* shape outside the compiled kernel envelope          */
    DMM_ERR_LAUNCH = 3,       /* HIP reported an error; see dmm_last_hip_error()     */
    DMM_ERR_WORKSPACE = 4     /* workspace too small                                 */
} dmm_status;

typedef enum dmm_dtype {
    DMM_F32 = 0, DMM_F16 = 1, DMM_BF16 = 2,
    DMM_PACKED1 = 3   /* 1 bit per pixel, already thresholded; uint64 words in the library's ballot layout (see (1c)) */
} dmm_dtype;

typedef void *dmm_stream_t; /* hipStream_t */

#define DMM_API __attribute__((visibility("default")))

/* Envelope of the FAST kernels: the solver keeps a frame's table in registers (M rows, Pp = max(N, M+1) columns).
 * DMM-Net's configurations sit well inside it (<= 100 proposals, a handful of objects).  The reference itself is
 * unbounded (relax_match.py:36-105), and so is the layer here, FORWARD AND BACKWARD: dmm_match_forward (5), dmm_cosine_f32
 * (2), dmm_mask_mix* (4), dmm_mask_mix_bwd, dmm_relax_match_bwd_f32 (its workspace holds the general kernel's state: ask
 * dmm_relax_bwd_workspace_bytes) and dmm_feature_sim_bwd_f32 take ANY N and M -- beyond the envelope through general kernels
 * (same operations in the same order, bit identical to the reference's CPU path in the forward; written for correctness,
 * not speed), dmm_iou_counts_* tiles any N x M.  The granular solver entries dmm_relax_match_f32 / _f16s / dmm_relax_solve_*
 * (no argument to hold the general solver's state: use dmm_relax_match_any_f32 (3d)), the 1-bit forms (5b) / (5c) and the
 * frame-step entries keep the envelope and answer DMM_ERR_UNSUPPORTED outside it. */
#define DMM_MAX_TEMPLATES 32  /* M  */
#define DMM_MAX_PROPOSALS 256 /* Pp */

/* Frame-stride sentinel of the entries that take (masks_p, sp_b): with sp_b == DMM_FRAME_TABLE, masks_p is a DEVICE array of
 * B pointers to each frame's first proposal plane (what the *_frames entries of (1d) / (4c) pass on) instead of the base
 * of B equally spaced frames. */
#define DMM_FRAME_TABLE INT64_MIN

/* ---------------------------------------------------------------------------------------------
 * (0) Dispatch options.  Where an entry point has two kernels (or a tuning value worth A/B-ing) the choice is a
 * process-wide integer set THROUGH THIS ABI.  The library never reads the environment: a stray variable cannot change what
 * production dispatches.  Defaults are the measured best; NO option changes a result (the parity tests pin each
 * alternative and compare bit for bit).  dmm_set_option answers DMM_ERR_BAD_ARG for an unknown option or a value outside
 * its range; dmm_get_option returns INT_MIN for an unknown option; dmm_reset_options restores every default.
 * Options are read at launch time: set them before the calls they should affect (they are not captured by value in
 * a HIP graph -- a captured launch keeps the choice it was captured with).
 * ------------------------------------------------------------------------------------------- */
typedef enum dmm_option {
    DMM_OPT_COST_KERNEL = 0,        /* dmm_iou_counts*: -1 by shape (default), 0 register tiles, 1 template lanes          */
    DMM_OPT_COST_TINY_FRAMES = 1,   /* largest B that takes the short-chunk instantiation of the register-tile kernel (8) */
    DMM_OPT_SOLVER_KERNEL = 2,      /* dmm_relax_*: -1 by shape (default), 0 thread per column, 1 row split               */
    DMM_OPT_FORCE_WIDE = 3,         /* 1: the any-size kernels also inside the fast envelope (0)                          */
    DMM_OPT_COSINE_KERNEL = 4,      /* fused feature similarity: 0 D over the lanes (default), 1 one thread per output    */
    DMM_OPT_COST_WGS = 5,           /* workgroup targets of the count kernels: register tiles (8192),                     */
    DMM_OPT_COST_SMALL_WGS = 6,     /*   sub-tiling threshold of small launches (512),                                     */
    DMM_OPT_COST_TL_WGS = 7,        /*   template lanes (512)                                                              */
    DMM_OPT_COST_XCD = 8,           /* XCD-aware workgroup -> (frame, range) mapping of the count kernels (1)              */
    DMM_OPT_MIX_XCD = 9,            /*   ... of the mix kernels, bits: 1 row kernel, 2 union kernel, 4 union backward (3)  */
    DMM_OPT_MIX_WGS = 10,           /* mix kernel: workgroup target (320000),                                              */
    DMM_OPT_MIX_STEPQ = 11,         /*   steps per workgroup quantum (2),                                                  */
    DMM_OPT_MIX_ALIGN = 12,         /*   store alignment in bytes: 16 / 32 / 64 / 128 (128),                               */
    DMM_OPT_MIX_NT = 13,            /*   non-temporal loads (bit 0) / stores (bit 1) (3)                                   */
    DMM_OPT_SOLVER_HELPER_MAX = 14, /* largest B whose one-wave solver launches carry the cost-norm helper wave (512)      */
    DMM_OPT_NMS_WAVE = 15,          /* dmm_nms_slots_f32: 1 the one-workgroup kernel for <= 64 boxes (default), 0 general  */
    DMM_OPT_COS_ROWS_MIN_N = 16,    /* dmm_cosine_f32: from which N the row-blocked form is used (65)                      */
    DMM_OPT_GEMM_TUNE = 17,         /* dmm_conv1x1_bf16: hipBLASLt heuristic candidates timed per new shape (1 = none)     */
    DMM_OPT_PACK_VARIANT = 18,      /* dmm_pack_masks: 4 = 128-block segments x 8 loads (default), 0 = 256 x 4             */
    DMM_OPT_SMALL_FUSED = 19,       /* dmm_match_forward, a handful of dense frames: 1 = the feature similarity rides in the
                                       count launch (similarity workgroups beside count workgroups; default), 0 = two launches */
    DMM_OPT_MIX_SHARED = 20,        /* mix / mix backward: -1 by entry point (default: dmm_mask_mix_shared_* and the backward
                                       stream the union of the rows' planes once), 0 row kernels always, 1 union kernels always */
    DMM_OPT_MIX_SHARED_STEPS = 21,  /* union kernels: 4 KiB steps of every plane per workgroup (1)                         */
    DMM_OPT_FEAT_BWD_FRAME = 22,    /* dmm_feature_sim_bwd_f32: -1 by batch size (default: one WAVE per feature row up to 256 frames,
                                       one workgroup per frame beyond), 2 / 1 / 0: wave per row / per frame / workgroup per row  */
    DMM_OPT_MIX_SHARED_LOCKSTEP = 23, /* union kernels: 1 = one workgroup barrier per group of 8 planes keeps the four waves (four
                                       neighbouring 1 KiB pieces of every plane) in step (default: the lines the pieces share are
                                       then asked for at the same time, -2 % traffic), 0 = free-running waves                  */
    DMM_OPT_COUNT = 24
} dmm_option;
DMM_API int dmm_set_option(int option, int value);
DMM_API int dmm_get_option(int option);
DMM_API int dmm_reset_options(void);

DMM_API int dmm_abi_version(void);
DMM_API const char *dmm_status_string(int status);
DMM_API int dmm_last_hip_error(void);         /* hipError_t of the last DMM_ERR_LAUNCH on this thread */
DMM_API const char *dmm_build_info(void);     /* "gfx950 ..." */
/* Diagnostic: kernels this library has enqueued in this process so far (every launch, the table-clearing ones included;
 * a replayed HIP graph is not counted again).  bench.py reports launches per call from differences of it. */
DMM_API long long dmm_launch_count(void);

/* ---------------------------------------------------------------------------------------------
 * (1) Pairwise binary-mask intersection / area tables.
 * Replaces compute_iou_binary_mask_2D over the expanded [O*P, HW] tensors
 * (match_helper.py:9-28 as called from match_model.py:83-89, and from
 * compute_matching_loss match_helper.py:34-43 with masks_t = targets).
 *   a = x > 0.5 (strict);  inter[b,m,n] = |T_m & P_n|;  area_p[b,n] = |P_n|;  area_t[b,m] = |T_m|
 * (union = area_p + area_t - inter).  Outputs are int32 and are overwritten.
 * masks_p: N planes per frame, plane stride sp_n, frame stride sp_b (elements);
 * masks_t: M planes per frame, strides st_m / st_b.
 * ------------------------------------------------------------------------------------------- */
DMM_API int dmm_iou_counts(const void *masks_p, const void *masks_t, int dtype, int B, int N, int M, int HW,
                   int64_t sp_b, int64_t sp_n, int64_t st_b, int64_t st_m,
                   const int32_t *n_valid, const int32_t *m_valid,
                   int32_t *inter /*[B,M,N]*/, int32_t *area_p /*[B,N]*/, int32_t *area_t /*[B,M]*/,
                   dmm_stream_t stream);

/* (1c) Bit-packed planes.  dmm_pack_masks thresholds (x > 0.5) and packs `planes` mask planes of HW pixels into
 * 4*ceil(HW/256) uint64 words each (ballot layout: bit l of word 4q+k = pixel 256q + 4l + k; pad bits 0);
 * dmm_pack_words(HW) returns that word count.  dmm_iou_counts / dmm_iou_counts_dual accept dtype DMM_PACKED1:
 * masks_* then point to such words and all strides are in WORDS.  Packing the proposal side once (or having
 * dmm_paste_masks_f32 emit it) shrinks the bytes of the cost pass 32x for those planes; the integer tables are
 * identical to the fp32 path by construction. */
DMM_API int64_t dmm_pack_words(int HW);
DMM_API int dmm_pack_masks(const void *masks, int dtype, int64_t planes, int HW, int64_t plane_stride,
                           uint64_t *packed, int64_t packed_stride, dmm_stream_t stream);

/* (1b) Training: the same pass also intersects the proposals with a SECOND template set of M planes per
 * frame -- the ground-truth targets of compute_matching_loss (match_helper.py:34-43) -- so the proposal
 * planes (the bulk of the bytes) are streamed once instead of twice.  inter2 [B,M,N], area_t2 [B,M]. */
DMM_API int dmm_iou_counts_dual(const void *masks_p, const void *masks_t, const void *masks_t2, int dtype, int B,
                                int N, int M, int HW, int64_t sp_b, int64_t sp_n, int64_t st_b, int64_t st_m,
                                int64_t st2_b, int64_t st2_m, const int32_t *n_valid, const int32_t *m_valid,
                                int32_t *inter, int32_t *area_p, int32_t *area_t, int32_t *inter2, int32_t *area_t2,
                                dmm_stream_t stream);

/* (1d) / (4c) PER-FRAME POINTER TABLES for the proposal planes.  The reference's driver holds the proposal masks
 * of a step as one tensor PER VIDEO (`prop_m[bid] = proposals[bid].get_field('mask').squeeze(1)`,
 * dmm/modules/dmm_model.py:58 / :111) and loops over them (:62 / :115).  The *_frames entry points take a DEVICE
 * array of B pointers -- masks_p_frames[b] = first plane of frame b, N_b planes at stride sp_n -- instead of
 * (masks_p, sp_b), so all videos go through one launch WITHOUT first being copied into a [B,Nmax,H,W] batch
 * (that copy moved 2 x 13 MB per video in front of a 15.6 MB cost pass).  Everything else as in (1), (1b), (4), (4b). */
DMM_API int dmm_iou_counts_frames(const void *const *masks_p_frames, const void *masks_t, int dtype, int B, int N,
                                  int M, int HW, int64_t sp_n, int64_t st_b, int64_t st_m, const int32_t *n_valid,
                                  const int32_t *m_valid, int32_t *inter, int32_t *area_p, int32_t *area_t,
                                  dmm_stream_t stream);
DMM_API int dmm_iou_counts_dual_frames(const void *const *masks_p_frames, const void *masks_t, const void *masks_t2,
                                       int dtype, int B, int N, int M, int HW, int64_t sp_n, int64_t st_b,
                                       int64_t st_m, int64_t st2_b, int64_t st2_m, const int32_t *n_valid,
                                       const int32_t *m_valid, int32_t *inter, int32_t *area_p, int32_t *area_t,
                                       int32_t *inter2, int32_t *area_t2, dmm_stream_t stream);
DMM_API int dmm_mask_mix_frames(const float *Rb, const void *const *masks_p_frames, int dtype, int B, int N, int M,
                                int Pp, int HW, int64_t sp_n, const int32_t *n_valid, const int32_t *m_valid,
                                float *out, int64_t so_b, int64_t so_m, dmm_stream_t stream);
DMM_API int dmm_mask_mix_bwd_frames(const float *Rb, const void *const *masks_p_frames, int dtype, const float *dout,
                                    int B, int N, int M, int Pp, int HW, int64_t sp_n, const int32_t *n_valid,
                                    const int32_t *m_valid, float *dRb, dmm_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * (2) Row-normalise feature vectors: out[r,:] = in[r,:] / max(||in[r,:]||_2, 1e-8).
 * First half of F.cosine_similarity as get_cosine_score uses it (match_helper.py:51-64).
 * Also returns the clamped norms (needed by the backward).  rows = B*N or B*M.
 * ------------------------------------------------------------------------------------------- */
DMM_API int dmm_feature_normalize_f32(const float *in, int64_t rows, int D, float *out /*[rows,D]*/,
                              float *norms /*[rows] or NULL*/, dmm_stream_t stream);

/* (2c) get_cosine_score (match_helper.py:51-64) from the RAW features in one launch: (2) for both inputs + (2b), bit
 * identical to that sequence.  Dense batches only, N >= 2, D % 64 == 0.  D = 256 / 512 / 1024 (the product's 4 x
 * hidden_size) runs with the D axis spread over the lanes of a wave (dmm_cosine_lanes.hip); any other D with one thread
 * per output, the proposal columns tiled so that a tile plus the M template rows fit the LDS ((nt + M) * (D + 4) * 4
 * bytes <= 160 KB).  DMM_ERR_UNSUPPORTED when not even one column does (callers then run (2), (2), (2b)).  Used by (5). */
DMM_API int dmm_cosine_features_f32(const float *feat_t /*[B,M,D]*/, const float *feat_p /*[B,N,D]*/, int B, int N,
                                    int M, int D, float *cos_out /*[B,M,N]*/, dmm_stream_t stream);

/* (2d) Backward of the feature similarity: d/d feat_t, d/d feat_p of  sum(dsim * sim) + sum_b d_loss[b] * cost_loss[b],
 * i.e. torch autograd through get_cosine_score (match_helper.py:51-64), the (1 - score_weight) mix (match_model.py:90)
 * and compute_matching_loss's mse (match_helper.py:48).  featn_* / norm_* are the outputs of (2) saved by the forward;
 * gt [B,M,N] (greedy one-hot, no gradient), cos and d_loss [B] may be NULL together (inference-style loss-free call).
 * One launch; compared with the reference's autograd at 2e-5 relative to the largest gradient entry (tests). */
DMM_API int dmm_feature_sim_bwd_f32(const float *dsim /*[B,M,N]*/, const float *cos /*[B,M,N]*/, const float *gt,
                                    const float *d_loss, float score_weight, const float *feat_t, const float *feat_p,
                                    const float *featn_t, const float *featn_p, const float *norm_t, const float *norm_p,
                                    int B, int N, int M, int D, const int32_t *n_valid, const int32_t *m_valid,
                                    float *g_feat_t /*[B,M,D]*/, float *g_feat_p /*[B,N,D]*/, dmm_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * (2b) Cosine table of normalised rows: cos[b,m,n] = <featn_t[b,m,:], featn_p[b,n,:]>
 * (second half of F.cosine_similarity, match_helper.py:59-63; == MatchModel's feature_sim for a
 * single template-feature entry, match_model.py:71-76).  featn_* come from (2).  M <= 32.
 * ------------------------------------------------------------------------------------------- */
DMM_API int dmm_cosine_f32(const float *featn_t /*[B,M,D]*/, const float *featn_p /*[B,N,D]*/, int B, int N, int M,
                           int D, const int32_t *n_valid, const int32_t *m_valid, float *cos_out /*[B,M,N]*/,
                           dmm_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * (3) Similarity mix + relaxed assignment + scores, one frame per wave(-group), solver state
 * resident in registers for all iterations.  Replaces, per frame:
 *   iou = inter / (union + 1e-6);  sim = (1-w)*feature_sim + w*iou      match_model.py:89-90
 *   pad to [M, Pp];  C = -sim_pad                                      match_model.py:107-116
 *   relax_matching(C, max_iter, proj_iter, lr) and R = mean(X_list)
 *                                       relax_match.py:36-105, match_model.py:118-121
 *   logic = (R == rowmax) if is_test else (R > 0.01);  Rb = R*logic    match_model.py:124-130
 *   match_score = max_p clamp(R,0,1)*sim_pad;  det_score = sum_p score_p*Rb     :146-147
 * cos_in [B,M,N] is feature_sim (from (2b)).
 * Outputs: sim [B,M,N], R (may be NULL) / Rb [B,M,Pp], match_score / det_score [B,M],
 * iters (may be NULL) [B] = executed outer iterations (len(X_list)-1), X_final (may be NULL)
 * [B,M,Pp].  Requires M <= DMM_MAX_TEMPLATES and Pp <= DMM_MAX_PROPOSALS.
 * ------------------------------------------------------------------------------------------- */
DMM_API int dmm_relax_match_f32(const float *cos_in, const int32_t *inter, const int32_t *area_p,
                                const int32_t *area_t, const float *score_p /*[B,N]*/, int B, int N, int M,
                                const int32_t *n_valid, const int32_t *m_valid,
                                float score_weight, int max_iter, int proj_iter, float lr, int is_test,
                                float *sim_out, float *R_out, float *Rb_out,
                                float *match_score, float *det_score, int32_t *iters_out, float *X_final,
                                dmm_stream_t stream);

/* (3d) The same for ANY N and M (the reference's relax_matching is unbounded, relax_match.py:36-105): outside the fast
 * kernels' envelope the general solver keeps its state -- 9 tables of M x Pp floats per frame -- in `scratch`
 * (>= dmm_relax_any_scratch_bytes(B, N, M)); inside the envelope this is (3) and the scratch is not touched.  Same
 * outputs, bit identical to the reference's CPU path at every size. */
DMM_API size_t dmm_relax_any_scratch_bytes(int B, int N, int M);
DMM_API int dmm_relax_match_any_f32(const float *cos_in, const int32_t *inter, const int32_t *area_p,
                                    const int32_t *area_t, const float *score_p, int B, int N, int M,
                                    const int32_t *n_valid, const int32_t *m_valid, float score_weight, int max_iter,
                                    int proj_iter, float lr, int is_test, float *sim_out, float *R_out, float *Rb_out,
                                    float *match_score, float *det_score, int32_t *iters_out, float *X_final,
                                    void *scratch, size_t scratch_bytes, dmm_stream_t stream);

/* (3c) The same with the solver STATE in packed fp16 and every sum in fp32 -- BASELINE configs[4]'s "fp16 Sinkhorn with
 * fp32 accumulate".  A TOLERANCE mode, opt-in: the default (dmm_relax_match_f32) reproduces the reference bit for bit
 * including its exact-equality exits (relax_match.py:88-89, :96-98); here the iteration runs on fp16 iterates, so R is
 * within 1e-2 of the fp32 result (2.5e-3 measured on the config-2 / config-5 shapes) while both execute the same number of iterations, the row argmax is the same wherever
 * the fp32 decision is not a near tie, and the exits fire at the fp16 iteration's own fixed point.  What it buys: the
 * 20 x 200 problem needs <= 128 VGPRs (fp32: 256 + spills), four waves per SIMD, so the solver runs beside the streaming
 * cost / mix kernels instead of serialising with them. */
DMM_API int dmm_relax_match_f16s(const float *cos_in, const int32_t *inter, const int32_t *area_p,
                                 const int32_t *area_t, const float *score_p /*[B,N]*/, int B, int N, int M,
                                 const int32_t *n_valid, const int32_t *m_valid,
                                 float score_weight, int max_iter, int proj_iter, float lr, int is_test,
                                 float *sim_out, float *R_out, float *Rb_out,
                                 float *match_score, float *det_score, int32_t *iters_out, float *X_final,
                                 dmm_stream_t stream);

/* Solver only, on caller-provided cost matrices C [B,n,m] (relax_matching itself,
 * relax_match.py:36-105; with max_iter = 0 it is the greedy initialisation used by
 * compute_matching_loss, match_helper.py:44): X_final, R = mean(X_list), cost list [B,max_iter+1]
 * (may be NULL), iters [B].  rows_valid / cols_valid [B] (may be NULL) restrict frame b to its top-left
 * [rows_valid[b], cols_valid[b]] block (the rest of X_final / R is zero filled).
 * n <= DMM_MAX_TEMPLATES, m <= DMM_MAX_PROPOSALS. */
DMM_API int dmm_relax_solve_f32(const float *C, int B, int n, int m, const int32_t *rows_valid,
                                const int32_t *cols_valid, int max_iter, int proj_iter, float lr,
                                float *X_final, float *R_out, float *cost_out, int32_t *iters_out,
                                dmm_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * (3e) Exact linear sum assignment (the reference's algo 'hun', match_model.py:122-123: scipy.optimize.
 * linear_sum_assignment, Crouse's shortest augmenting path in fp64).  One wave per frame; the same assignment as scipy
 * on every input, ties included.  C [B,nr,nc]: frame b solves its top-left [rows_valid[b], cols_valid[b]] block
 * (NULL = all), a block with more live rows than live columns through its transpose, as scipy does.
 * Outputs: X [B,nr,nc] one-hot (may be NULL), col4row [B,nr] with -1 for an unassigned row (may be NULL), status [B]:
 * 0 ok, 1 a NaN or -inf entry (scipy: "invalid numeric entries"), 2 no complete assignment (scipy: "cost matrix is
 * infeasible"); the outputs of such a frame are zero (-1).  Requires nr <= nc, nr <= DMM_MAX_TEMPLATES and
 * nc <= DMM_MAX_PROPOSALS (DMM_ERR_UNSUPPORTED otherwise).
 * ------------------------------------------------------------------------------------------- */
DMM_API int dmm_lsap_f32(const float *C, int B, int nr, int nc, const int32_t *rows_valid, const int32_t *cols_valid,
                         float *X, int32_t *col4row, int32_t *status, dmm_stream_t stream);

/* (3f) (3) with the assignment of (3e) in place of the relaxed solver: sim exactly as (3) computes it, C = -sim padded
 * with -0.0 to each frame's live width Pp_b = max(n_b, m_b + 1), R = Rb = the one-hot assignment [B,M,Pp] (R may be
 * NULL), match_score = max_p clamp(R,0,1)*sim_pad, det_score = sum_p score_p*Rb [B,M], status [B] as in (3e).  Same
 * envelope as (3). */
DMM_API int dmm_hungarian_match_f32(const float *cos_in, const int32_t *inter, const int32_t *area_p,
                                    const int32_t *area_t, const float *score_p, int B, int N, int M,
                                    const int32_t *n_valid, const int32_t *m_valid, float score_weight, int is_test,
                                    float *sim_out, float *R_out, float *Rb_out, float *match_score, float *det_score,
                                    int32_t *status, dmm_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * (3b) Backward of (3) with respect to sim (the reference gets it from torch autograd through
 * relax_match.py:68-98 and match_model.py:121-147; the greedy init, the masks and the early exits
 * carry no gradient).  The kernel re-runs the forward solver from the saved `sim` (same code, hence
 * the same iterates and exits), tapes 1 relu bit per element + 1 column bit per sweep into
 * `workspace`, and walks the tape backwards.
 *   dRb [B,M,Pp]        upstream gradient of Rb (= dOut @ masks_p^T; logic is applied inside); may be NULL
 *   d_match_score, d_det_score [B,M]   upstream gradients of the two score vectors; may be NULL
 *   dsim_out [B,M,N]    gradient of the loss w.r.t. sim (feature_sim gets (1-w) * dsim)
 * workspace >= dmm_relax_bwd_workspace_bytes(...).  max_iter <= 1024.
 * ------------------------------------------------------------------------------------------- */
DMM_API size_t dmm_relax_bwd_workspace_bytes(int B, int N, int M, int max_iter, int proj_iter);

DMM_API int dmm_relax_match_bwd_f32(const float *sim, const float *score_p, int B, int N, int M,
                                    const int32_t *n_valid, const int32_t *m_valid,
                                    int max_iter, int proj_iter, float lr, int is_test,
                                    const float *dRb, const float *d_match_score, const float *d_det_score,
                                    float *dsim_out, void *workspace, size_t workspace_bytes,
                                    dmm_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * (4) Assignment-weighted mask mix: full_outmask[b,m,:] = sum_n Rb[b,m,n] * masks_p[b,n,:]
 * (torch.mm at match_model.py:144; padded columns n >= N carry zero planes, :134-142).
 * Only planes with a non-zero weight are read (in test mode <= M planes per frame).
 * Rb is [B,M,Pp] with row stride Pp.  out: [B,M,HW] fp32, strides so_b / so_m (elements).
 * Rows m >= m_valid[b] are zero filled.
 * ------------------------------------------------------------------------------------------- */
DMM_API int dmm_mask_mix(const float *Rb, const void *masks_p, int dtype, int B, int N, int M, int Pp, int HW,
                 int64_t sp_b, int64_t sp_n, const int32_t *n_valid, const int32_t *m_valid,
                 float *out, int64_t so_b, int64_t so_m, dmm_stream_t stream);

/* (4a) Same with a choice of the output element type: DMM_F32, or the planes' own 16-bit type (dtype) -- BASELINE
 * config 5 keeps the masks in fp16: the matched masks are the next frame's templates (mask_last_occurence,
 * dmm_model.py:78-80), so they are written back in the storage type (the fp32 result rounded once, nearest-even).
 * out strides so_b / so_m are in OUTPUT elements. */
DMM_API int dmm_mask_mix_to(const float *Rb, const void *masks_p, int dtype, int B, int N, int M, int Pp, int HW,
                            int64_t sp_b, int64_t sp_n, const int32_t *n_valid, const int32_t *m_valid, void *out,
                            int out_dtype, int64_t so_b, int64_t so_m, dmm_stream_t stream);

/* (4d) dmm_mask_mix_to for weight tables whose ROWS SHARE PLANES -- train mode: logic = (R > 0.01) keeps many entries per
 * row (match_model.py:126-129), torch.mm then reads every plane once for all rows (:144).  One workgroup streams each
 * plane of the union of the rows' supports once and fans it into the rows; per row the accumulation is the one of
 * dmm_mask_mix_to (non-zero weights in ascending column order), so the two entries agree bit for bit.  M <= 32, N <= 256
 * take the union kernel, anything else the general one.  dmm_mask_mix_shared_frames: proposal planes as a device table of
 * per-frame base pointers (see (4c)). */
DMM_API int dmm_mask_mix_shared_to(const float *Rb, const void *masks_p, int dtype, int B, int N, int M, int Pp, int HW,
                                   int64_t sp_b, int64_t sp_n, const int32_t *n_valid, const int32_t *m_valid,
                                   void *out, int out_dtype, int64_t so_b, int64_t so_m, dmm_stream_t stream);
DMM_API int dmm_mask_mix_shared_frames(const float *Rb, const void *const *masks_p_frames, int dtype, int B, int N,
                                       int M, int Pp, int HW, int64_t sp_n, const int32_t *n_valid,
                                       const int32_t *m_valid, float *out, int64_t so_b, int64_t so_m,
                                       dmm_stream_t stream);

/* (4b) Backward of (4) w.r.t. Rb: dRb[b,m,n] = <dout[b,m,:], masks_p[b,n,:]> on the support of Rb (entries with
 * Rb == 0 were masked by the constant logic mask, match_model.py:124-130, and get 0).  dout: [B,M,HW] fp32
 * contiguous; dRb: [B,M,Pp] fp32, overwritten.  Only the selected planes are read. */
DMM_API int dmm_mask_mix_bwd(const float *Rb, const void *masks_p, int dtype, const float *dout, int B, int N, int M,
                             int Pp, int HW, int64_t sp_b, int64_t sp_n, const int32_t *n_valid,
                             const int32_t *m_valid, float *dRb, dmm_stream_t stream);
/* Deterministic forms of (4b) and its per-frame-table form: the same kernels and decomposition, but each workgroup stores its
 * per-pair partials to a slab plane of its own (workspace, zeroed by the entry) and one fixed-order fold writes dRb --
 * bit-identical run after run.  workspace: dmm_mask_mix_bwd_det_workspace_bytes(B, N, M, Pp, HW) bytes at the current dispatch
 * options (0: the table goes to the wide kernel, deterministic as it is, and no workspace is needed); shorter answers
 * DMM_ERR_WORKSPACE before anything is launched.  (5e) has a deterministic form of its own: dmm_match_train_backward_det. */
DMM_API size_t dmm_mask_mix_bwd_det_workspace_bytes(int B, int N, int M, int Pp, int HW);
DMM_API int dmm_mask_mix_bwd_det(const float *Rb, const void *masks_p, int dtype, const float *dout, int B, int N, int M,
                                 int Pp, int HW, int64_t sp_b, int64_t sp_n, const int32_t *n_valid, const int32_t *m_valid,
                                 float *dRb, void *workspace, size_t workspace_bytes, dmm_stream_t stream);
DMM_API int dmm_mask_mix_bwd_frames_det(const float *Rb, const void *const *masks_p_frames, int dtype, const float *dout,
                                        int B, int N, int M, int Pp, int HW, int64_t sp_n, const int32_t *n_valid,
                                        const int32_t *m_valid, float *dRb, void *workspace, size_t workspace_bytes,
                                        dmm_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * (5) The whole forward of MatchModel for B frames (match_model.py:24-47, targets=None):
 * (1) -> (2) -> (3) -> (4) on `stream`, intermediates in `workspace`.
 * Outputs as in (3)/(4).  workspace >= dmm_workspace_bytes(B, N, M, D).  Any N, M: outside the fast kernels' envelope
 * (M > 32 or max(N, M+1) > 256) the workspace also holds the general solver's state (9 tables of M x Pp floats per
 * frame; dmm_workspace_bytes accounts for it) and the general kernels run inside this call.
 * ------------------------------------------------------------------------------------------- */
DMM_API size_t dmm_workspace_bytes(int B, int N, int M, int D);

DMM_API int dmm_match_forward(const void *masks_p, const void *masks_t, int mask_dtype,
                      const float *feat_p /*[B,N,D]*/, const float *feat_t /*[B,M,D]*/,
                      const float *score_p /*[B,N]*/, int B, int N, int M, int HW, int D,
                      int64_t sp_b, int64_t sp_n, int64_t st_b, int64_t st_m,
                      const int32_t *n_valid, const int32_t *m_valid,
                      float score_weight, int max_iter, int proj_iter, float lr, int is_test,
                      float *full_outmask /*[B,M,HW]*/, float *match_score /*[B,M]*/,
                      float *det_score /*[B,M]*/, float *sim_out /*[B,M,N] or NULL*/,
                      float *R_out /*[B,M,Pp] or NULL*/, float *Rb_out /*[B,M,Pp] or NULL*/,
                      int32_t *iters_out /*[B] or NULL*/,
                      void *workspace, size_t workspace_bytes, dmm_stream_t stream);

/* (5a') dmm_match_forward for a caller that keeps ONE workspace over a sequence of calls (the per-frame use) and carries
 * the library's note about what it left there: *ws_state in = the value the previous call on this workspace wrote (same
 * B, N, M, D; DMM_WS_UNKNOWN for a fresh or otherwise touched workspace), out = the state the work enqueued by this call
 * leaves behind.  With DMM_WS_TABLES_ZERO a handful of dense frames run without a clearing launch in front of the IoU
 * counts (the solver zeroes each count-table entry right after reading it); results are the same either way.  The state
 * describes the workspace AFTER the enqueued work: calls that share a workspace must be ordered on one stream, and a
 * captured call must be replayed with the workspace in the state it was captured with (it is, if nothing else touches
 * the workspace between replays: a call that starts from DMM_WS_TABLES_ZERO and returns it leaves what it found).
 * ws_state == NULL: exactly dmm_match_forward.
 * The CALLER owns this note: reset it to DMM_WS_UNKNOWN whenever anything but the previous dmm_match_forward_ws call with
 * the same (B, N, M, D) may have written the workspace -- another shape (the carving moves), another entry point, a
 * re-allocation, a second stream or thread sharing it.  A stale DMM_WS_TABLES_ZERO makes the counts accumulate onto old
 * tables: a silently wrong result the library cannot detect.  (dmm_net_amd/ops.py keeps one note per (device, stream,
 * shape) and drops it on every such event; the dispatch options of (0) are process-wide and not part of this state.) */
enum { DMM_WS_UNKNOWN = 0, DMM_WS_TABLES_ZERO = 1 };
DMM_API int dmm_match_forward_ws(const void *masks_p, const void *masks_t, int mask_dtype, const float *feat_p,
                                 const float *feat_t, const float *score_p, int B, int N, int M, int HW, int D,
                                 int64_t sp_b, int64_t sp_n, int64_t st_b, int64_t st_m, const int32_t *n_valid,
                                 const int32_t *m_valid, float score_weight, int max_iter, int proj_iter, float lr,
                                 int is_test, float *full_outmask, float *match_score, float *det_score, float *sim_out,
                                 float *R_out, float *Rb_out, int32_t *iters_out, void *workspace, size_t workspace_bytes,
                                 int *ws_state, dmm_stream_t stream);

/* (5b) The same forward with the proposal side of the cost pass on 1-bit planes the caller already holds
 * (dmm_paste_masks_f32 / dmm_paste_kept_f32 emit them next to the soft planes): packed_p [B,N,words] uint64, strides
 * pk_b / pk_n in WORDS.  The M template planes of every frame are packed inside (st_b == M * st_m required), the counts
 * run on the words -- identical integer tables from 1/32 of the proposal bytes -- and the mix reads the soft planes.
 * The feature similarity runs in the one-launch kernel for all frames, each in the summation order of ITS live proposal
 * count (the reference is called per frame; ATen's order over the [D, P] products depends on P), template rows past m_valid
 * are computed and never read.
 * This is the per-frame call of the evaluator's loop (dmm_model.py:75-77 for all videos of the step at once).
 * workspace >= dmm_workspace_bytes_packed(B, N, M, D, HW). */
DMM_API size_t dmm_workspace_bytes_packed(int B, int N, int M, int D, int HW);
DMM_API int dmm_match_forward_packed(const void *masks_p, const uint64_t *packed_p, const void *masks_t, int mask_dtype,
                                     const float *feat_p, const float *feat_t, const float *score_p, int B, int N, int M,
                                     int HW, int D, int64_t sp_b, int64_t sp_n, int64_t pk_b, int64_t pk_n, int64_t st_b,
                                     int64_t st_m, const int32_t *n_valid, const int32_t *m_valid, float score_weight,
                                     int max_iter, int proj_iter, float lr, int is_test, float *full_outmask,
                                     float *match_score, float *det_score, float *sim_out, float *R_out, float *Rb_out,
                                     int32_t *iters_out, void *workspace, size_t workspace_bytes, dmm_stream_t stream);

/* (5c) Cost + assignment of a fixed-slot frame step with BOTH sides of the cost pass on 1-bit planes and no mix (the
 * mix is part of (8c)): packed_p [B,N,words] from dmm_paste_kept_f32, packed_t [B,M,words] from the previous frame's
 * dmm_step_finish_f32 (or dmm_pack_masks for the first frame), both dense.  cosine -> counts -> solver
 * (match_model.py:49-130, :146-147); Rb [B,M,Pp], match_score / det_score [B,M], sim (may be NULL), R (may be NULL),
 * iters (may be NULL).  workspace >= dmm_workspace_bytes(B, N, M, D). */
DMM_API int dmm_match_solve_packed(const uint64_t *packed_p, const uint64_t *packed_t, const float *feat_p,
                                   const float *feat_t, const float *score_p, int B, int N, int M, int HW, int D,
                                   const int32_t *n_valid, const int32_t *m_valid, float score_weight, int max_iter,
                                   int proj_iter, float lr, int is_test, float *Rb_out, float *match_score,
                                   float *det_score, float *sim_out, float *R_out, int32_t *iters_out, void *workspace,
                                   size_t workspace_bytes, dmm_stream_t stream);

/* (5c') (5c) with the assignment of (3f) in place of the relaxed solver (algo 'hun'): Rb [B,M,Pp] one-hot,
 * match_score / det_score [B,M], sim (may be NULL), R (may be NULL), status [B] as in (3e).
 * workspace >= dmm_workspace_bytes(B, N, M, D). */
DMM_API int dmm_match_solve_packed_hun(const uint64_t *packed_p, const uint64_t *packed_t, const float *feat_p,
                                       const float *feat_t, const float *score_p, int B, int N, int M, int HW, int D,
                                       const int32_t *n_valid, const int32_t *m_valid, float score_weight, int is_test,
                                       float *Rb_out, float *match_score, float *det_score, float *sim_out, float *R_out,
                                       int32_t *status, void *workspace, size_t workspace_bytes, dmm_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * (1e) The tail of compute_matching_loss (match_helper.py:43-48) on the device, after the counts of (1b):
 *   gt_iou = inter2 / (area_p + area_t2 - inter2 + 1e-6)  (compute_iou_binary_mask_2D on proposals x targets, :9-28, :43)
 *   gt     = relax_matching(-gt_iou, 0, 0, 0)[0]          (the greedy one-hot initialisation, relax_match.py:45-55; :44)
 *   loss   = F.mse_loss(feature_sim, gt)                   (:48; feature_sim = cos, BEFORE the IoU mix)
 * gt [B,M,N] (zeros outside a ragged frame's live [m_valid, n_valid] block), loss [B] (0 for a frame without live
 * templates or proposals, dmm_model.py:118-122).  One launch; N <= 8192, M <= 4096.
 * ------------------------------------------------------------------------------------------- */
DMM_API int dmm_matching_loss_f32(const int32_t *inter2 /*[B,M,N]*/, const int32_t *area_p /*[B,N]*/,
                                  const int32_t *area_t2 /*[B,M]*/, const float *cos /*[B,M,N]*/, int B, int N, int M,
                                  const int32_t *n_valid, const int32_t *m_valid, float *gt /*[B,M,N]*/,
                                  float *loss /*[B]*/, dmm_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * (5d) / (5e) The TRAINING call of the layer -- MatchModel.forward with targets as the trainer issues it once per (video,
 * frame), dmm_model.py:130-132, and torch autograd back through it -- as ONE entry each way, so that a one-frame call
 * costs the host two library calls instead of twelve (the drop-in was host bound there).
 *
 * dmm_match_train_forward: (2c) feature similarity -> (1b) counts against templates AND targets in one pass over the
 *   proposal planes (targets == NULL: (1) and no loss) -> (3) -> (4d) [is_test: (4)] -> (1e).  Same kernels, same results
 *   bit for bit as the granular entries.  sp_b may be DMM_FRAME_TABLE.  targets: M planes per frame of the masks' dtype,
 *   strides sg_b / sg_m.  Outputs full_outmask [B,M,HW] fp32 contiguous, match_score / det_score [B,M], cost_loss [B]
 *   (NULL without targets), iters [B] (may be NULL); and what (5e) needs: cos, sim [B,M,N], Rb [B,M,Pp], gt [B,M,N]
 *   (NULL without targets).  Inside the fast kernels' envelope only (DMM_ERR_UNSUPPORTED otherwise: wider tables train
 *   through the granular entries).  workspace >= dmm_match_train_forward_workspace_bytes(B, N, M, D).
 * dmm_match_train_backward: d/d feat_t, d/d feat_p of
 *     sum(d_full * full_outmask) + sum(d_match_score * match_score) + sum(d_det_score * det_score) + sum(d_loss * cost_loss)
 *   = (2) on both feature sets (one launch; the forward keeps no normalised rows) -> (4b) -> (3b) -> (2d).  Any of d_full
 *   [B,M,HW], d_match_score, d_det_score [B,M] may be NULL (no gradient from that output); gt / d_loss / cos NULL together
 *   (no loss term).  Any N, M.  workspace >= dmm_match_train_backward_workspace_bytes(B, N, M, D, max_iter, proj_iter).
 * The solver's TAPE (optional, both entries): the reference's autograd keeps every intermediate of relax_matching
 *   (relax_match.py:68-98) for its backward; (3b) alone re-runs the solver to rebuild what it needs.  Given a caller block
 *   `tape` of dmm_match_train_tape_bytes(B, N, M, max_iter, proj_iter) bytes (0 = this table is not taped: wider than 64 solver
 *   columns) and iters_out != NULL, the forward's solver kernel records it there (R, and per projection sweep and column 8
 *   bytes of gate bits) and sets *taped = 1; handed back with that flag and the forward's iters, the backward walks the
 *   records instead of re-running the solver (same gradient: the same gates).  tape == NULL / taped == 0: as before.
 * ------------------------------------------------------------------------------------------- */
DMM_API size_t dmm_match_train_tape_bytes(int B, int N, int M, int max_iter, int proj_iter);
DMM_API size_t dmm_match_train_forward_workspace_bytes(int B, int N, int M, int D);
DMM_API int dmm_match_train_forward(const void *masks_p, const void *masks_t, const void *targets, int mask_dtype,
                                    const float *feat_p, const float *feat_t, const float *score_p, int B, int N, int M,
                                    int HW, int D, int64_t sp_b, int64_t sp_n, int64_t st_b, int64_t st_m, int64_t sg_b,
                                    int64_t sg_m, const int32_t *n_valid, const int32_t *m_valid, float score_weight,
                                    int max_iter, int proj_iter, float lr, int is_test, float *full_outmask,
                                    float *match_score, float *det_score, float *cost_loss, int32_t *iters_out,
                                    float *cos_out, float *sim_out, float *Rb_out, float *gt_out, void *workspace,
                                    size_t workspace_bytes, void *tape, size_t tape_bytes, int *taped /* host, may be NULL */,
                                    dmm_stream_t stream);
DMM_API size_t dmm_match_train_backward_workspace_bytes(int B, int N, int M, int D, int max_iter, int proj_iter);
DMM_API int dmm_match_train_backward(const void *masks_p, int mask_dtype, const float *feat_p, const float *feat_t,
                                     const float *score_p, const float *cos, const float *sim, const float *Rb,
                                     const float *gt, const float *d_full, const float *d_match_score,
                                     const float *d_det_score, const float *d_loss, int B, int N, int M, int HW, int D,
                                     int64_t sp_b, int64_t sp_n, const int32_t *n_valid, const int32_t *m_valid,
                                     float score_weight, int max_iter, int proj_iter, float lr, int is_test,
                                     float *g_feat_t /*[B,M,D]*/, float *g_feat_p /*[B,N,D]*/, void *workspace,
                                     size_t workspace_bytes, const void *tape, const int32_t *iters /*[B], the forward's*/,
                                     int taped, dmm_stream_t stream);
/* (5e) deterministic form: the same arguments and results, bit-identical run after run -- its mix backward is
 * dmm_mask_mix_bwd_det, whose slab follows the (5e) workspace: dmm_match_train_backward_det_workspace_bytes bytes (takes HW). */
DMM_API size_t dmm_match_train_backward_det_workspace_bytes(int B, int N, int M, int D, int max_iter, int proj_iter, int HW);
DMM_API int dmm_match_train_backward_det(const void *masks_p, int mask_dtype, const float *feat_p, const float *feat_t,
                                         const float *score_p, const float *cosv, const float *sim, const float *Rb,
                                         const float *gt, const float *d_full, const float *d_match_score,
                                         const float *d_det_score, const float *d_loss, int B, int N, int M, int HW, int D,
                                         int64_t sp_b, int64_t sp_n, const int32_t *n_valid, const int32_t *m_valid,
                                         float score_weight, int max_iter, int proj_iter, float lr, int is_test,
                                         float *g_feat_t, float *g_feat_p, void *workspace, size_t workspace_bytes,
                                         const void *tape, const int32_t *iters, int taped, dmm_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * (6) Fused 4-level ROIAlign + spatial mean: the reference's ROI feature extractor
 * (dmm/modules/feature_extractor.py:20-52: maskrcnn_benchmark legacy ROIAlign, 14x14 bins,
 * sampling_ratio 2, at the four scales on EVERY roi, then .mean(4).mean(3) -> [R, 4*C]).
 * feat[l]: [B, C, H[l], W[l]] contiguous NCHW (dtype fp32 / fp16 / bf16), rois: [R,5] fp32
 * (batch index, x1, y1, x2, y2) in image coordinates, scale[l] = 1/stride.  out: [R, 4*C] fp32,
 * out[r, l*C + c].  The backward accumulates (fp32 atomics) into dfeat[l] (same shapes, fp32,
 * zeroed by the caller); boxes receive no gradient (as in maskrcnn_benchmark).
 * H[l], W[l] <= 1024.  No upstream fixture exists for this third-party op; forward and gradients are pinned against an
 * independent differentiable formulation of the published per-bin definition (tests/golden G12) and the oracle.
 * dmm_roialign4_mean_nhwc_fwd: the same forward on channels-last features, feat[l] = [B, H[l], W[l], C] contiguous (what
 * the inference encoder produces): 16-byte lane loads of contiguous channels.  Needs C % (16 / element size) == 0 with
 * the quotient a power of two <= 64 or a multiple of 64, 16-byte aligned bases; otherwise DMM_ERR_UNSUPPORTED.
 * ------------------------------------------------------------------------------------------- */
DMM_API int dmm_roialign4_mean_nhwc_fwd(const void *const feat[4], int dtype, int B, int C, const int H[4],
                                        const int W[4], const float scale[4], const float *rois, int R, float *out,
                                        dmm_stream_t stream);
DMM_API int dmm_roialign4_mean_fwd(const void *const feat[4], int dtype, int B, int C, const int H[4], const int W[4],
                                   const float scale[4], const float *rois, int R, float *out, dmm_stream_t stream);
DMM_API int dmm_roialign4_mean_bwd(const float *dout, int B, int C, const int H[4], const int W[4],
                                   const float scale[4], const float *rois, int R, float *const dfeat[4],
                                   dmm_stream_t stream);
/* Deterministic form of dmm_roialign4_mean_bwd (same arguments and the same accumulation into dfeat): a gather with no atomics,
 * each dfeat element computed once with its rois in ascending order -- bit-identical run after run.  workspace:
 * dmm_roialign4_mean_bwd_det_workspace_bytes(R, H, W) bytes (the rois' weight vectors and patch ranges; 0 when R <= 0 or a
 * level is outside the envelope); shorter answers DMM_ERR_WORKSPACE before anything is launched. */
DMM_API size_t dmm_roialign4_mean_bwd_det_workspace_bytes(int R, const int H[4], const int W[4]);
DMM_API int dmm_roialign4_mean_bwd_det(const float *dout, int B, int C, const int H[4], const int W[4], const float scale[4],
                                       const float *rois, int R, float *const dfeat[4], void *workspace, size_t workspace_bytes,
                                       dmm_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * (7) Proposal preprocessing (the step right before the path; host Python loops in the reference).
 * dmm_paste_masks_f32: paste_mask_in_image + binmask_to_box (dmm/utils/masker.py:110-173) for P proposals:
 *   prob [P,M,M] mask probabilities, boxes [P,4] xyxy -> planes [P, im_h*im_w] (plane_stride elements apart; the
 *   soft masks the matching layer consumes) and new_boxes [P,4] = tight box of (plane > thresh), or
 *   [0,0,im_h,im_w] when empty.  M + 2*padding <= 64.  Optionally also emits the DMM_PACKED1 form of the planes.
 * dmm_nms_f32: NMS + top-k of filter_results (dmm/utils/boxlist_ops.py:15-29, maskrcnn_benchmark nms semantics:
 *   descending score, legacy +1 areas, IoU > thresh suppresses) per image: boxes [sum n,4], scores [sum n],
 *   offsets [images+1] (device int32) -> keep[offsets[i] ...] = kept local indices in score order,
 *   keep_count[i].  max_per_image (<= 1024) bounds n.
 * ------------------------------------------------------------------------------------------- */
DMM_API int dmm_paste_masks_f32(const float *prob, int P, int M, const float *boxes, int im_h, int im_w, float thresh,
                                int padding, float *planes, int64_t plane_stride, float *new_boxes,
                                uint64_t *packed /* NULL or [P, dmm_pack_words(im_h*im_w)]: (plane > 0.5) bits */,
                                dmm_stream_t stream);
DMM_API int dmm_nms_f32(const float *boxes, const float *scores, const int32_t *offsets, int images, int max_per_image,
                        float thresh, int max_keep, int32_t *keep, int32_t *keep_count, dmm_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * (7b) The same preprocessing in TWO PHASES on FIXED SLOTS, with no host round trip: what the evaluator does per frame
 * before the layer (dmm/modules/model_encoder.py:115-134: Masker paste of every raw proposal, then filter_results =
 * NMS + top-k, dmm/utils/boxlist_ops.py:15-29, then BoxList indexing of the kept ones) without ever writing the planes
 * of proposals NMS drops and without gathering the kept ones into a new tensor.
 *   raw inputs: prob [.., images, R, M, M], boxes [.., images, R, 4] xyxy, scores [.., images, R], counts [.., images]
 *   (NULL = R each) -- the leading axis is the FRAME of a clip-resident buffer, selected by the DEVICE scalar *step
 *   (NULL = frame 0), so a captured graph can replay the frame step of every frame of a clip (see (8b));
 * dmm_proposal_boxes_f32: tight [images, R, 4] = box of (pasted value > thresh) of every raw proposal, [0,0,im_h,im_w]
 *   when nothing passes (masker.py:164), zeros for empty raw slots -- the values are evaluated, no plane is written;
 * dmm_nms_slots_f32: NMS(thresh) + top-K on the tight boxes -> keep [images, K] raw indices in descending score order,
 *   keep_count [images] (stays on the device: it is the n_valid of the matching entry points); R <= 1024;
 * dmm_paste_kept_f32: slot (i, k), k < keep_count[i], receives raw proposal keep[i, k]: its soft plane
 *   planes[(i*K + k) * plane_stride ..] (NULL = do not write soft planes, see (8c)), its 1-bit plane packed [images, K,
 *   dmm_pack_words] (may be NULL), kept_boxes
 *   [images, K, 4] (the tight box), kept_scores [images, K] and the ROIAlign row rois [images*K, 5] = (img_base[*step]
 *   + i, tight box) (each may be NULL; img_base NULL = 0).  Dead slots: plane untouched, score 0, box 0, roi image
 *   index -1 (dmm_roialign4_mean_fwd writes a zero feature row for it).
 * Bit identical to dmm_paste_masks_f32 + dmm_nms_f32 + gather (same device function evaluates every pasted value).
 * ------------------------------------------------------------------------------------------- */
DMM_API int dmm_proposal_boxes_f32(const float *prob, const float *boxes, const int32_t *counts, int images, int R, int M,
                                   int im_h, int im_w, float thresh, int padding, const int32_t *step, float *tight,
                                   dmm_stream_t stream);
DMM_API int dmm_nms_slots_f32(const float *tight, const float *scores, const int32_t *counts, int images, int R,
                              float thresh, int K, const int32_t *step, int32_t *keep, int32_t *keep_count,
                              dmm_stream_t stream);
DMM_API int dmm_paste_kept_f32(const float *prob, const float *boxes, const float *scores, const float *tight,
                               const int32_t *keep, const int32_t *keep_count, int images, int R, int M, int K, int im_h,
                               int im_w, int padding, const int32_t *step, const int32_t *img_base, float *planes,
                               int64_t plane_stride, uint64_t *packed, float *kept_boxes, float *kept_scores, float *rois,
                               dmm_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * (8) Frame-loop reductions (the step right after the path).
 * dmm_mask_boxes_f32: ohw_mask2boxlist (dmm/utils/utils.py:179-210, binmask_to_bbox_xyxy_pt :114-143) for R
 *   planes [R, H*W] (plane_stride elements apart): boxes [R,4] = tight xyxy box of (plane > thresh), or
 *   [0,0,W-1,H-1] when no pixel passes; valid [R] = 1 iff the plane has a pixel > 0 (reference: plane sum > 0).
 * dmm_merge_labels_f32: the per-frame label map of the evaluator (dmm/modules/evaluator.py:134-139):
 *   labels[b,x] = argmax([1 - max_o m[b,o,x], m[b,0,x], ..., m[b,O_b-1,x]]), first maximum wins (0 = background).
 *   masks [B,O,HW] with element strides; o_valid [B] int32 (NULL = O) live-template prefix per video; O <= 255.
 * ------------------------------------------------------------------------------------------- */
DMM_API int dmm_mask_boxes_f32(const float *masks, int R, int H, int W, int64_t plane_stride, float thresh,
                               float *boxes, int32_t *valid, dmm_stream_t stream);
DMM_API int dmm_merge_labels_f32(const float *masks, int B, int O, int HW, int64_t stride_b, int64_t stride_o,
                                 const int32_t *o_valid, uint8_t *labels, dmm_stream_t stream);

/* (8b) Device-resident frame cursor of the evaluator's loop (dmm/modules/evaluator.py:63-213: `for t in range(T)` with
 * every per-frame argument rebuilt on the host).  With the clip's raw proposals resident on the device ((7b)) and the
 * frame index in a device scalar, ONE captured HIP graph replays every frame step of the clip without host input:
 * dmm_step_select_i32: out[i] = table[*step * n + i] (a row of a per-clip table -- live template counts, commit flags
 *   per video -- copied to a fixed address); dmm_step_advance: *step += 1 (the graph's last node).
 * dmm_commit_masks_f32: out_mask_last of the per-video driver (dmm/modules/dmm_model.py:66-69 / :78-80): hist[b] =
 *   full[b] ([per_video] floats each) where commit[b] != 0; a skipped video (no live template, 'extra' frame) keeps its
 *   template planes. */
/* (8c) Frame-step epilogue on fixed slots: the mask mix (match_model.py:134-144), out_mask_last (dmm_model.py:66-69 /
 * :78-80) and the label map (evaluator.py:134-139) of every video of the step in ONE pass over the pixels, pasting the
 * few selected proposals ON THE FLY from their raw probabilities (so dmm_paste_kept_f32 may run with planes = NULL: the
 * soft planes of a frame, 10x the bytes of everything else in the step, are never written):
 *   full[b,m,:]  = sum_n Rb[b,m,n] * paste(raw proposal keep[b,n])   for m < m_valid[b], zeros otherwise (bit identical
 *                  to dmm_paste_kept_f32 + dmm_mask_mix: same paste arithmetic, same fma order);
 *   hist[b]      = full[b] where commit[b] != 0 (a skipped video keeps its template planes);
 *   packed_hist  = 1-bit planes of the new hist[b] (what the next frame's (5c) counts on; may be NULL);
 *   labels[b,x]  = as dmm_merge_labels_f32 over the first o_valid[b] rows of full (may be NULL).
 * Rb [B,M,Pp]; raw prob / boxes as in (7b) (clip resident, frame *step); keep / keep_count from dmm_nms_slots_f32.
 * M <= 8 rows, mask size + 2 padding <= 32; otherwise DMM_ERR_UNSUPPORTED (callers then paste the planes and use (4)). */
DMM_API int dmm_step_finish_f32(const float *Rb, int Pp, const float *prob, const float *boxes, const int32_t *keep,
                                const int32_t *keep_count, int B, int R, int Mm, int K, int M, int im_h, int im_w,
                                int padding, const int32_t *step, const int32_t *m_valid, const int32_t *commit,
                                const int32_t *o_valid, float *full, float *hist, uint64_t *packed_hist, uint8_t *labels,
                                dmm_stream_t stream);
DMM_API int dmm_step_select_i32(const int32_t *table, const int32_t *step, int n, int32_t *out, dmm_stream_t stream);
DMM_API int dmm_step_advance(int32_t *step, dmm_stream_t stream);
DMM_API int dmm_commit_masks_f32(const float *full, float *hist, const int32_t *commit, int B, int64_t per_video,
                                 dmm_stream_t stream);

/* dmm_ragged_pad: the batching step of the per-video driver (the reference loops MatchModel over the videos,
 *   dmm/modules/dmm_model.py:62-82 / :115-139; here they run as one ragged launch): out[b, i, :] = src_table[b][i, :] for
 *   i < counts[b], zeros up to P_max.  src_table: B device pointers (device memory) to contiguous [counts[b], row_bytes]
 *   blocks; counts [B] int32 (device); row_bytes % 4 == 0; out [B, P_max, row_bytes]. */
DMM_API int dmm_ragged_pad(const void *const *src_table, const int32_t *counts, int B, int P_max, int64_t row_bytes,
                           void *out, dmm_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * (9) Encoder epilogue (inference, channels-last bf16): x[r, c] = act(x[r, c] + bias[c] (+ residual[r, c])) in place,
 * one pass, fp32 arithmetic, one rounding.  What remains of conv -> BatchNorm -> ReLU (dmm/modules/base.py:43-54,
 * model_encoder.py:137-146) and of the residual tails of the torchvision blocks (dmm/modules/vision.py:6-38) once the
 * BatchNorm is folded into the contraction.  x, residual: [rows, C] bfloat16 (16-byte lane accesses when C % 8 == 0); bias: [C] fp32 or NULL.
 * ------------------------------------------------------------------------------------------- */
DMM_API int dmm_bias_act_bf16(void *x, const float *bias, const void *residual, int64_t rows, int C, int relu,
                              dmm_stream_t stream);

/* (9d) Stem tail of the channels-last inference encoder: y = maxpool3x3/s2/p1( relu(x + bias[c]) ) in ONE pass over the stem
 * convolution's output x [B, H, W, C] bf16 (C % 8 == 0) -> y [B, (H-1)/2+1, (W-1)/2+1, C]; bit identical to
 * dmm_bias_act_bf16 followed by the pool (bias, relu and rounding are monotone, so the window maximum is taken first).
 * Replaces bn1 -> relu -> maxpool of the torchvision bodies (dmm/modules/vision.py:11-21 forward) after BatchNorm folding. */
DMM_API int dmm_bias_relu_maxpool_bf16(const void *x, const float *bias, int B, int H, int W, int C, void *y,
                                       dmm_stream_t stream);

/* (9c) Patch matrix of a 3x3 / padding 1 / stride 1|2 convolution on a channels-last bf16 activation x [B, H, W, C]
 * (C % 8 == 0): cols [B * Ho * Wo, 9 * C] with cols[(b, ho, wo), (kh, kw, c)] = x[b, s ho + kh - 1, s wo + kw - 1, c], zero
 * outside the image; Ho = (H - 1) / s + 1.  With it the small-spatial 3x3 convolutions of the encoder (layer3 / layer4 of
 * the torchvision bodies, dmm/modules/vision.py:6-38, and the 3x3 heads, base.py:35-54) run as dmm_conv1x1_bf16 on the
 * patch matrix -- one GEMM with bias (+ residual) + ReLU in its epilogue -- where that beats MIOpen's convolution + a
 * separate bias / ReLU pass (encoder.FastEncoder times both once per shape). */
DMM_API int dmm_im2col3x3_bf16(const void *x, int B, int H, int W, int C, int stride, void *cols, dmm_stream_t stream);

/* (9b) A 1x1 convolution of the channels-last inference encoder with its whole tail as ONE hipBLASLt GEMM:
 *   y[rows, cout] = relu?( x[rows, cin] . w[cin, cout] + bias[cout] (+ residual[rows, cout]) )
 * x, w, residual, y bfloat16 row-major and dense, bias fp32, fp32 accumulation, one rounding.  Replaces conv1 / conv3 /
 * downsample of the torchvision bottlenecks (dmm/modules/vision.py:6-38) and the 1x1 head convolutions (base.py:35-54)
 * after BatchNorm folding; the residual rides as the GEMM's C operand (beta = 1) instead of a separate pass.
 * workspace: caller-owned scratch (may be NULL / 0: kernels that need one are then not considered);
 * DMM_ERR_UNSUPPORTED when the library offers no kernel for the shape (callers fall back to torch.mm + (9)). */
DMM_API int dmm_conv1x1_bf16(const void *x, const void *w, const float *bias, const void *residual, int64_t rows, int cin,
                             int cout, int relu, void *y, void *workspace, size_t workspace_bytes, dmm_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * (10) Training-mode BatchNorm (+ residual) (+ ReLU) of the encoder, channels-last bf16, fp32 statistics: two launches each
 * way where the stock path issues five or six (three BatchNorm kernels + add + clamp).  Replaces, in the trainer's step
 * (train.py:296-307), bn -> relu and bn -> (+ identity) -> relu of the torchvision blocks (dmm/modules/vision.py:6-38),
 * the conv -> BN -> ReLU -> conv -> BN heads (base.py:43-54) and the skip projections' bn (model_encoder.py:137-140).
 * x, residual, y, dy, dx, dres: [rows, C] bfloat16 (C % 8 == 0 and 256 % (C / 8) == 0, else DMM_ERR_UNSUPPORTED);
 * everything else fp32.  Forward: dmm_bn_stats_bf16 accumulates sum(x), sum(x^2) per channel into stats [2, C] (the CALLER
 * zeroes it beforehand; atomics, order free); dmm_bn_apply_bf16 turns them into mean / invstd (biased variance, eps inside
 * the root), writes y = act(x * w * invstd + (b - mean * w * invstd) (+ residual)), saved [2, C] = (mean, invstd) and -- when
 * running_mean / running_var are given -- running <- (1 - momentum) * running + momentum * batch with the UNBIASED variance
 * (torch.nn.BatchNorm2d in training mode).  Backward: with g = dy * [y > 0] when relu, else dy: dmm_bn_bwd_reduce_bf16
 * accumulates sum(g), sum(g * xhat) into sums [2, C] (caller-zeroed); dmm_bn_bwd_dx_bf16 writes
 * dx = w * invstd * (g - mean(g) - xhat * mean(g * xhat)), dres = g (NULL: no residual branch), dweight = sum(g * xhat),
 * dbias = sum(g).  relu: 0 none; 1 the mask from the output y; 2 (no residual: dres NULL) the mask recomputed from x with the forward's
 * own fma, x * (w * invstd) + (b - mean * w * invstd) > 0 -- weight / bias as the forward saw them; y is then not read at all.
 * What every entry of (10) and (10a) answers, in this order (where two faults coincide, the earlier one is named):
 *   1. DMM_ERR_BAD_ARG      rows < 0, C <= 0, groups outside 1..64 or not dividing rows, relu outside 0..2 (the backward
 *                           entries; the apply entries take relu as a flag, any value other than 0 is a ReLU)
 *   2. DMM_OK               rows == 0: nothing to do, whatever the pointers and C
 *   3. DMM_ERR_BAD_ARG      a null pointer the entry cannot do without (stats / sums of the atomic entries among them, the
 *                           workspace of the deterministic ones not yet), running_mean without running_var or the reverse,
 *                           relu == 1 without y, relu == 2 without weight / bias (reduce), without bias or with dres (dx)
 *   4. DMM_ERR_UNSUPPORTED  C % 8 != 0 or 256 % (C / 8) != 0
 *   5. (10a) only           DMM_ERR_BAD_ARG for a null workspace, then DMM_ERR_WORKSPACE for a short one
 * ------------------------------------------------------------------------------------------- */
DMM_API int dmm_bn_stats_bf16(const void *x, int64_t rows, int C, float *stats, dmm_stream_t stream);
DMM_API int dmm_bn_apply_bf16(const void *x, const void *residual, int64_t rows, int C, const float *stats,
                              const float *weight, const float *bias, float *running_mean, float *running_var,
                              float momentum, float eps, int relu, void *y, float *saved, dmm_stream_t stream);
DMM_API int dmm_bn_bwd_reduce_bf16(const void *dy, const void *x, const void *y, int64_t rows, int C, const float *saved,
                                   const float *weight, const float *bias, int relu, float *sums, dmm_stream_t stream);
DMM_API int dmm_bn_bwd_dx_bf16(const void *dy, const void *x, const void *y, int64_t rows, int C, const float *saved,
                               const float *weight, const float *bias, const float *sums, int relu, void *dx, void *dres,
                               float *dweight, float *dbias, dmm_stream_t stream);
/* The same four with `groups` STATISTICS GROUPS: the rows are `groups` consecutive ranges of rows / groups rows, each normalised
 * with its own batch statistics -- one launch computes what `groups` calls of the layer on the ranges, in order, compute: the
 * reference's trainer calls the encoder once per frame of a clip (trainer.py:95-131: BatchNorm statistics over the videos of ONE
 * frame step), and a clip batched into one encoder call keeps exactly those statistics with groups = frames.  stats / saved / sums
 * are [groups][2][C]; the running statistics take `groups` momentum updates in group order; dweight / dbias are the sums over the
 * groups.  rows % groups == 0, 1 <= groups <= 64.  (The plain entries are groups = 1.)  The two backward entries take a SECOND
 * gradient plane dy2 (may be NULL): the layer's output went to two consumers (a residual block's first convolution and its identity
 * branch, dmm/modules/vision.py:26-38) and the gradient is dy + dy2, added in fp32 inside the kernels instead of by a launch. */
DMM_API int dmm_bn_stats_grouped_bf16(const void *x, int64_t rows, int C, int groups, float *stats, dmm_stream_t stream);
DMM_API int dmm_bn_apply_grouped_bf16(const void *x, const void *residual, int64_t rows, int C, int groups, const float *stats,
                                      const float *weight, const float *bias, float *running_mean, float *running_var,
                                      float momentum, float eps, int relu, void *y, float *saved, dmm_stream_t stream);
DMM_API int dmm_bn_bwd_reduce_grouped_bf16(const void *dy, const void *dy2, const void *x, const void *y, int64_t rows, int C, int groups,
                                           const float *saved, const float *weight, const float *bias, int relu, float *sums,
                                           dmm_stream_t stream);
DMM_API int dmm_bn_bwd_dx_grouped_bf16(const void *dy, const void *dy2, const void *x, const void *y, int64_t rows, int C, int groups,
                                       const float *saved, const float *weight, const float *bias, const float *sums, int relu,
                                       void *dx, void *dres, float *dweight, float *dbias, dmm_stream_t stream);
/* (10a) DETERMINISTIC forms of the grouped entries: bit-identical results run after run (no float atomics).  The statistics /
 * reduce launch stores one fp32 partial per (group, row group, statistic, channel) into the caller's workspace -- a slab of
 * dmm_bn_det_workspace_bytes(rows, C, groups) bytes (0 for a shape outside the envelope), written whole, no zeroing -- and the
 * consuming launch (apply / dx) folds the slab in a fixed order in its prologue.  The two launches of a direction take the
 * SAME workspace and the same rows / C / groups.  dmm_bn_fold_det folds a statistics slab on its own into out [groups][2][C]
 * (sum(x), sum(x^2): a bias gradient is its first row).  Arguments otherwise as above; a short workspace answers
 * DMM_ERR_WORKSPACE before anything is launched.  Not bitwise equal to the atomic entries (a different addition order). */
DMM_API size_t dmm_bn_det_workspace_bytes(int64_t rows, int C, int groups);
DMM_API int dmm_bn_stats_det_grouped_bf16(const void *x, int64_t rows, int C, int groups, void *workspace,
                                          size_t workspace_bytes, dmm_stream_t stream);
DMM_API int dmm_bn_apply_det_grouped_bf16(const void *x, const void *residual, int64_t rows, int C, int groups,
                                          const void *workspace, size_t workspace_bytes, const float *weight, const float *bias,
                                          float *running_mean, float *running_var, float momentum, float eps, int relu, void *y,
                                          float *saved, dmm_stream_t stream);
DMM_API int dmm_bn_bwd_reduce_det_grouped_bf16(const void *dy, const void *dy2, const void *x, const void *y, int64_t rows, int C,
                                               int groups, const float *saved, const float *weight, const float *bias, int relu,
                                               void *workspace, size_t workspace_bytes, dmm_stream_t stream);
DMM_API int dmm_bn_bwd_dx_det_grouped_bf16(const void *dy, const void *dy2, const void *x, const void *y, int64_t rows, int C,
                                           int groups, const float *saved, const float *weight, const float *bias,
                                           const void *workspace, size_t workspace_bytes, int relu, void *dx, void *dres,
                                           float *dweight, float *dbias, dmm_stream_t stream);
DMM_API int dmm_bn_fold_det(const void *workspace, size_t workspace_bytes, int64_t rows, int C, int groups, float *out,
                            dmm_stream_t stream);

/* (10b) Weight gradient of the encoder's convolutions (channels-last bf16 activations, fp32 gradient), what autograd
 * computes for conv1 / conv3 / downsample (1x1) and conv2 / the heads (3x3, padding 1) of dmm/modules/vision.py:6-38 and
 * base.py:35-54 under the trainer's backward (train.py:296-307):
 *   dmm_wgrad_bf16:     dw[co, ci]         = sum_r dy[r, co] * x[r, ci]            dy [rows, ldy], x [rows, ldx] (element strides)
 *   dmm_wgrad3x3_bf16:  dw[co, ci, kh, kw] = sum_(b,ho,wo) dy[(b,ho,wo), co] * x[b, s*ho+kh-1, s*wo+kw-1, ci]   (zero outside)
 *     dy [B*Ho*Wo, co], x [B, H, W, ci] dense, Ho = (H-1)/s + 1, s in {1, 2}; the patch matrix is never materialised; dw comes
 *     out in the parameter's own [co, ci, 3, 3] contiguous layout.
 * dw is fp32 and OVERWRITTEN (no zeroing, no atomics, deterministic: row slabs -> partial tables in the caller's workspace
 * -> summed in slab order).  workspace: dmm_wgrad_workspace_bytes(rows, co, cv) bytes (cv = ci, or 9 * ci for the 3x3 form;
 * 0 when the shape is not taken).  co % 64 == 0 and ci % 64 == 0 (every width of the ResNet bodies and 128-wide heads), else
 * DMM_ERR_UNSUPPORTED (callers fall back to the library product).  MFMA 32x32x16 bf16, fp32 accumulation; memory bound. */
/* (10c) Weight and layout helpers of the training encoder (dmm/modules/vision.py:6-38 under train.py:296-307).
 * dmm_wprep3x3_bf16: every 3x3 weight of a segment in one launch.  `table` = n device records of 40 bytes
 * {const float *src; uint16 *dst; uint16 *dstT; int32 co; int32 ci; int64 tile0}: src the fp32 master [co, ci, 3, 3], dst the bf16
 * channels-last weight [co, kh, kw, ci], dstT (may be null) [ci, 2-kh, 2-kw, co] -- the weight with which the DATA gradient of a
 * stride 1 / padding 1 convolution is itself a forward convolution, dX = conv(dY, dstT) (MIOpen's forward kernel for that problem
 * is ~1.8x faster than its backward-data kernel on gfx950).  co, ci multiples of 32, dst / dstT 16-byte aligned; tile0 = sum of (co/32)*(ci/32) of the records
 * before; tiles = that sum over all records.
 * dmm_subsample2_bf16: y[b, ho, wo, :] = x[b, 2ho, 2wo, :] on channels-last bf16 (the stride of a 1x1 downsample convolution);
 * dmm_upsample2_zero_bf16: its gradient, dx [B, H, W, C] written once (dy at even positions, zero elsewhere).  C % 8 == 0. */
DMM_API int dmm_wprep3x3_bf16(const void *table, int n, int64_t tiles, dmm_stream_t stream);
/* fp32 -> bf16 copies of n tensors in one launch (the 1x1 weights of a segment): device records of 32 bytes
 * {const float *src; uint16 *dst; int64 n; int64 block0}, n a multiple of 8, both 16-byte aligned; a workgroup converts 8192
 * elements: block0 = sum of ceil(n / 8192) of the records before, blocks = that sum over all records. */
DMM_API int dmm_cast_many_bf16(const void *table, int n, int64_t blocks, dmm_stream_t stream);
DMM_API int dmm_subsample2_bf16(const void *x, int B, int H, int W, int C, void *y, dmm_stream_t stream);
DMM_API int dmm_upsample2_zero_bf16(const void *dy, int B, int H, int W, int C, void *dx, dmm_stream_t stream);
DMM_API size_t dmm_wgrad_workspace_bytes(int64_t rows, int co, int cv);
DMM_API int dmm_wgrad_bf16(const void *dy, const void *x, int64_t rows, int co, int ci, int64_t ldy, int64_t ldx, float *dw,
                           void *workspace, size_t workspace_bytes, dmm_stream_t stream);
DMM_API int dmm_wgrad3x3_bf16(const void *dy, const void *x, int B, int H, int W, int ci, int co, int stride, float *dw,
                              void *workspace, size_t workspace_bytes, dmm_stream_t stream);

/* (10d) 3x3 / padding 1 convolution of the training encoder for the DETERMINISTIC mode (conv2 of the bottlenecks and the 3x3
 * head convolutions, dmm/modules/vision.py:6-38 and base.py:35-54, as train.py:46 runs them under cudnn.deterministic):
 *   y[b, ho, wo, co] = bf16( bias[co] + sum_(kh,kw,ci) x[b, s*ho+kh-1, s*wo+kw-1, ci] * w[co, kh, kw, ci] )      (zero outside)
 * x [B, H, W, ci] and y [B, Ho, Wo, co] dense channels-last bf16, Ho = (H-1)/s + 1, Wo likewise, s in {1, 2}; w the bf16
 * channels-last weight [co, kh, kw, ci] (what dmm_wprep3x3_bf16 writes as dst); bias bf16 [co] or NULL.  fp32 accumulation, the
 * bias added in fp32, ONE rounding.  The DATA gradient of such a convolution is the same entry on dy with dmm_wprep3x3_bf16's
 * dstT (stride 2: on dmm_upsample2_zero_bf16(dy), at stride 1).  Implicit GEMM on MFMA 32x32x16 bf16; no atomics: where the
 * reduction is split, every split stores its fp32 partial into the caller's workspace and a second launch sums them in order.
 * The split is a function of (H, W, ci, co, stride) only -- an image's result does not depend on B, on arrival order or on
 * what else runs -- so results are bit-identical call after call, eagerly and in graph replay (no host reads, no allocation).
 * workspace: dmm_conv3x3_workspace_bytes(...) bytes (0: none needed, NULL is fine; 0 as well for arguments the entry rejects).
 * Answers, before any launch: DMM_ERR_BAD_ARG for B < 0, H / W / ci / co <= 0, a stride other than 1 or 2, ci or co not a
 * multiple of 64; DMM_OK for B == 0; DMM_ERR_BAD_ARG for a null x / w / y, a pointer that is not 16-byte aligned, a needed
 * workspace that is null or shorter than dmm_conv3x3_workspace_bytes. */
DMM_API size_t dmm_conv3x3_workspace_bytes(int B, int H, int W, int ci, int co, int stride);
DMM_API int dmm_conv3x3_bf16(const void *x, const void *w, const void *bias, int B, int H, int W, int ci, int co, int stride,
                             void *y, void *workspace, size_t workspace_bytes, dmm_stream_t stream);

/* (10e) The NARROW 3x3 / padding 1 / stride 1 convolutions of the training encoder for the DETERMINISTIC mode: widths that are
 * multiples of 32 but not of 64 -- the level-2 heads of base.py:35-54 (256 -> 32, 32 -> 128) as train.py:46 runs them under
 * cudnn.deterministic -- which (10b) and (10d) reject.  Multiples of 64 are taken too.
 * dmm_conv3x3_narrow_bf16: the contract of (10d) at stride 1: x [B, H, W, ci] and y [B, H, W, co] dense channels-last bf16, w the
 *   bf16 channels-last weight [co, kh, kw, ci] (dmm_wprep3x3_bf16's dst), bias bf16 [co] or NULL; fp32 accumulation, the bias added
 *   in fp32, ONE rounding.  The DATA gradient is the same entry on dy with dmm_wprep3x3_bf16's dstT.  No atomics, no split of the
 *   reduction, no workspace: the summation order of an output element is a function of (ci, co) alone, an image's bits do not
 *   depend on its batch, results are bit-identical call after call, eagerly and in graph replay.  Answers, before any launch:
 *   DMM_ERR_BAD_ARG for B < 0, H / W / ci / co <= 0, ci or co not a multiple of 32; DMM_OK for B == 0; DMM_ERR_BAD_ARG for a null
 *   x / w / y, a pointer that is not 16-byte aligned, more than 2^31 - 1 tiles of 128 pixels.
 * dmm_wgrad3x3_narrow_bf16:  dw[co, ci, kh, kw] = sum_(b,h,w) dy[(b,h,w), co] * x[b, h+kh-1, w+kw-1, ci]   (zero outside), dy
 *   [B*H*W, co] and x [B, H, W, ci] dense bf16; dw fp32 in the parameter's own [co, ci, 3, 3] layout, OVERWRITTEN (no zeroing, no
 *   atomics: row slabs -> partial tables in the caller's workspace -> summed in slab order, as (10b)).  workspace:
 *   dmm_wgrad3x3_narrow_workspace_bytes(...) bytes, 16-byte aligned (0 for arguments the entry rejects and for B == 0).  Answers,
 *   before any launch: DMM_ERR_BAD_ARG for B < 0, H / W / ci / co <= 0, a width that is not a multiple of 32, a null dw; for
 *   B == 0 dw is zeroed and the answer is DMM_OK; DMM_ERR_BAD_ARG for a null dy / x, a dy / x / dw that is not 4-byte aligned;
 *   DMM_ERR_WORKSPACE for a null or short workspace. */
DMM_API int dmm_conv3x3_narrow_bf16(const void *x, const void *w, const void *bias, int B, int H, int W, int ci, int co,
                                    void *y, dmm_stream_t stream);
DMM_API size_t dmm_wgrad3x3_narrow_workspace_bytes(int B, int H, int W, int ci, int co);
DMM_API int dmm_wgrad3x3_narrow_bf16(const void *dy, const void *x, int B, int H, int W, int ci, int co, float *dw,
                                     void *workspace, size_t workspace_bytes, dmm_stream_t stream);

/* (10f) The 7x7 / stride 2 / padding 3 STEM convolution (3 -> 64, dmm/modules/vision.py's ResNet conv1) of the training encoder
 * for the DETERMINISTIC mode, as train.py:46 runs it under cudnn.deterministic: three input channels are 6-byte pixels, which
 * the 16-byte operand pieces of (10b) / (10d) / (10e) cannot take.  ci = 3 and co = 64 are fixed.
 * dmm_conv7x7s2_stem_bf16:
 *   y[b, ho, wo, co] = bf16( bias[co] + sum_(kh,kw,ci) x[b, 2ho+kh-3, 2wo+kw-3, ci] * w[co, kh, kw, ci] )        (zero outside)
 *   x [B, H, W, 3] and y [B, Ho, Wo, 64] dense channels-last bf16, Ho = (H-1)/2 + 1, Wo likewise; w the bf16 channels-last weight
 *   [64, 7, 7, 3] (weight.to(bf16, channels_last)); bias bf16 [64] or NULL.  fp32 accumulation, the bias added in fp32, ONE
 *   rounding.  MFMA 32x32x16 bf16 over K = 7 kernel rows x 32 lanes (21 real; the other 11 are exact zeros on BOTH operands: no
 *   value from outside the 7x7 window or from outside the tensor is fetched, let alone multiplied).  No atomics, no split of the
 *   reduction, no workspace: the summation order of an output element is a function of nothing but a term's position in the
 *   147-term reduction, an image's bits do not depend on its batch, results are bit-identical call after call, eagerly and in
 *   graph replay.  x needs only its natural 2-byte alignment (an image row is 6 W bytes); w and y 16-byte; the bias 2-byte.
 *   Answers, before any launch: DMM_ERR_BAD_ARG for B < 0, H / W <= 0, B * H * W > 2^56; DMM_OK for B == 0; DMM_ERR_BAD_ARG for
 *   a null x / w / y, a misaligned pointer.
 * dmm_wgrad7x7s2_stem_bf16:  dw[co, ci, kh, kw] = sum_(b,ho,wo) dy[(b,ho,wo), co] * x[b, 2ho+kh-3, 2wo+kw-3, ci]   (zero outside),
 *   dy [B*Ho*Wo, 64] dense bf16 (16-byte aligned), x as above; dw fp32 (4-byte aligned) in the parameter's own [64, 3, 7, 7]
 *   layout, OVERWRITTEN (no zeroing, no atomics: pixel slabs -> fp32 partial tables in the caller's workspace -> summed in slab
 *   order by a second launch, as (10b) / (10e)).  The slab count is a function of (B, H, W) only.  workspace:
 *   dmm_wgrad7x7s2_stem_workspace_bytes(B, H, W) bytes, 4-byte aligned (0 for arguments the entry rejects and for B == 0).
 *   Answers, before any launch: DMM_ERR_BAD_ARG for B < 0, H / W <= 0, B * H * W > 2^56, a null or misaligned dw; for B == 0 dw
 *   is zeroed and the answer is DMM_OK; DMM_ERR_BAD_ARG for a null or misaligned dy / x; DMM_ERR_WORKSPACE for a null or short
 *   workspace; DMM_ERR_BAD_ARG for a misaligned one.
 * No data gradient: the image never requires one. */
DMM_API int dmm_conv7x7s2_stem_bf16(const void *x, const void *w, const void *bias, int B, int H, int W, void *y,
                                    dmm_stream_t stream);
DMM_API size_t dmm_wgrad7x7s2_stem_workspace_bytes(int B, int H, int W);
DMM_API int dmm_wgrad7x7s2_stem_bf16(const void *dy, const void *x, int B, int H, int W, float *dw, void *workspace,
                                     size_t workspace_bytes, dmm_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * (11) HIP-graph hygiene for captured steps that contain other libraries' launches (MIOpen, hipBLASLt, torch): between the
 * end of a stream capture and hipGraphInstantiate, replace every memset node (flags & 1; element size 1 / 2 / 4) and every
 * 1-D device-to-device memcpy node (flags & 2) of `graph` (a hipGraph_t) by a kernel node with the same dependencies and
 * dependents.  On the runtime of this image a replayed memset node is not reliably ordered before the kernel node behind it
 * (profiles/r04_graph_memset_node.txt; round 6: MIOpen's bf16 weight-gradient solvers clear their split-K workspace that
 * way).  n_memset / n_memcpy: nodes replaced; n_left: memset / memcpy nodes left as they were (other kinds, flags off).
 * Nothing in the reference corresponds to it (train.py:296-307 launches eagerly); used by dmm_net_amd/train_encoder.py.
 * ------------------------------------------------------------------------------------------- */
DMM_API int dmm_graph_nodes_to_kernels(void *graph, int flags, int *n_memset, int *n_memcpy, int *n_left);

/* ---------------------------------------------------------------------------------------------
 * (12) The ConvLSTM refine decoder (dmm/modules/base.py:71-188 RSISMask, dmm/modules/clstm.py:68-131 ConvLSTMCellMask, driven
 * per object by dmm/modules/evaluator.py:179-212): everything BETWEEN its convolutions.  fp32 ((12i)-(12k): the evaluator's
 * forward on bf16 activations), dense planes (row stride = width, channel stride = plane), batch / object strides in elements;
 * nothing allocates, no memset nodes.  Used by
 * dmm_net_amd/decoder.py, which keeps the convolutions on the library.  (12a)-(12d) are the forward; (12e) is the backward of
 * the cell (12b); (12f)-(12h) are what the refine step of TRAINING (dmm/modules/trainer.py:236-306) runs around the decoder:
 * the backward of the pyramid (12a), the backward of the upsample (12c) in 'write' mode, and the trainer's own finish
 * (nearest interpolation, sigmoid, pad) with its backward.  None of (12f)-(12h) uses an atomic or a workspace.  (12i)-(12k) are
 * (12b)-(12d) on bf16 activations, for the evaluator behind a bf16 encoder (RSISMask.compute_dtype = torch.bfloat16); (12l)-(12o)
 * are (12e), (12g) and (12h) on bf16 activations, for the trainer behind one (RSISMask.train_dtype = torch.bfloat16).
 *
 * (12a) dmm_mask_pyramid_f32 -- evaluator.py:188-195: MaxPool2d((2,2), ceil_mode=True) applied 5, 4, 3 and 2 times to the planes
 *   prev_mask[b, t], y_mask[b, t], init_pred[b, t] (each H x W at base + b * sb + t * so), b < B, t < n_obj, in ONE launch and
 *   without the reference's cat.  k nested ceil-mode pools = the maximum over the clipped 2^k x 2^k window, size ceil(H / 2^k):
 *   bit exact.  out_k: [n_obj, B, 3, ceil(H / 2^k), ceil(W / 2^k)] dense, plane order (prev_mask, y_mask, init_pred) -- object
 *   t's slice is the [B, 3, h, w] entry of the reference's mask_lstm.  B * n_obj * 3 <= 65535.
 *
 * (12b) dmm_clstm_gates_f32 -- clstm.py:112-129 for the three cell evaluations of a level (base.py:134-153), which differ in
 *   the one-channel mask plane only:  gates_k = (pre0 + pre1 + pre2) + stencil3x3(w_mask, m_k), k = plane 0, 2, 1 (prev_mask,
 *   init_pred, y_mask: base.py:116-118, 134-150); gate order in / remember / out / cell (chunk(4, 1)); cell_k = sigmoid(remember)
 *   * cell_prev + sigmoid(in) * tanh(cellgate), hidden_k = sigmoid(out) * tanh(cell_k); hidden = (h_0 + h_2 + h_1) / 3, cell
 *   likewise (base.py:152-153).  pre0..2: the shared pre-activation [B, 4 * hidden_size, h, w] as up to three addends (batch
 *   strides sb0..2; pre1 / pre2 may be null); masks [B, 3, h, w] (batch stride sb_masks); w_mask [4 * hidden_size, 9] = the mask
 *   channel of Gates.weight; cell_prev [B, hidden_size, h, w] dense or null (= zeros, the reference's None state); hidden /
 *   cell [B, hidden_size, h, w] dense; hidden_copy (may be null; batch stride sb_copy): a second copy of hidden, written into
 *   the convolution input of the next object's evaluation of this level.
 *
 * (12c) dmm_upsample_bilinear_into_f32 -- base.py:165-175, 179-181: UpsamplingBilinear2d (align_corners = True, coordinates
 *   and weights as ATen computes them) of src [B, C, h, w] to H x W, combined into channels c0 .. c0 + C of dst [B, C_dst, H, W]
 *   by mode 0 = write (skip modes 'concat' / 'none'), 1 = add ('sum'), 2 = multiply ('mul').
 *
 * (12d) dmm_refine_finish_f32 -- evaluator.py:200-212 for every object of the frame in one launch: logits[b, t] (h x w at base +
 *   b * sb_logits + t * so_logits, conv_out's output) -> bilinear (align_corners = True) to H x W -> sigmoid -> outs[b, t]; the
 *   same value into mask_hist[b, t] where valid[b * O + t] != 0 (int32, read on the device; mask_hist may be null); rows
 *   n_obj <= t < O of outs are zeroed.  outs / mask_hist [B, O, H, W] dense.
 *
 * (12e) dmm_clstm_gates_bwd_f32 -- the backward of (12b).  Reads what the forward read (pre0..2, masks, w_mask, cell_prev, the
 *   same strides and null meanings) and the upstream gradients d_hidden / d_cell [B, hidden_size, h, w] dense (either may be
 *   null = zeros, not both).  Nothing of the forward is saved: the gates are recomputed with the forward's expressions in the
 *   forward's order.  With u = d_hidden / 3, v = d_cell / 3 and, per plane k, the activated gates i, r, o, g, c_k and
 *   t_k = tanh(c_k):  dc_k = v + u o (1 - t_k^2);  the pre-activation gradients are  in: dc_k g i (1 - i),  remember:
 *   dc_k cell_prev r (1 - r) (0 without cell_prev),  out: u t_k o (1 - o),  cell: dc_k i (1 - g^2)  -- ds_{q,k} below.
 *   Outputs (a null pointer = not wanted, and no work is done for it; d_pre is required):
 *     d_pre       [B, 4 * hidden_size, h, w] dense = (ds_{q,0} + ds_{q,2}) + ds_{q,1}: the gradient of the sum, so of every addend
 *     d_cell_prev [B, hidden_size, h, w] dense = (dc_0 r_0 + dc_2 r_2) + dc_1 r_1; must be null when cell_prev is null
 *     d_masks     [B, 3, h, w] dense, the input's plane order: the transposed stencil of ds_{.,k} (sources outside the plane: none)
 *     d_w_mask    [4 * hidden_size, 9] = sum over (b, y, x, k) of ds_{q,k} * m_k at the tap (taps outside the plane: 0)
 *   One launch for d_pre / d_cell_prev alone; two when d_masks or d_w_mask is wanted (the second folds the workspace).  No float
 *   atomics: d_masks sums the channel groups' partials in ascending order, d_w_mask the 64-lane tree, the four waves and then
 *   the position blocks in ascending order -- every output's bits are a function of the inputs and (B, hidden_size, h, w).
 *   ws: dmm_clstm_gates_bwd_workspace_bytes(B, hidden_size, h, w) bytes (0 for sizes the entry refuses or has no work for),
 *   4-byte aligned, written before it is read (no zeroing); needed only when d_masks or d_w_mask is wanted (else may be null).
 *
 * (12f) dmm_mask_pyramid_bwd_f32 -- the backward of (12a) for the planes that carry a gradient in training: prev_mask (last
 *   frame's outs, trainer.py:124-125) and init_pred (the matching layer's output).  Reads the planes the forward read (same
 *   strides) and the gradients of its four outputs, d_out_k [n_obj, B, 3, ceil(H / 2^k), ceil(W / 2^k)] dense, k = 5, 4, 3, 2
 *   (a null d_out_k = zeros); channel 1 of them, the reference mask's, is ignored.  Writes d_prev / d_init: plane (b, t) at
 *   base + b * sb + t * so, H x W dense, so >= H * W; either may be null = not wanted (no work is done for it; both null: DMM_OK,
 *   nothing launched).  EVERY pixel of every wanted plane is written: the caller does not pre-zero.
 *   The four levels share one chain of pools: one pool, then four more, outputs after the 2nd to 5th.  The gradient of a level-k
 *   output descends to the ONE pixel that wins its clipped 2^k x 2^k window under ATen's rule applied pool by pool: a 2 x 2 pool
 *   scans its (clipped) window in row-major order and a later element wins on a strict '>' only, so the first maximum wins.
 *   For the composite window: among equal maxima the pixel with the smallest Z-order code wins -- the code interleaves the bits
 *   of (y, x) inside the window, the y bit above the x bit at every level.  This is NOT the first maximum in row-major order
 *   (in the 4 x 4 window, pixel (1, 0) has code 2 and beats pixel (0, 2), code 4).  Masks are full of exact zeros and ones: ties
 *   are the normal case.  A pixel's gradient is (((0 + g_2) + g_3) + g_4) + g_5 over the levels it wins, in this fixed order.
 *   Inputs are taken as finite.  B * n_obj * 3 <= 65535 as in (12a).
 *
 * (12g) dmm_upsample_bilinear_bwd_f32 -- the backward of (12c) in mode 0 (write).  d_dst: channels c0 .. c0 + C of a
 *   [B, C_dst, H, W] tensor (batch stride sb_dst), as the forward writes one; d_src [B, C, h, w] (batch stride sb_src), every
 *   element written.  Gather form: d_src[b, c, y, x] = sum over Y ascending, then X ascending, of (wy(Y) * wx(X)) * d_dst[b,
 *   c0 + c, Y, X] over the destination pixels whose interpolation touches (y, x); with (i0, step, l0, l1) = the forward's own
 *   fp32 index rule for Y (src = scale * Y, scale = (h - 1) / (H - 1) in fp32 or 0 for H == 1, i0 = trunc(src) clipped to
 *   h - 1, step = (i0 < h - 1), l1 = src - i0, l0 = 1 - l1):  wy(Y) = l0 if i0 == y, plus l1 if i0 + step == y.  The kernel
 *   classifies its candidates with the very function the forward uses, so both agree on every index and weight, h == 1 and
 *   H == 1 included.  H >= h >= 1 and W >= w >= 1; anything else: DMM_ERR_UNSUPPORTED.
 *
 * (12h) dmm_refine_train_finish_f32 / dmm_refine_train_finish_bwd_f32 -- trainer.py:275-287, 302-304 for every object of the
 *   frame in one launch.  Forward: outs[b, t, Y, X] = sigmoid(logits[b, t, iy(Y), ix(X)]) for t < n_obj, zero rows for
 *   n_obj <= t < O; outs [B, O, H, W] dense; logits strided as (12d)'s.  The interpolation is torch's default NEAREST, not the
 *   evaluator's bilinear: i(dst) = min((int)floorf(dst * scale), in - 1), scale = (float)in / (float)out in fp32.  Backward:
 *   d_logits[b, t, y, x] = p (1 - p) * sum of d_outs[b, t, Y, X] over the destination pixels that read (y, x) -- a contiguous
 *   block, summed Y then X ascending; a logit nobody reads (out < in) gets 0; p is recomputed from the logit.  d_outs
 *   [B, O, H, W] dense (rows t >= n_obj are not read); d_logits: plane (b, t), t < n_obj, at base + b * sb_d + t * so_d.
 *
 * (12i)-(12k) The forward entries (12b)-(12d) with the ACTIVATIONS -- what the library convolutions write and read -- stored as
 *   bf16 (the upper 16 bits of the fp32 pattern; pointers declared void *, 2-byte aligned, strides in ELEMENTS as before).  One
 *   rule for all three: every 16-bit value is widened to fp32 on load (exact), the expressions are those of the fp32 entry in
 *   the same order (the library is built with -ffp-contract=off; the kernels are one template over the storage type), and every
 *   16-bit output is rounded ONCE, to nearest even, at its store (a NaN becomes 0x7FC0, torch's rule).  So entry_bf16(x) equals
 *   bf16(entry_f32(widened x)) bit for bit, and its fp32 outputs equal entry_f32's bit for bit.  A lane owns one position and
 *   issues 2-byte loads and stores: any width, any 2-byte-aligned plane or row, nothing stored outside the tensor.  No
 *   atomics, no workspace (the backward forms are (12l)-(12o)).  Each entry validates as its fp32 sibling does: the same answers in the same order, before
 *   any HIP call.
 * (12i) dmm_clstm_gates_bf16 -- (12b) with pre0..2, hidden and hidden_copy bf16 (same null meanings and batch strides).  masks,
 *   w_mask, cell_prev and cell stay fp32: the cell state is the recurrence along the object chain and keeps full precision; the
 *   mask planes and the 36-weight stencil are what (12a) and the fp32 parameters hand over.
 * (12j) dmm_upsample_bilinear_into_bf16 -- (12c) with src and dst bf16, modes 0 / 1 / 2; in modes 1 and 2 dst is read as bf16,
 *   combined in fp32 and rounded once.
 * (12k) dmm_refine_finish_bf16 -- (12d) with bf16 logits (the output of a bf16 conv_out); outs and mask_hist fp32, valid int32.
 *
 * (12l)-(12o) The TRAINING entries (12e), (12g), (12h) on bf16 activations (RSISMask.train_dtype = torch.bfloat16, behind a bf16
 *   TrainEncoder).  The rule of (12i)-(12k) holds for each: 16-bit values widened on load, the fp32 entry's expressions in its
 *   order (one template over the storage type), every 16-bit output rounded once at its store, 2-byte loads and stores by the lane
 *   that owns the element -- any 2-byte-aligned base.  So entry_bf16(x) == bf16(entry_f32(widened x)) for its 16-bit outputs and
 *   == entry_f32(widened x) for its fp32 outputs, bit for bit.  The operands that are fp32 in the forward are fp32 here; the
 *   pyramid and its backward (12a), (12f) have no 16-bit form (mask planes are fp32 in every form).  Each entry validates as its
 *   fp32 sibling does, the same answers in the same order before any launch; strides in elements; no float atomics.
 * (12l) dmm_clstm_gates_bwd_bf16 -- (12e), the backward of (12i).  bf16: pre0..2, d_hidden (the gradient of the bf16 hidden) and
 *   d_pre.  fp32: masks, w_mask, cell_prev, d_cell, d_cell_prev, d_masks, d_w_mask and the workspace -- the gate gradients reach
 *   both reductions unrounded.  Same null meanings (pre1 / pre2 / cell_prev absent; d_hidden or d_cell = zeros, not both; a null
 *   output = not wanted), the same batch strides, the same dmm_clstm_gates_bwd_workspace_bytes, the same fold launch and fixed
 *   orders as (12e).
 * (12m) dmm_upsample_bilinear_bwd_bf16 -- (12g) with d_dst and d_src bf16: the gather accumulates in fp32, Y then X ascending,
 *   and rounds once.  H >= h >= 1 and W >= w >= 1, anything else DMM_ERR_UNSUPPORTED; batch strides sb_dst / sb_src as (12g).
 * (12n) dmm_refine_train_finish_bf16 -- the forward of (12h) on bf16 logits (the output of a bf16 conv_out; strided as (12d)'s:
 *   sb_logits / so_logits, dense planes); outs [B, O, H, W] fp32 dense, zero rows for n_obj <= t < O.  Equals the fp32 entry on
 *   the widened logits bit for bit.
 * (12o) dmm_refine_train_finish_bwd_bf16 -- the backward of (12h): logits bf16 (strided as above), d_outs fp32 [B, O, H, W] dense,
 *   d_logits bf16 (plane (b, t) at base + b * sb_d + t * so_d, so_d >= h * w): the block sum and the product with p (1 - p) are
 *   fp32, rounded once.
 *
 * Answers of (12f)-(12h) before any launch, in this order: DMM_ERR_BAD_ARG for a negative B / O / n_obj, n_obj > O, a size
 * <= 0, a channel range outside d_dst; (12g) DMM_ERR_UNSUPPORTED for H < h or W < w; DMM_OK when there is nothing to do
 * (B == 0, no object, no wanted plane); DMM_ERR_BAD_ARG for a needed null pointer, a negative stride, an output plane stride
 * below the plane, a batch stride below the sample ((12g)); DMM_ERR_UNSUPPORTED for a grid beyond the launch limits.
 * ------------------------------------------------------------------------------------------- */
DMM_API int dmm_mask_pyramid_f32(const float *prev_mask, const float *y_mask, const float *init_pred, int64_t sb_prev,
                                 int64_t so_prev, int64_t sb_y, int64_t so_y, int64_t sb_init, int64_t so_init, int B, int n_obj,
                                 int H, int W, float *out5, float *out4, float *out3, float *out2, dmm_stream_t stream);
DMM_API int dmm_clstm_gates_f32(const float *pre0, const float *pre1, const float *pre2, int64_t sb0, int64_t sb1, int64_t sb2,
                                const float *masks, int64_t sb_masks, const float *w_mask, const float *cell_prev, int B,
                                int hidden_size, int h, int w, float *hidden, float *cell, float *hidden_copy, int64_t sb_copy,
                                dmm_stream_t stream);
DMM_API size_t dmm_clstm_gates_bwd_workspace_bytes(int B, int hidden_size, int h, int w);
DMM_API int dmm_clstm_gates_bwd_f32(const float *pre0, const float *pre1, const float *pre2, int64_t sb0, int64_t sb1, int64_t sb2,
                                    const float *masks, int64_t sb_masks, const float *w_mask, const float *cell_prev, int B,
                                    int hidden_size, int h, int w, const float *d_hidden, const float *d_cell, float *d_pre,
                                    float *d_cell_prev, float *d_masks, float *d_w_mask, void *ws, size_t ws_bytes,
                                    dmm_stream_t stream);
DMM_API int dmm_upsample_bilinear_into_f32(const float *src, int64_t sb_src, int B, int C, int h, int w, float *dst,
                                           int64_t sb_dst, int C_dst, int c0, int H, int W, int mode, dmm_stream_t stream);
DMM_API int dmm_refine_finish_f32(const float *logits, int64_t sb_logits, int64_t so_logits, int h, int w, const int *valid,
                                  int B, int O, int n_obj, int H, int W, float *outs, float *mask_hist, dmm_stream_t stream);
DMM_API int dmm_clstm_gates_bf16(const void *pre0, const void *pre1, const void *pre2, int64_t sb0, int64_t sb1, int64_t sb2,
                                 const float *masks, int64_t sb_masks, const float *w_mask, const float *cell_prev, int B,
                                 int hidden_size, int h, int w, void *hidden, float *cell, void *hidden_copy, int64_t sb_copy,
                                 dmm_stream_t stream);
DMM_API int dmm_upsample_bilinear_into_bf16(const void *src, int64_t sb_src, int B, int C, int h, int w, void *dst,
                                            int64_t sb_dst, int C_dst, int c0, int H, int W, int mode, dmm_stream_t stream);
DMM_API int dmm_refine_finish_bf16(const void *logits, int64_t sb_logits, int64_t so_logits, int h, int w, const int *valid,
                                   int B, int O, int n_obj, int H, int W, float *outs, float *mask_hist, dmm_stream_t stream);
DMM_API int dmm_mask_pyramid_bwd_f32(const float *prev_mask, const float *init_pred, int64_t sb_prev, int64_t so_prev,
                                     int64_t sb_init, int64_t so_init, int B, int n_obj, int H, int W, const float *d_out5,
                                     const float *d_out4, const float *d_out3, const float *d_out2, float *d_prev,
                                     int64_t sb_dprev, int64_t so_dprev, float *d_init, int64_t sb_dinit, int64_t so_dinit,
                                     dmm_stream_t stream);
DMM_API int dmm_upsample_bilinear_bwd_f32(const float *d_dst, int64_t sb_dst, int B, int C, int H, int W, int C_dst, int c0,
                                          float *d_src, int64_t sb_src, int h, int w, dmm_stream_t stream);
DMM_API int dmm_refine_train_finish_f32(const float *logits, int64_t sb_logits, int64_t so_logits, int h, int w, int B, int O,
                                        int n_obj, int H, int W, float *outs, dmm_stream_t stream);
DMM_API int dmm_refine_train_finish_bwd_f32(const float *logits, int64_t sb_logits, int64_t so_logits, int h, int w,
                                            const float *d_outs, int B, int O, int n_obj, int H, int W, float *d_logits,
                                            int64_t sb_d, int64_t so_d, dmm_stream_t stream);
DMM_API int dmm_clstm_gates_bwd_bf16(const void *pre0, const void *pre1, const void *pre2, int64_t sb0, int64_t sb1, int64_t sb2,
                                     const float *masks, int64_t sb_masks, const float *w_mask, const float *cell_prev, int B,
                                     int hidden_size, int h, int w, const void *d_hidden, const float *d_cell, void *d_pre,
                                     float *d_cell_prev, float *d_masks, float *d_w_mask, void *ws, size_t ws_bytes,
                                     dmm_stream_t stream);
DMM_API int dmm_upsample_bilinear_bwd_bf16(const void *d_dst, int64_t sb_dst, int B, int C, int H, int W, int C_dst, int c0,
                                           void *d_src, int64_t sb_src, int h, int w, dmm_stream_t stream);
DMM_API int dmm_refine_train_finish_bf16(const void *logits, int64_t sb_logits, int64_t so_logits, int h, int w, int B, int O,
                                         int n_obj, int H, int W, float *outs, dmm_stream_t stream);
DMM_API int dmm_refine_train_finish_bwd_bf16(const void *logits, int64_t sb_logits, int64_t so_logits, int h, int w,
                                             const float *d_outs, int B, int O, int n_obj, int H, int W, void *d_logits,
                                             int64_t sb_d, int64_t so_d, dmm_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * (13) The soft-IoU mask loss of the trainer's frame step, forward and backward, with the logged hard IoU riding along.
 * Replaces softIoU (dmm/utils/hungarian.py:62-86, need_sigmoid = 0) under softIoULoss (dmm/utils/objectives.py:25-35) as the
 * trainer calls it on the matching layer's output (dmm/modules/trainer.py:205-206) and on the refine decoder's
 * (trainer.py:281-293), together with the hard IoU logged beside each (compute_iou_binary_mask_2D, match_helper.py:9-28, as
 * called from trainer.py:188-196 and :296-300).  Rows are r = (b, t), b < B, t < n_obj <= O; p = pred (fp32 probabilities),
 * y = target as a VALUE (not thresholded in the soft part):
 *   I_r = sum p y      U_r = sum (p + y - p y) + 1e-6      cost_r = 1 - I_r / U_r
 *   sel_r = ((uint8)sw[b, t] != 0) when any sw[b, t] > 0 (b < B, t < n_obj), else 1 for every row;  K = sum sel_r
 *   loss = (1 / K) sum sel_r cost_r          (K == 0: NaN, the reference's mean of an empty selection)
 *   hard_r = float(#(p > 0.5 & y > 0.5)) / (float(#(p > 0.5 | y > 0.5)) + 1e-6)         (strict >, fp32)
 *   nv = sum valid[b, t] over ALL B * O slots (valid == NULL: nv = 0)
 *   hard_valid = sum hard_r valid[b, t] / (nv + 1e-6), hard_all = sum hard_r / (nv + 1e-6); both 0 when nv == 0
 *   d loss / d p[r, i] = sel_r / K * (I_r - (U_r + I_r) y[r, i]) / U_r^2                (nothing else gets a gradient)
 * "any sw > 0" and "nv == 0" are decided on the device: no host read, both entries are graph capturable.  No float atomics:
 * every sum has a fixed order (16 pixels per lane in ascending order, the 64-lane tree, waves in order, chunks in ascending
 * order; the scalars: rows r, r + 256, ... per thread, the 64-lane tree, waves in order), results are bitwise reproducible.
 *
 * dmm_mask_iou_loss_fwd -- two launches.  pred: fp32 planes at pred + b * sb_pred + t * so_pred; target: planes of
 * target_dtype (DMM_F32 / DMM_F16 / DMM_BF16) at strides sb_tgt / so_tgt; a plane is HW contiguous elements, plane strides are
 * at least HW, rows need no alignment beyond their element's.  sw: float [B, >= n_obj], batch stride sb_sw; valid: int32
 * [B, O] dense or NULL.  Writes cost [B, n_obj], hard [B, n_obj], scalars[3] = (loss, hard_valid, hard_all) and the
 * workspace: the coefficient pairs the backward reads, then one 16-byte partial per (row, chunk of DMM_MASK_LOSS_CHUNK
 * pixels).  workspace: dmm_mask_iou_loss_workspace_bytes(B, n_obj, HW) bytes (0 when any of the three is <= 0), 4-byte aligned.
 *
 * dmm_mask_iou_loss_bwd -- one launch.  The SAME workspace after the forward on the same B / n_obj / HW; d_loss: the upstream
 * gradient of `loss`, one fp32 on the DEVICE.  Writes dpred[b, t] (HW contiguous fp32 at dpred + b * sb_dpred + t * so_dpred)
 * for every t < O: the gradient for t < n_obj, zeros for n_obj <= t < O (here O = planes per frame of dpred).  The gradient is
 * evaluated as d_loss * (a_r y + b_r (1 - y)) with the pair a_r = -sel_r / (K U_r), b_r = sel_r I_r / (K U_r^2) -- the formula
 * above with I_r (1 - y) and U_r y kept apart, so that binary targets select a coefficient instead of cancelling two.
 *
 * What both entries answer, in this order (where two faults coincide, the earlier one is named):
 *   1. DMM_ERR_BAD_ARG      B, O, n_obj or HW negative, n_obj > O, a plane stride below HW or a negative batch stride
 *   2. DMM_OK               B == 0, HW == 0, n_obj == 0 (forward) or O == 0 (backward): nothing to do, pointers not looked at
 *   3. DMM_ERR_BAD_ARG      a null pointer other than valid and the workspace
 *   4. DMM_ERR_UNSUPPORTED  target_dtype is none of the three, or more than 65535 planes (B * O)
 *   5. DMM_ERR_WORKSPACE    the workspace is null or shorter than dmm_mask_iou_loss_workspace_bytes
 * ------------------------------------------------------------------------------------------- */
#define DMM_MASK_LOSS_CHUNK 4096 /* pixels of one row per workgroup of the partials and backward kernels */
DMM_API size_t dmm_mask_iou_loss_workspace_bytes(int B, int n_obj, int HW);
DMM_API int dmm_mask_iou_loss_fwd(const float *pred, int64_t sb_pred, int64_t so_pred, const void *target, int target_dtype,
                                  int64_t sb_tgt, int64_t so_tgt, const float *sw, int64_t sb_sw, const int *valid, int B,
                                  int O, int n_obj, int HW, float *cost, float *hard, float scalars[3], void *workspace,
                                  size_t workspace_bytes, dmm_stream_t stream);
DMM_API int dmm_mask_iou_loss_bwd(const void *target, int target_dtype, int64_t sb_tgt, int64_t so_tgt, const float *d_loss,
                                  int B, int O, int n_obj, int HW, const void *workspace, size_t workspace_bytes,
                                  float *dpred, int64_t sb_dpred, int64_t so_dpred, dmm_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * (14) The integer counts under the DAVIS measures of a clip: region similarity J and boundary accuracy F per frame and object.
 * Replaces the pixel work of db_eval_iou (dmm/measures/jaccard.py:15-37) and db_eval_boundary with seg2bmap
 * (dmm/measures/f_boundary.py:14-78 and :80-140; skimage's binary_dilation by disk(bound_pix) at :47-50) as db_eval_sequence
 * calls them on `an == obj_id, sg == obj_id` (dmm/dataloader/evaluation.py:44-46).  The divisions and the case analysis of
 * the two measures stay on the host (dmm_net_amd/measures.py): everything here is an integer, equal to the reference bit for bit.
 *
 * pred, gt: uint8 label maps, frame f at pred + f * frame_stride_pred (gt likewise), H dense rows of W pixels; 0 = background,
 * o + 1 = object o; a label above n_obj belongs to no object.  For frame f and object o, S = (pred == o + 1), A = (gt == o + 1):
 *   counts[f, o, 0] = #(S & A)                       counts[f, o, 1] = #(S | A)
 *   counts[f, o, 2] = #bmap(S)          (n_fg)       counts[f, o, 3] = #bmap(A)          (n_gt)
 *   counts[f, o, 4] = #(bmap(S) & dil(bmap(A)))      counts[f, o, 5] = #(bmap(A) & dil(bmap(S)))
 * (slot 4 / slot 2 is the reference's precision, slot 5 / slot 3 its recall: its names fg_match / gt_match are crossed.)
 * bmap is seg2bmap at equal size: with e, s, se the mask shifted by one pixel towards the origin from the east, the south
 * and the south-east (zero where the shift leaves the image), b = (m ^ e) | (m ^ s) | (m ^ se); then the last row is
 * m ^ e, then the last column is m ^ s, then the bottom-right pixel is 0 -- in this order, which decides the corner and the
 * 1 x W and H x 1 images.  dil is the binary dilation by the disk dx * dx + dy * dy <= radius * radius, zeros outside the image.
 *
 * Two launches (a clearing kernel, not a memset node, then the counts); no host synchronisation, no allocation: capturable.
 * Band partials meet in `counts` by integer atomics, so the bytes are the same on every run and the workspace is empty:
 * dmm_davis_counts_workspace_bytes answers 0 today and callers still ask it.  A workgroup owns DMM_DAVIS_BAND_ROWS(radius)
 * rows (fewer when H is smaller) of a column tile of 64-pixel words.
 *
 * What the entry answers, in this order (where two faults coincide, the earlier one is named):
 *   1. DMM_ERR_BAD_ARG      frames, n_obj, H, W or radius negative, or a frame stride below H * W
 *   2. DMM_OK               frames == 0 or n_obj == 0: nothing to do, nothing launched, pointers not looked at
 *   3. DMM_ERR_BAD_ARG      pred, gt or counts null
 *   4. DMM_ERR_UNSUPPORTED  radius > DMM_DAVIS_MAX_RADIUS, n_obj > 255, H * W >= 2^31, or 2^31 or more workgroups / count words
 *   5. DMM_ERR_WORKSPACE    the workspace is null or shorter than dmm_davis_counts_workspace_bytes (when that is not 0)
 * H == 0 or W == 0 (after these checks): every count is 0.
 * ------------------------------------------------------------------------------------------- */
#define DMM_DAVIS_MAX_RADIUS 63 /* a horizontal shift crosses at most one 64-bit word boundary */
#define DMM_DAVIS_BAND_ROWS(radius) (3 * (radius) + 8 < 16 ? 16 : 3 * (radius) + 8 > 64 ? 64 : 3 * (radius) + 8)
DMM_API size_t dmm_davis_counts_workspace_bytes(int frames, int n_obj, int H, int W, int radius);
DMM_API int dmm_davis_counts_u8(const uint8_t *pred, const uint8_t *gt, int frames, int n_obj, int H, int W,
                                int64_t frame_stride_pred, int64_t frame_stride_gt, int radius, int32_t *counts, void *workspace,
                                size_t workspace_bytes, dmm_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * (14b), (14d) The nearest resize of a prediction whose size Hs x Ws is not the annotation's H x W, so that (14) can score it.
 * Replaces the resize both measures make first -- Image.resize((w, h), Image.NEAREST) of the prediction at
 * dmm/measures/jaccard.py:28-32 and dmm/measures/f_boundary.py:34-38 -- which is PIL's ImagingScaleAffine: per axis a source
 * coordinate walked by repeated double additions, NOT floor((i + 0.5) * n_in / n_out) (the two differ on 448 -> 854).
 * The index rule, for one axis of n_in source and n_out destination samples:
 *   a = (double)n_in / (double)n_out;  o = a * 0.5;
 *   for i in 0 .. n_out - 1:  tab[i] = (o < 0 ? -1 : (int)o);  o += a;          (sequential double additions)
 * Destination pixel (y, x) reads source pixel (tab_y[y], tab_x[x]); an index outside [0, n_in) reads as label 0 (PIL leaves
 * that pixel of its zeroed output unset).  `a` is formed on the host, in the launcher, by exactly that C division; the
 * additions run on the device, one after the other, in IEEE double (the library is built without contraction or fast-math).
 * The radius of (14) stays the caller's: the reference takes bound_pix from the prediction's shape BEFORE the resize
 * (f_boundary.py:30-31), which dmm_net_amd/measures.py follows.
 *
 * (14b) dmm_nearest_index_tables_i32 writes tables[0 .. H) = tab_y (Hs -> H) and tables[H .. H + W) = tab_x (Ws -> W).  One
 * launch; one lane per axis does the walk.  The tables belong to the caller, who builds them once per size pair and reuses
 * them: a scorer resizes once per frame.  Capturable.  What the entry answers, in this order:
 *   1. DMM_ERR_BAD_ARG      Hs, Ws, H or W negative
 *   2. DMM_OK               H + W == 0: nothing to do, nothing launched, pointer not looked at
 *   3. DMM_ERR_BAD_ARG      tables null
 *   4. DMM_ERR_UNSUPPORTED  Hs, Ws, H or W above DMM_NEAREST_MAX_AXIS
 *
 * (14c) is not there: dmm_davis_counts_resized_u8, (14) with its prediction load a gather through the tables, was built and
 * measured against (14d) followed by (14) and was the slower of the two (profiles/r13_davis_resized.md: each object's
 * workgroups repeat the gather that (14d) makes once).  Resized scoring is (14d) into a buffer, then (14).
 *
 * (14d) dmm_resize_labels_nearest_u8 is the resize: dst[f, y, x] = src[f, tab_y[y], tab_x[x]], frame f at
 * src + f * frame_stride_src and dst + f * frame_stride_dst, dense rows; `tables` is read as it stands (any int32 values: an
 * entry outside the source reads as label 0).  One launch, no host read, no allocation: capturable.  What it answers, in order:
 *   1. DMM_ERR_BAD_ARG      frames, Hs, Ws, H or W negative, frame_stride_src below Hs * Ws or frame_stride_dst below H * W
 *   2. DMM_OK               frames == 0, H == 0 or W == 0: nothing to do, nothing launched, pointers not looked at
 *   3. DMM_ERR_BAD_ARG      src, dst or tables null, or dst == src (a gather cannot run in place)
 *   4. DMM_ERR_UNSUPPORTED  H * W or Hs * Ws >= 2^31, or DMM_RESIZE_MAX_WORKGROUPS or more workgroups, where a workgroup writes
 *                           1024 bytes and a frame takes ceil((ceil(H * W / 4) + 1) / 256) of them (the grid stays below
 *                           2^32 threads: split a larger clip into several calls)
 * ------------------------------------------------------------------------------------------- */
#define DMM_RESIZE_MAX_WORKGROUPS 16777216 /* 2^24 workgroups of 256 threads: 16 GiB of labels in one call */
#define DMM_NEAREST_MAX_AXIS 16384 /* one lane walks an axis, one dependent double addition per sample: the cap bounds (14b) */
DMM_API int dmm_nearest_index_tables_i32(int Hs, int Ws, int H, int W, int32_t *tables, dmm_stream_t stream);
DMM_API int dmm_resize_labels_nearest_u8(const uint8_t *src, int Hs, int Ws, int64_t frame_stride_src, uint8_t *dst, int H, int W,
                                         int64_t frame_stride_dst, const int32_t *tables, int frames, dmm_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * (15) The augmentation of training clips: one nearest-neighbour affine warp per frame, applied to the image planes, the
 * annotation and every pasted proposal mask, with the proposals' boxes and the target planes out of the same pass.  Replaces
 * the per-plane Python loop of dmm/dataloader/dataset.py:222-258 -- the clip's flip, Affine(tf_matrix, interp='nearest')
 * (th_affine2d(center=True) + th_nearest_interp2d, dmm/dataloader/transforms/utils.py:67-148) on img, annot and each mask,
 * binmask_to_bbox_xyxy_pt (dmm/utils/utils.py:114-143, pad = 0) of each warped mask > 0.5 -- and sequence_from_masks
 * (dataset.py:300-338) on the warped annotation.
 *
 * n frames (a clip, or clips back to back).  Frame f has its own row-major 3 x 3 fp32 matrix m = matrices + 9 f (the last row
 * is not read) and its own flip flag flips[f] (the reference flips a whole clip: repeat the flag; flips == NULL: none).  The
 * source of output pixel (r, c), in fp32 with one rounding per operation, in exactly this order:
 *   cr = H / 2 - 0.5,  cc = W / 2 - 0.5                   (formed in double, rounded to fp32 once)
 *   x  = float(r) - cr;  y = float(c) - cc
 *   sr = (((m[0] * x) + (m[1] * y)) + m[2]) + cr
 *   sc = (((m[3] * x) + (m[4] * y)) + m[5]) + cc
 *   ri = (int) rintf(min(max(sr, 0), H - 1))              (clamp BEFORE rounding; ties to even)
 *   ci = (int) rintf(min(max(sc, 0), W - 1))
 *   if flips[f]: ci = W - 1 - ci                          (the reference flips first and warps the flipped frame)
 * and out[r, c] = in[ri, ci] for every plane of the frame (a plane is H dense rows of W elements):
 *   C image planes   fp32, plane ch of frame f at frames_in + f * fs_frames_in + ch * ps_frames_in (frames_out likewise)
 *   1 label plane    uint8, frame f at labels_in + f * fs_labels_in (labels_out likewise)
 *   P mask planes    fp32 soft masks at masks_in + f * fs_masks_in + p * ps_masks_in (masks_out likewise); P may be 0
 * Strides are in elements; output planes must not overlap each other or any input.
 *   boxes_out [n, P, 4] fp32 xyxy, box_valid [n, P] int32: the inclusive min / max column and row of (masks_out[f, p] > 0.5)
 *     (strict) and 1; where the warped mask has no such pixel, boxes_in[f, p] copied through and 0 (the reference keeps the
 *     old box).  Until the last launch boxes_out holds the integer table the workgroups meet in.
 *   targets [n, F, H, W] fp32 dense: targets[f, o] = (labels_out[f] == o + 1) as 1.0 / 0.0; sizes [n, F] int32: its pixel
 *     count.  Labels 0, 255 and anything above F belong to no plane.  (Label 0 is ALWAYS background: the reference's
 *     np.unique(annot)[1:] drops the smallest object id of a frame without a background pixel; that is not reproduced.)
 *
 * At most three launches: a clearing kernel for the two integer tables (a kernel, not a memset node), the warp, and -- when
 * P > 0 -- the box finish.  No host synchronisation, no allocation: capturable.  Boxes meet by integer max and sizes by
 * integer add, both order-free, so the bytes are the same on every run and the workspace is empty:
 * dmm_augment_clip_workspace_bytes answers 0 today and callers still ask it.
 *
 * What the entry answers, in this order (where two faults coincide, the earlier one is named):
 *   1. DMM_ERR_BAD_ARG      n, C, P, F, H or W negative; a frame stride of the labels below H * W; with C > 0 a frame or plane
 *                           stride of the image planes below H * W; with P > 0 likewise of the mask planes
 *   2. DMM_OK               n == 0, H == 0 or W == 0: nothing to do, nothing launched, nothing written, pointers not looked at
 *   3. DMM_ERR_BAD_ARG      labels_in, labels_out or matrices null; with C > 0 frames_in or frames_out; with P > 0 masks_in,
 *                           masks_out, boxes_in, boxes_out or box_valid; with F > 0 targets or sizes; or an output that IS its
 *                           input (labels, frames, masks, boxes): a gather cannot run in place
 *   4. DMM_ERR_UNSUPPORTED  H * W >= 2^31, F > DMM_AUGMENT_MAX_TARGETS, or 2^31 or more workgroups, box words or size words
 *   5. DMM_ERR_WORKSPACE    the workspace is null or shorter than dmm_augment_clip_workspace_bytes (when that is not 0)
 * ------------------------------------------------------------------------------------------- */
#define DMM_AUGMENT_MAX_TARGETS 254 /* label 255 is "ignore" in DAVIS 2017 and is never a target plane */
DMM_API size_t dmm_augment_clip_workspace_bytes(int n, int C, int P, int F, int H, int W);
DMM_API int dmm_augment_clip_f32(const float *frames_in, int64_t fs_frames_in, int64_t ps_frames_in, float *frames_out,
                                 int64_t fs_frames_out, int64_t ps_frames_out, const uint8_t *labels_in, int64_t fs_labels_in,
                                 uint8_t *labels_out, int64_t fs_labels_out, const float *masks_in, int64_t fs_masks_in,
                                 int64_t ps_masks_in, float *masks_out, int64_t fs_masks_out, int64_t ps_masks_out,
                                 const float *boxes_in, float *boxes_out, int32_t *box_valid, float *targets, int32_t *sizes,
                                 const float *matrices, const int32_t *flips, int n, int C, int P, int F, int H, int W,
                                 void *workspace, size_t workspace_bytes, dmm_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * (16) Frames as the encoders take them, from decoded images: PIL's resize of an 8-bit RGB image, then ToTensor and Normalize.
 * Replaces what the reference's dataset workers do per frame -- Image.open(jpg).resize((W, H)) at dmm/dataloader/dataset.py:
 * 202-219, then transforms.ToTensor() and transforms.Normalize(mean, std), composed at train.py:76-77 and eval.py:51-52.
 * Everything is an integer or a table look-up: the result equals the host pipeline bit for bit.
 *
 * A source frame is uint8 [Hs, Ws, 3], pixel-interleaved (np.array(Image.open(...))): frame f at src + f * fs_src, row y at
 * + y * rs_src, 3 * Ws dense bytes per row.  The destination is H x W.
 *
 * Coefficient tables (dmm_prepare_frames_u8).  Per axis with n_in -> n_out the caller forms, on the host in IEEE double and in
 * exactly this order (PIL's precompute_coeffs and normalize_coeffs_8bpc; dmm_net_amd/frames.py resample_tables):
 *   scale = n_in / n_out;  fs = max(scale, 1.0);  support = filter_support * fs;  ksize = (int)ceil(support) * 2 + 1
 *   for i in 0 .. n_out - 1:
 *     center = (i + 0.5) * scale;  ss = 1.0 / fs
 *     lo  = max((int)(center - support + 0.5), 0)
 *     cnt = min((int)(center + support + 0.5), n_in) - lo
 *     w[k] = filter((k + lo - center + 0.5) * ss)  for k in 0 .. cnt - 1
 *     ww   = w[0] + w[1] + ...                                              (left to right)
 *     if ww != 0: w[k] /= ww
 *     coef[i][k] = (int)(w[k] * 2^22 + 0.5) if w[k] >= 0 else (int)(w[k] * 2^22 - 0.5)      ((int) truncates toward zero)
 *     coef[i][cnt ..] = 0;  bounds[i] = (lo, cnt)
 *   bilinear(x) (support 1):          x = |x|;  x < 1 ? 1 - x : 0
 *   bicubic(x)  (support 2, a = -0.5): x = |x|;  x < 1 ? ((a + 2) * x - (a + 3)) * x * x + 1 : x < 2 ? (((x - 5) * x + 8) * x - 4) * a : 0
 * bounds is int32 [n_out, 2], coef int32 [n_out, ksize], both dense.  One pass along an axis, per channel:
 *   acc = 2^21 + sum_k coef[i][k] * src[lo + k]          (int32, wrapping)
 *   out = clamp(acc >> 22, 0, 255)                       (arithmetic shift)
 * The horizontal pass runs first into a uint8 intermediate [Hs, W, 3], the vertical pass follows into [H, W, 3]; the uint8
 * rounding between them is part of the result.  A pass whose axis does not change size is skipped: no table, no launch, the
 * same bytes.  The tables are read as they stand: lo is clamped into [0, n_in] and cnt into [0, min(ksize, n_in - lo)], so
 * no values in them make a kernel read outside the source.
 *
 * Nearest (dmm_prepare_frames_nearest_u8).  PIL's affine walk, i.e. the index tables of (14b) as dmm_nearest_index_tables_i32
 * writes them (tab_y [H], then tab_x [W]): dst[y, x, :] = src[tab_y[y], tab_x[x], :]; an index outside the source reads as 0.
 *
 * Normalisation.  out[c, y, x] = lut[c * 256 + u8], lut fp32 [3, 256] formed by the caller with the reference's own operations
 * (dmm_net_amd/frames.py normalise_lut), so no device rounding enters.  out_f32: plane c of frame f at
 * out_f32 + f * fs_out + c * ps_out, H dense rows of W floats (a slice of a larger batch is addressable).  out_u8: the resized
 * image itself, what PIL returns, frame f at out_u8 + f * fs_u8, interleaved and dense.  Either may be null, not both; lut is
 * needed with out_f32.  Strides are in elements.
 *
 * Launches: one per pass that runs -- at most two; one when one axis keeps its size, when both do (a copy through the look-up)
 * and for nearest.  The last launch writes both outputs.  The horizontal kernel stages the span of each source row its columns
 * need in LDS and writes the intermediate into the workspace with a row pitch of 3 * W rounded up to 16 bytes;
 * dmm_prepare_frames_workspace_bytes is that, n * Hs rows of it, when both axes change and 0 otherwise (and for nearest).
 * No allocation, no host read: capturable.
 *
 * What the entries answer, in this order (where two faults coincide, the earlier one is named):
 *   1. DMM_ERR_BAD_ARG      n, C, Hs, Ws, H, W or a ksize negative; rs_src below 3 * Ws, fs_src below Hs * 3 * Ws; with out_f32
 *                           given ps_out or fs_out below H * W; with out_u8 given fs_u8 below H * W * 3
 *   2. DMM_OK               n == 0, H == 0 or W == 0: nothing to do, nothing launched, pointers not looked at
 *   3. DMM_ERR_BAD_ARG      src null (unless Hs * Ws == 0 under nearest, where nothing is read); out_f32 and out_u8 both null;
 *                           lut null with out_f32 given; bounds_x or coef_x null, or ksize_x == 0, when Ws != W, and likewise
 *                           for y when Hs != H (a table is required exactly when its axis changes size); tables null (nearest)
 *   4. DMM_ERR_UNSUPPORTED  C != 3 (other modes are out of scope); Hs, Ws, H or W above DMM_NEAREST_MAX_AXIS; Hs or Ws == 0 with a table pass (PIL refuses an empty
 *                           image); a required ksize above DMM_RESAMPLE_MAX_TAPS; Hs * Ws * 3, H * W * 3 or Hs * W * 3 >= 2^31,
 *                           or DMM_RESIZE_MAX_WORKGROUPS or more workgroups in a launch (a grid stays below 2^32 threads: split
 *                           a larger clip set into several calls)
 *   5. DMM_ERR_WORKSPACE    the workspace is null, shorter than dmm_prepare_frames_workspace_bytes or not 16-byte aligned
 *                           (when that size is not 0)
 * ------------------------------------------------------------------------------------------- */
#define DMM_RESAMPLE_MAX_TAPS 257 /* ksize of a 64-fold bicubic (128-fold bilinear) reduction */
DMM_API size_t dmm_prepare_frames_workspace_bytes(int n, int Hs, int Ws, int H, int W);
DMM_API int dmm_prepare_frames_u8(const uint8_t *src, int64_t fs_src, int64_t rs_src, int n, int C, int Hs, int Ws, int H,
                                  int W, const int32_t *bounds_x, const int32_t *coef_x, int ksize_x, const int32_t *bounds_y,
                                  const int32_t *coef_y, int ksize_y, const float *lut, float *out_f32, int64_t fs_out,
                                  int64_t ps_out, uint8_t *out_u8, int64_t fs_u8, void *workspace, size_t workspace_bytes,
                                  dmm_stream_t stream);
DMM_API int dmm_prepare_frames_nearest_u8(const uint8_t *src, int64_t fs_src, int64_t rs_src, int n, int C, int Hs, int Ws, int H,
                                          int W, const int32_t *tables, const float *lut, float *out_f32, int64_t fs_out, int64_t ps_out,
                                          uint8_t *out_u8, int64_t fs_u8, dmm_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* DMM_MATCH_H */
