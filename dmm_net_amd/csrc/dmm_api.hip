// dmm_api.hip -- C-ABI glue of libdmm_match.so: status/reporting and the one-call forward entries that chain the
// kernels of MatchModel.forward (dmm/modules/match_model.py:24-47) on one stream: validate, carve the workspace, front
// (similarity + counts: match_front, dmm_front.hip), solver, mix.
#include <limits.h>
#include <stdlib.h>

#include <atomic>

#include "dmm_launchers.h"
#include "dmm_solve.h"

namespace dmm {
static thread_local int g_last_hip_error = 0;
void set_last_hip_error(int e) { g_last_hip_error = e; }
static std::atomic<long long> g_launches{0};
void note_launch() { g_launches.fetch_add(1, std::memory_order_relaxed); }

// ---- dispatch options -------------------------------------------------------------------------------------------------
static constexpr int kOptDefaults[DMM_OPT_COUNT] = {
    /* COST_KERNEL */ -1,      /* COST_TINY_FRAMES */ 8,   /* SOLVER_KERNEL */ -1,  /* FORCE_WIDE */ 0,
    /* COSINE_KERNEL */ 0,     /* COST_WGS */ 8192,        /* COST_SMALL_WGS */ 512, /* COST_TL_WGS */ 512,
    /* COST_XCD */ 1,          /* MIX_XCD */ 3,            /* MIX_WGS */ 320000,    /* MIX_STEPQ */ 2,
    /* MIX_ALIGN */ 128,       /* MIX_NT */ 3,             /* SOLVER_HELPER_MAX */ 512, /* NMS_WAVE */ 1,
    /* COS_ROWS_MIN_N */ 65,   /* GEMM_TUNE */ 1,          /* PACK_VARIANT */ 4,    /* SMALL_FUSED */ 1,
    /* MIX_SHARED */ -1,       /* MIX_SHARED_STEPS */ 1,   /* FEAT_BWD_FRAME */ -1, /* MIX_SHARED_LOCKSTEP */ 1,
};
static std::atomic<int> g_opts[DMM_OPT_COUNT] = {
    {kOptDefaults[0]},  {kOptDefaults[1]},  {kOptDefaults[2]},  {kOptDefaults[3]},  {kOptDefaults[4]},
    {kOptDefaults[5]},  {kOptDefaults[6]},  {kOptDefaults[7]},  {kOptDefaults[8]},  {kOptDefaults[9]},
    {kOptDefaults[10]}, {kOptDefaults[11]}, {kOptDefaults[12]}, {kOptDefaults[13]}, {kOptDefaults[14]},
    {kOptDefaults[15]}, {kOptDefaults[16]}, {kOptDefaults[17]}, {kOptDefaults[18]}, {kOptDefaults[19]},
    {kOptDefaults[20]}, {kOptDefaults[21]}, {kOptDefaults[22]}, {kOptDefaults[23]},
};
static_assert(DMM_OPT_COUNT == 24, "kOptDefaults / g_opts list every option");
int opt(int key) { return g_opts[key].load(std::memory_order_relaxed); }

static inline size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

struct Workspace {
    int32_t *inter, *area_p, *area_t;
    float *featn_p, *featn_t, *cosv, *sim, *Rb;
    float *wide;                       // solver state of the general kernel (tables outside the compiled envelope)
    size_t bytes;
};

// tables the fast solver kernels are not compiled for: the general forms of dmm_wide.hip take them
// (DMM_OPT_FORCE_WIDE: tests send tables inside the envelope there too)
static bool wide_shape(int N, int M) {
    const int Pp = N > M ? N : M + 1;
    return M > DMM_MAX_TEMPLATES || Pp > DMM_MAX_PROPOSALS || opt(DMM_OPT_FORCE_WIDE) == 1;
}

static Workspace carve(void *base, int B, int N, int M, int D) {
    const int Pp = N > M ? N : M + 1;
    Workspace w;
    size_t off = 0;
    auto take = [&](size_t n) {
        void *p = base ? (void *)((char *)base + off) : nullptr;
        off += align_up(n, 256);
        return p;
    };
    // inter | area_p | area_t back to back: the front clears them in one pass (match_front, dmm_front.hip)
    w.inter = (int32_t *)take(sizeof(int32_t) * ((size_t)B * M * N + (size_t)B * N + (size_t)B * M));
    w.area_p = w.inter ? w.inter + (size_t)B * M * N : nullptr;
    w.area_t = w.area_p ? w.area_p + (size_t)B * N : nullptr;
    w.featn_p = (float *)take(sizeof(float) * (size_t)B * N * D);
    w.featn_t = (float *)take(sizeof(float) * (size_t)B * M * D);
    w.cosv = (float *)take(sizeof(float) * (size_t)B * M * N);
    w.sim = (float *)take(sizeof(float) * (size_t)B * M * N);
    w.Rb = (float *)take(sizeof(float) * (size_t)B * M * Pp);
    w.wide = nullptr;
    if (wide_shape(N, M))                                        // the one test both the sizes and the dispatch use
        w.wide = (float *)take(sizeof(float) * (size_t)B * wide_scratch_floats(M, Pp));
    w.bytes = off;
    return w;
}

static float *or_ws(float *out, float *ws) { return out ? out : ws; }   // an output the caller did not ask for: workspace

// the front on the carved workspace: cosine into w.cosv, counts into the three tables (the entry sets the flags)
static Front ws_front(const Workspace &w, const void *masks_p, const void *masks_t, int dtype, int64_t sp_b, int64_t sp_n,
                      int64_t st_b, int64_t st_m, const float *feat_p, const float *feat_t, int B, int N, int M, int HW, int D,
                      const int32_t *n_valid, const int32_t *m_valid) {
    Front f{};
    f.masks_p = masks_p; f.masks_t = masks_t; f.dtype = dtype;
    f.sp_b = sp_b; f.sp_n = sp_n; f.st_b = st_b; f.st_m = st_m;
    f.feat_p = feat_p; f.feat_t = feat_t;
    f.B = B; f.N = N; f.M = M; f.HW = HW; f.D = D;
    f.n_valid = n_valid; f.m_valid = m_valid;
    f.cos = w.cosv;
    f.inter = w.inter; f.area_p = w.area_p; f.area_t = w.area_t;
    f.table_words = (size_t)B * M * N + (size_t)B * N + (size_t)B * M;
    f.featn_p = w.featn_p; f.featn_t = w.featn_t;
    return f;
}
// the front of the entries whose planes are 1-bit words on both sides (dmm_pack_words(HW) per plane)
static Front packed_front(const Workspace &w, const uint64_t *packed_p, int64_t pk_b, int64_t pk_n, const uint64_t *packed_t,
                          const float *feat_p, const float *feat_t, int B, int N, int M, int HW, int D,
                          const int32_t *n_valid, const int32_t *m_valid) {
    const int64_t wd = dmm_pack_words(HW);
    Front f = ws_front(w, packed_p, packed_t, DMM_PACKED1, pk_b, pk_n, (int64_t)M * wd, wd, feat_p, feat_t, B, N, M, HW, D,
                       n_valid, m_valid);
    f.ragged_lanes = true;
    return f;
}
}  // namespace dmm

extern "C" int dmm_abi_version(void) { return DMM_ABI_VERSION; }

extern "C" int dmm_set_option(int option, int value) {
    if (option < 0 || option >= DMM_OPT_COUNT) return DMM_ERR_BAD_ARG;
    switch (option) {                                            // ranges: a bad value must not reach a launch computation
        case DMM_OPT_FEAT_BWD_FRAME: if (value < -1 || value > 2) return DMM_ERR_BAD_ARG; break;
        case DMM_OPT_COST_KERNEL: case DMM_OPT_SOLVER_KERNEL: case DMM_OPT_MIX_SHARED:
            if (value < -1 || value > 1) return DMM_ERR_BAD_ARG; break;
        case DMM_OPT_MIX_XCD: if (value < 0 || value > 7) return DMM_ERR_BAD_ARG; break;
        case DMM_OPT_FORCE_WIDE: case DMM_OPT_COSINE_KERNEL: case DMM_OPT_COST_XCD:
        case DMM_OPT_NMS_WAVE: case DMM_OPT_SMALL_FUSED: case DMM_OPT_MIX_SHARED_LOCKSTEP:
            if (value < 0 || value > 1) return DMM_ERR_BAD_ARG; break;
        case DMM_OPT_MIX_ALIGN: if (value != 16 && value != 32 && value != 64 && value != 128) return DMM_ERR_BAD_ARG; break;
        case DMM_OPT_MIX_NT: if (value < 0 || value > 3) return DMM_ERR_BAD_ARG; break;
        case DMM_OPT_COST_WGS: case DMM_OPT_COST_SMALL_WGS: case DMM_OPT_COST_TL_WGS: case DMM_OPT_MIX_WGS:
        case DMM_OPT_MIX_STEPQ: case DMM_OPT_GEMM_TUNE: case DMM_OPT_COS_ROWS_MIN_N: case DMM_OPT_MIX_SHARED_STEPS:
            if (value < 1) return DMM_ERR_BAD_ARG; break;
        default: if (value < 0) return DMM_ERR_BAD_ARG; break;
    }
    dmm::g_opts[option].store(value, std::memory_order_relaxed);
    return DMM_OK;
}

extern "C" int dmm_get_option(int option) {
    return (option < 0 || option >= DMM_OPT_COUNT) ? INT_MIN : dmm::opt(option);
}

extern "C" int dmm_reset_options(void) {
    for (int k = 0; k < DMM_OPT_COUNT; ++k) dmm::g_opts[k].store(dmm::kOptDefaults[k], std::memory_order_relaxed);
    return DMM_OK;
}

extern "C" const char *dmm_status_string(int status) {
    switch (status) {
        case DMM_OK: return "ok";
        case DMM_ERR_BAD_ARG: return "bad argument";
        case DMM_ERR_UNSUPPORTED: return "shape outside the compiled kernel envelope";
        case DMM_ERR_LAUNCH: return "HIP launch/runtime error (see dmm_last_hip_error)";
        case DMM_ERR_WORKSPACE: return "workspace too small";
        default: return "unknown status";
    }
}

extern "C" int dmm_last_hip_error(void) { return dmm::g_last_hip_error; }

extern "C" long long dmm_launch_count(void) { return dmm::g_launches.load(std::memory_order_relaxed); }

#define DMM_STR_(x) #x
#define DMM_STR(x) DMM_STR_(x)
extern "C" const char *dmm_build_info(void) { return "libdmm_match gfx950 (CDNA4, wave64) abi " DMM_STR(DMM_ABI_VERSION); }

extern "C" size_t dmm_workspace_bytes(int B, int N, int M, int D) {
    if (B <= 0 || N <= 0 || M <= 0 || D < 0) return 0;
    return dmm::carve(nullptr, B, N, M, D).bytes;
}

extern "C" int dmm_match_forward(const void *masks_p, const void *masks_t, int mask_dtype, const float *feat_p,
                                 const float *feat_t, const float *score_p, int B, int N, int M, int HW, int D,
                                 int64_t sp_b, int64_t sp_n, int64_t st_b, int64_t st_m, const int32_t *n_valid,
                                 const int32_t *m_valid, float score_weight, int max_iter, int proj_iter, float lr,
                                 int is_test, float *full_outmask, float *match_score, float *det_score,
                                 float *sim_out, float *R_out, float *Rb_out, int32_t *iters_out, void *workspace,
                                 size_t workspace_bytes, dmm_stream_t stream) {
    return dmm_match_forward_ws(masks_p, masks_t, mask_dtype, feat_p, feat_t, score_p, B, N, M, HW, D, sp_b, sp_n, st_b, st_m,
                                n_valid, m_valid, score_weight, max_iter, proj_iter, lr, is_test, full_outmask, match_score,
                                det_score, sim_out, R_out, Rb_out, iters_out, workspace, workspace_bytes, nullptr, stream);
}

// (5a') dmm_match_forward for a caller that keeps ONE workspace for a sequence of calls and lets the library remember
// what it left there.  *ws_state in: DMM_WS_TABLES_ZERO if the previous call on this workspace (same B, N, M) returned
// that value, DMM_WS_UNKNOWN otherwise; out: the state the work enqueued by this call leaves behind.  A handful of dense
// frames (the small-batch front kernel) then run without the clearing launch in front of the counts -- a launch is
// ~4.5 us of a ~95 us one-frame call: the solver zeroes every table entry right after reading it.  Every other path
// returns DMM_WS_UNKNOWN.  On an error return the state is DMM_WS_UNKNOWN.
extern "C" int dmm_match_forward_ws(const void *masks_p, const void *masks_t, int mask_dtype, const float *feat_p,
                                    const float *feat_t, const float *score_p, int B, int N, int M, int HW, int D,
                                    int64_t sp_b, int64_t sp_n, int64_t st_b, int64_t st_m, const int32_t *n_valid,
                                    const int32_t *m_valid, float score_weight, int max_iter, int proj_iter, float lr,
                                    int is_test, float *full_outmask, float *match_score, float *det_score,
                                    float *sim_out, float *R_out, float *Rb_out, int32_t *iters_out, void *workspace,
                                    size_t workspace_bytes, int *ws_state, dmm_stream_t stream) {
    const bool tables_zero = ws_state && *ws_state == DMM_WS_TABLES_ZERO;
    if (ws_state) *ws_state = DMM_WS_UNKNOWN;
    bool go;
    int rc = dmm::one_call_check(B, N, M, HW, D, masks_p && masks_t && feat_p && feat_t && score_p && full_outmask &&
                                 match_score && det_score && workspace, &go);
    if (!go) return rc;
    if (!dmm::soft_planes(mask_dtype)) return DMM_ERR_BAD_ARG;   // (reject before any launch)
    const dmm::Workspace w = dmm::carve(workspace, B, N, M, D);
    if (workspace_bytes < w.bytes) return DMM_ERR_WORKSPACE;
    const dmm::SolveIn in{w.cosv, w.inter, w.area_p, w.area_t, score_p, B, N, M, n_valid, m_valid};
    const dmm::SolveOut out{dmm::or_ws(sim_out, w.sim), R_out, dmm::or_ws(Rb_out, w.Rb), match_score, det_score, iters_out,
                            nullptr};
    const dmm::RelaxParams prm{max_iter, proj_iter, lr};
    if (dmm::wide_shape(N, M)) {
        // Outside the envelope of the fast kernels (M <= 32, Pp <= 256): counts (they tile any N x M), the features
        // normalised, then the general kernels -- same operations, same order, any size (dmm_wide.hip).
        if (!w.wide || B > 65535) return DMM_ERR_UNSUPPORTED;
        rc = dmm_iou_counts(masks_p, masks_t, mask_dtype, B, N, M, HW, sp_b, sp_n, st_b, st_m, n_valid, m_valid, w.inter,
                            w.area_p, w.area_t, stream);
        if (rc != DMM_OK) return rc;
        rc = dmm_feature_normalize_f32(feat_p, (int64_t)B * N, D, w.featn_p, nullptr, stream);
        if (rc != DMM_OK) return rc;
        rc = dmm_feature_normalize_f32(feat_t, (int64_t)B * M, D, w.featn_t, nullptr, stream);
        if (rc != DMM_OK) return rc;
        rc = dmm::launch_cosine_wide(w.featn_t, w.featn_p, B, N, M, D, n_valid, m_valid, w.cosv, (hipStream_t)stream);
        if (rc != DMM_OK) return rc;
        rc = dmm::solve_entry_check(in, out, max_iter, proj_iter, false, &is_test, &go);
        if (!go) return rc;
        float w_feat, w_iou;
        dmm::sim_weights(score_weight, w_feat, w_iou);
        rc = dmm::launch_relax_match_wide(in, w_feat, w_iou, prm, is_test, out, w.wide, (hipStream_t)stream);
        if (rc != DMM_OK) return rc;
        return dmm_mask_mix(out.Rb, masks_p, mask_dtype, B, N, M, dmm::padded_width(N, M), HW, sp_b, sp_n, n_valid, m_valid,
                            full_outmask, (int64_t)M * HW, HW, stream);
    }
    // ragged batches keep the three-launch similarity here; dense ones may take the tile kernel
    dmm::Front f = dmm::ws_front(w, masks_p, masks_t, mask_dtype, sp_b, sp_n, st_b, st_m, feat_p, feat_t, B, N, M, HW, D,
                                 n_valid, m_valid);
    f.tables_zero = tables_zero;
    f.dense_tile = true;
    f.split_norm = true;
    bool fused;
    rc = dmm::match_front(f, (hipStream_t)stream, &fused);
    if (rc != DMM_OK) return rc;
    // behind the fused front the solver reads the tables and (asked to) leaves them zero for the next call on this workspace
    int cleared = 0;
    rc = dmm::relax_match_launch(in, score_weight, prm, is_test, out, fused && ws_state, &cleared, stream);
    if (rc != DMM_OK) return rc;
    rc = dmm::match_mix(out.Rb, masks_p, mask_dtype, B, N, M, HW, sp_b, sp_n, n_valid, m_valid, is_test, full_outmask, stream);
    if (rc == DMM_OK && ws_state && cleared) *ws_state = DMM_WS_TABLES_ZERO;
    return rc;
}

// ---------------------------------------------------------------------------------------------
// (5b) The same forward with the proposal side of the cost pass on 1-bit planes (DMM_PACKED1) that the caller already
// holds -- dmm_paste_masks_f32 / dmm_paste_kept_f32 emit them next to the soft planes.  The M template planes of each
// frame are packed here (one read of them, what the float count kernel would have read anyway), the counts run on the
// words (1/32 of the proposal bytes, identical integer tables), the mix reads the soft planes.
// ---------------------------------------------------------------------------------------------
static size_t packed_t_bytes(int B, int M, int HW) {
    return dmm::align_up(sizeof(uint64_t) * (size_t)B * M * (size_t)dmm_pack_words(HW), 256);
}

extern "C" size_t dmm_workspace_bytes_packed(int B, int N, int M, int D, int HW) {
    if (B <= 0 || N <= 0 || M <= 0 || D < 0 || HW < 0) return 0;
    return dmm::carve(nullptr, B, N, M, D).bytes + packed_t_bytes(B, M, HW);
}

extern "C" int dmm_match_forward_packed(const void *masks_p, const uint64_t *packed_p, const void *masks_t, int mask_dtype,
                                        const float *feat_p, const float *feat_t, const float *score_p, int B, int N, int M,
                                        int HW, int D, int64_t sp_b, int64_t sp_n, int64_t pk_b, int64_t pk_n, int64_t st_b,
                                        int64_t st_m, const int32_t *n_valid, const int32_t *m_valid, float score_weight,
                                        int max_iter, int proj_iter, float lr, int is_test, float *full_outmask,
                                        float *match_score, float *det_score, float *sim_out, float *R_out, float *Rb_out,
                                        int32_t *iters_out, void *workspace, size_t workspace_bytes, dmm_stream_t stream) {
    bool go;
    int rc = dmm::one_call_check(B, N, M, HW, D, masks_p && packed_p && masks_t && feat_p && feat_t && score_p &&
                                 full_outmask && match_score && det_score && workspace, &go);
    if (!go) return rc;
    if (!dmm::in_fast_envelope(N, M)) return DMM_ERR_UNSUPPORTED;
    if (!dmm::soft_planes(mask_dtype)) return DMM_ERR_BAD_ARG;
    if (st_b != (int64_t)M * st_m) return DMM_ERR_UNSUPPORTED;          // templates: one plane stride over the batch
    const dmm::Workspace w = dmm::carve(workspace, B, N, M, D);
    if (workspace_bytes < w.bytes + packed_t_bytes(B, M, HW)) return DMM_ERR_WORKSPACE;
    uint64_t *packed_t = (uint64_t *)((char *)workspace + w.bytes);
    const dmm::SolveIn in{w.cosv, w.inter, w.area_p, w.area_t, score_p, B, N, M, n_valid, m_valid};
    const dmm::SolveOut out{dmm::or_ws(sim_out, w.sim), R_out, dmm::or_ws(Rb_out, w.Rb), match_score, det_score, iters_out,
                            nullptr};
    rc = dmm_pack_masks(masks_t, mask_dtype, (int64_t)B * M, HW, st_m, packed_t, dmm_pack_words(HW), stream);
    if (rc != DMM_OK) return rc;
    rc = dmm::match_front(dmm::packed_front(w, packed_p, pk_b, pk_n, packed_t, feat_p, feat_t, B, N, M, HW, D, n_valid, m_valid),
                          (hipStream_t)stream);
    if (rc != DMM_OK) return rc;
    rc = dmm::relax_match_launch(in, score_weight, {max_iter, proj_iter, lr}, is_test, out, 0, nullptr, stream);
    if (rc != DMM_OK) return rc;
    return dmm::match_mix(out.Rb, masks_p, mask_dtype, B, N, M, HW, sp_b, sp_n, n_valid, m_valid, is_test, full_outmask, stream);
}

// (5c) Cost + assignment of the fixed-slot frame step, BOTH sides of the cost pass on 1-bit planes and no mix: the
// proposals' words from dmm_paste_kept_f32, the templates' words from the previous frame's dmm_step_finish_f32.
// cosine (also clears the count tables) -> counts on the words -> solver; Rb / scores / iters out.
extern "C" int dmm_match_solve_packed(const uint64_t *packed_p, const uint64_t *packed_t, const float *feat_p,
                                      const float *feat_t, const float *score_p, int B, int N, int M, int HW, int D,
                                      const int32_t *n_valid, const int32_t *m_valid, float score_weight, int max_iter,
                                      int proj_iter, float lr, int is_test, float *Rb_out, float *match_score,
                                      float *det_score, float *sim_out, float *R_out, int32_t *iters_out, void *workspace,
                                      size_t workspace_bytes, dmm_stream_t stream) {
    bool go;
    int rc = dmm::one_call_check(B, N, M, HW, D, packed_p && packed_t && feat_p && feat_t && score_p && Rb_out &&
                                 match_score && det_score && workspace, &go);
    if (!go) return rc;
    if (!dmm::in_fast_envelope(N, M)) return DMM_ERR_UNSUPPORTED;
    const dmm::Workspace w = dmm::carve(workspace, B, N, M, D);
    if (workspace_bytes < w.bytes) return DMM_ERR_WORKSPACE;
    const int64_t wd = dmm_pack_words(HW);
    rc = dmm::match_front(dmm::packed_front(w, packed_p, (int64_t)N * wd, wd, packed_t, feat_p, feat_t, B, N, M, HW, D, n_valid,
                                            m_valid), (hipStream_t)stream);
    if (rc != DMM_OK) return rc;
    return dmm::relax_match_launch({w.cosv, w.inter, w.area_p, w.area_t, score_p, B, N, M, n_valid, m_valid}, score_weight,
                                   {max_iter, proj_iter, lr}, is_test,
                                   {dmm::or_ws(sim_out, w.sim), R_out, Rb_out, match_score, det_score, iters_out, nullptr}, 0,
                                   nullptr, stream);
}

// (5c') the same with the Hungarian solver (algo 'hun')
extern "C" int dmm_match_solve_packed_hun(const uint64_t *packed_p, const uint64_t *packed_t, const float *feat_p,
                                          const float *feat_t, const float *score_p, int B, int N, int M, int HW, int D,
                                          const int32_t *n_valid, const int32_t *m_valid, float score_weight, int is_test,
                                          float *Rb_out, float *match_score, float *det_score, float *sim_out,
                                          float *R_out, int32_t *status, void *workspace, size_t workspace_bytes,
                                          dmm_stream_t stream) {
    (void)is_test;                                               // a one-hot row keeps its one under both logic rules
    if (B > 0 && M == 0 && N >= 0 && HW >= 0 && D >= 0) return dmm::lsap_zero_status(status, B, stream);
    bool go;
    int rc = dmm::one_call_check(B, N, M, HW, D, packed_p && packed_t && feat_p && feat_t && score_p && Rb_out &&
                                 match_score && det_score && status && workspace, &go);
    if (!go) return rc;
    if (!dmm::in_fast_envelope(N, M)) return DMM_ERR_UNSUPPORTED;
    const dmm::Workspace w = dmm::carve(workspace, B, N, M, D);
    if (workspace_bytes < w.bytes) return DMM_ERR_WORKSPACE;
    const int64_t wd = dmm_pack_words(HW);
    rc = dmm::match_front(dmm::packed_front(w, packed_p, (int64_t)N * wd, wd, packed_t, feat_p, feat_t, B, N, M, HW, D, n_valid,
                                            m_valid), (hipStream_t)stream);
    if (rc != DMM_OK) return rc;
    return dmm::hungarian_match_launch({w.cosv, w.inter, w.area_p, w.area_t, score_p, B, N, M, n_valid, m_valid}, score_weight,
                                       {dmm::or_ws(sim_out, w.sim), R_out, Rb_out, match_score, det_score, nullptr, nullptr},
                                       status, stream);
}
