// dmm_lsap.hip -- exact rectangular linear sum assignment on gfx950: the 'hun' solver slot
// (dmm/modules/match_model.py:122-123 -> scipy.optimize.linear_sum_assignment in the reference).
//
// scipy's solver is Crouse's shortest augmenting path (rectangular_lsap.cpp) in fp64; this is the same algorithm on the
// float32 costs converted to double exactly, and it picks the same assignment on every input, ties included.  Per row
// curRow it grows a shortest-path tree from curRow until it reaches an unassigned column, then updates the duals u / v
// and augments along `path`.  The one sequential piece of scipy's loop is the column choice: a scan over `remaining`
// (a list that starts as nc-1 .. 0 and loses a picked column by `remaining[index] = remaining[--num]`) with the rule
// `spc[j] < lowest || (spc[j] == lowest && row4col[j] == -1)`.  Every column here keeps its POSITION in that list, and
// the scan becomes an order-free reduction: the smallest spc wins; at equal spc an unassigned column beats an assigned
// one; among unassigned columns the largest position wins, among assigned ones the smallest (tests/lsap_model.py restates
// this in NumPy and pins it against scipy).
//
// Mapping: one wave64 per frame.  Lane l owns columns l, l+64, l+128, l+192 (nc <= 256) -- their v, shortest-path cost,
// path, row4col and position -- and row l (nr <= 32): its u, col4row and SR bit.  The frame's live cost block is staged
// once in LDS (<= 32 x 256 floats = 32 KiB; the launch sizes it to the table, so small frames share a CU widely).  Each
// step is two wave reductions with __shfl_xor (the fp64 minimum, then a 32-bit (rank, column) maximum) and a few
// broadcasts; no atomics, one workgroup = one wave, so the result is the same on every run.  Invalid tables follow scipy: a NaN or -inf entry -> status 1 ("invalid numeric entries"), no complete
// assignment -> status 2 ("cost matrix is infeasible"); such a frame's outputs are zero (col4row -1).
#include "dmm_solve_core.h"

namespace dmm {

constexpr int kLsapSlots = DMM_MAX_PROPOSALS / 64;
constexpr int kLsapOk = 0, kLsapInvalid = 1, kLsapInfeasible = 2;

__device__ __forceinline__ double wave_min_f64(double x) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const double y = __shfl_xor(x, o, 64);
        x = y < x ? y : x;
    }
    return x;
}

__device__ __forceinline__ int wave_max_i32(int x) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const int y = __shfl_xor(x, o, 64);
        x = y > x ? y : x;
    }
    return x;
}

// value of slot s (a wave-uniform index) of lane `src`
template <typename T>
__device__ __forceinline__ T from_slot(const T (&a)[kLsapSlots], int s, int src) {
    T x = a[0];
#pragma unroll
    for (int k = 1; k < kLsapSlots; ++k)
        if (s == k) x = a[k];
    return __shfl(x, src, 64);
}

// Solves the nr x nc table cs[i * nc + j] (LDS, nr <= nc <= DMM_MAX_PROPOSALS, nr <= 32).  Returns the status; on
// kLsapOk lane r < nr holds col4row[r] in `c4r`.
__device__ int lsap_wave(const float *cs, int nr, int nc, int &c4r) {
    const int lane = threadIdx.x;
    c4r = -1;
    {
        bool bad = false;
        for (int k = lane; k < nr * nc; k += 64) {
            const float c = cs[k];
            bad |= (c != c) || c == -__builtin_inff();
        }
        if (__any(bad)) return kLsapInvalid;
    }
    const double INF = __builtin_inf();
    double u = 0.0;                                              // row `lane`
    double v[kLsapSlots], spc[kLsapSlots];                       // column lane + 64 s
    int path[kLsapSlots], r4c[kLsapSlots], pos[kLsapSlots];
#pragma unroll
    for (int s = 0; s < kLsapSlots; ++s) {
        v[s] = 0.0;
        path[s] = -1;
        r4c[s] = -1;
    }
    for (int cur = 0; cur < nr; ++cur) {
#pragma unroll
        for (int s = 0; s < kLsapSlots; ++s) {
            const int j = lane + 64 * s;
            pos[s] = j < nc ? nc - 1 - j : -1;                   // remaining[it] = nc-1-it
            spc[s] = INF;
        }
        bool sr = false;
        double min_val = 0.0;
        int i = cur, num = nc, sink = -1;
        while (sink < 0) {
            if (lane == i) sr = true;
            const double ui = __shfl(u, i, 64);
            const float *ci = cs + i * nc;
            double low = INF;
#pragma unroll
            for (int s = 0; s < kLsapSlots; ++s) {
                if (pos[s] >= 0) {
                    const double r = ((min_val + (double)ci[lane + 64 * s]) - ui) - v[s];
                    if (r < spc[s]) {
                        path[s] = i;
                        spc[s] = r;
                    }
                    low = spc[s] < low ? spc[s] : low;
                }
            }
            const double lowest = wave_min_f64(low);
            if (!(lowest < INF)) return kLsapInfeasible;
            // scan rule as a rank: unassigned 512 + pos (largest first), assigned 511 - pos (smallest first)
            int key = -1;
#pragma unroll
            for (int s = 0; s < kLsapSlots; ++s) {
                if (pos[s] >= 0 && spc[s] == lowest) {
                    const int rk = r4c[s] < 0 ? 512 + pos[s] : 511 - pos[s];
                    const int kk = (rk << 9) | (lane + 64 * s);
                    key = kk > key ? kk : key;
                }
            }
            key = wave_max_i32(key);
            const int jw = key & 511, rk = key >> 9;
            const int pw = rk >= 512 ? rk - 512 : 511 - rk;
            const int sw = jw >> 6, lw = jw & 63;
            min_val = from_slot(spc, sw, lw);                    // scipy: minVal = lowest = spc[winner]
            const int row_of = from_slot(r4c, sw, lw);
            --num;
#pragma unroll
            for (int s = 0; s < kLsapSlots; ++s) {
                if (pos[s] == num) pos[s] = pw;                  // remaining[index] = remaining[--num]
                if (lane + 64 * s == jw) pos[s] = -1;            // SC[jw]
            }
            if (row_of < 0) sink = jw;
            else i = row_of;
        }
        // duals: u[cur] += minVal; u[i] += minVal - spc[col4row[i]] (SR rows but cur); v[j] -= minVal - spc[j] (SC)
        {
            const int c = c4r < 0 ? 0 : c4r;
            double sc = 0.0;
#pragma unroll
            for (int s = 0; s < kLsapSlots; ++s) {
                const double t = __shfl(spc[s], c & 63, 64);
                if ((c >> 6) == s) sc = t;
            }
            if (lane == cur) u += min_val;
            else if (sr && lane < nr) u += min_val - sc;
        }
#pragma unroll
        for (int s = 0; s < kLsapSlots; ++s)
            if (lane + 64 * s < nc && pos[s] < 0) v[s] -= min_val - spc[s];
        // augment along path
        int j = sink;
        while (true) {
            const int sj = j >> 6, lj = j & 63;
            const int ip = from_slot(path, sj, lj);
#pragma unroll
            for (int s = 0; s < kLsapSlots; ++s)
                if (lane + 64 * s == j) r4c[s] = ip;
            const int old = __shfl(c4r, ip, 64);
            if (lane == ip) c4r = j;
            j = old;
            if (ip == cur) break;
        }
    }
    return kLsapOk;
}

// Stages the frame's live rv x cv block (entry (i, j) = get(i, j), called once each) in LDS and solves it; rv > cv solves
// the transpose, as scipy does.  Returns the status; lane r < rv gets the column of row r (-1 for an unassigned row).
template <typename GET>
__device__ __forceinline__ int lsap_frame(float *cs, int rv, int cv, GET get, int &col_of_row) {
    const int lane = threadIdx.x;
    const bool tr = rv > cv;
    const int nr = tr ? cv : rv, nc = tr ? rv : cv;
    for (int k = lane; k < rv * cv; k += 64) {
        const int i = k / cv, j = k - i * cv;
        cs[tr ? j * rv + i : k] = get(i, j);
    }
    __syncthreads();                                             // one wave: orders the staging stores before the reads
    int c4r;
    const int st = lsap_wave(cs, nr, nc, c4r);
    col_of_row = -1;
    if (st != kLsapOk) return st;
    if (!tr) {
        col_of_row = lane < rv ? c4r : -1;
    } else {
        for (int k = 0; k < cv; ++k) {                           // row c4r_T[k] of the original table takes column k
            const int t = __shfl(c4r, k, 64);
            if (lane == t) col_of_row = k;
        }
    }
    return st;
}

__global__ __launch_bounds__(64) void lsap_kernel(const float *__restrict__ C, int nr, int nc,
                                                  const int32_t *__restrict__ rows_valid,
                                                  const int32_t *__restrict__ cols_valid, float *__restrict__ X,
                                                  int32_t *__restrict__ col4row, int32_t *__restrict__ status) {
    extern __shared__ float cs[];                                // the staged cost block (sized by the launch)
    const int b = blockIdx.x, lane = threadIdx.x;
    int rv = rows_valid ? rows_valid[b] : nr, cv = cols_valid ? cols_valid[b] : nc;
    rv = rv < 0 ? 0 : (rv > nr ? nr : rv);
    cv = cv < 0 ? 0 : (cv > nc ? nc : cv);
    const float *Cb = C + (int64_t)b * nr * nc;
    int cr = -1, st = kLsapOk;
    if (rv > 0 && cv > 0) st = lsap_frame(cs, rv, cv, [&](int i, int j) { return Cb[(int64_t)i * nc + j]; }, cr);
    if (col4row && lane < nr) col4row[(int64_t)b * nr + lane] = cr;
    if (status && lane == 0) status[b] = st;
    if (X) {
        float *Xb = X + (int64_t)b * nr * nc;
        for (int r = 0; r < nr; ++r) {
            const int c = __shfl(cr, r, 64);
            for (int j = lane; j < nc; j += 64) Xb[(int64_t)r * nc + j] = j == c ? 1.0f : 0.0f;
        }
    }
}

// The layer with the Hungarian solver (match_model.py:89-130 with algo 'hun', :146-147): sim from the counts exactly as
// the relaxed solver's prologue computes it (mix_sim), C = -sim padded with -0.0 to the frame's live width
// Pp = max(Nb, Mb + 1), the assignment, R = Rb = its one-hot (every live row is assigned: Mb < Pp, so both logic rules
// keep exactly the one), match_score = max_p clamp(R,0,1)*sim_pad, det_score = sum_p score_p*Rb = the score of the
// assigned proposal (0 for a padded column).
__global__ __launch_bounds__(64) void hungarian_match_kernel(
    const float *__restrict__ cos_in, const int32_t *__restrict__ inter, const int32_t *__restrict__ area_p,
    const int32_t *__restrict__ area_t, const float *__restrict__ score_p, int N, int M,
    const int32_t *__restrict__ n_valid, const int32_t *__restrict__ m_valid, float w_feat, float w_iou,
    float *__restrict__ sim_out, float *__restrict__ R_out, float *__restrict__ Rb_out, float *__restrict__ match_score,
    float *__restrict__ det_score, int32_t *__restrict__ status) {
    extern __shared__ float cs[];                                // the staged cost block (sized by the launch)
    const int b = blockIdx.x, lane = threadIdx.x;
    const int PpS = N > M ? N : M + 1;                           // table stride
    int Nb = n_valid ? n_valid[b] : N, Mb = m_valid ? m_valid[b] : M;
    Nb = Nb < 0 ? 0 : (Nb > N ? N : Nb);
    Mb = Mb < 0 ? 0 : (Mb > M ? M : Mb);
    const bool live = Nb > 0 && Mb > 0;                          // dead frame: zeros (dmm_model.py:118-122)
    const int Pp = Nb > Mb ? Nb : Mb + 1;
    const float *cos_b = cos_in + (int64_t)b * M * N;
    const int32_t *inter_b = inter + (int64_t)b * M * N;
    float *sim_b = sim_out + (int64_t)b * M * N;
    for (int k = lane; k < M * N; k += 64) {                     // sim outside the live block: zeros
        const int i = k / N, p = k - i * N;
        if (!(live && i < Mb && p < Nb)) sim_b[k] = 0.0f;
    }
    int cr = -1, st = kLsapOk;
    if (live) {
        // staged as C = -sim_pad (padded columns -0.0), sim stored on the way
        st = lsap_frame(cs, Mb, Pp, [&](int i, int p) {
            if (p >= Nb) return -0.0f;
            const int64_t k = (int64_t)i * N + p;
            const float s = mix_sim(cos_b[k], inter_b[k], area_p[(int64_t)b * N + p], area_t[(int64_t)b * M + i], w_feat,
                                    w_iou);
            sim_b[k] = s;
            return -s;
        }, cr);
    }
    if (status && lane == 0) status[b] = st;
    float *Rb_b = Rb_out + (int64_t)b * M * PpS;
    float *R_b = R_out ? R_out + (int64_t)b * M * PpS : nullptr;
    for (int r = 0; r < M; ++r) {
        const int c = __shfl(cr, r, 64);
        const bool row_live = st == kLsapOk && live && r < Mb;  // (only a live row's cost block was staged)
        float ms = -__builtin_inff();
        for (int p = lane; p < PpS; p += 64) {
            const float x = p == c ? 1.0f : 0.0f;
            Rb_b[(int64_t)r * PpS + p] = x;
            if (R_b) R_b[(int64_t)r * PpS + p] = x;
            if (row_live && p < Pp) {
                const float m = x * -cs[r * Pp + p];             // sim_pad (+0 in the padded columns)
                ms = m > ms ? m : ms;
            }
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const float y = __shfl_xor(ms, o, 64);
            ms = y > ms ? y : ms;
        }
        if (lane == 0) {
            match_score[(int64_t)b * M + r] = row_live ? ms : 0.0f;
            det_score[(int64_t)b * M + r] = (row_live && c < Nb) ? score_p[(int64_t)b * N + c] : 0.0f;
        }
    }
}

__global__ __launch_bounds__(64) void lsap_zero_status_kernel(int32_t *__restrict__ status, int B) {
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (i < B) status[i] = 0;
}

// status [B] = 0 (kLsapOk) for a call with nothing to solve (M == 0): the caller reads it like any other
int lsap_zero_status(int32_t *status, int B, dmm_stream_t stream) {
    if (!status) return DMM_ERR_BAD_ARG;
    hipLaunchKernelGGL(lsap_zero_status_kernel, dim3((B + 63) / 64), dim3(64), 0, (hipStream_t)stream, status, B);
    return check_launch();
}

}  // namespace dmm

extern "C" int dmm_lsap_f32(const float *C, int B, int nr, int nc, const int32_t *rows_valid, const int32_t *cols_valid,
                            float *X, int32_t *col4row, int32_t *status, dmm_stream_t stream) {
    if (B < 0 || nr < 0 || nc < 0) return DMM_ERR_BAD_ARG;
    if (B == 0) return DMM_OK;
    if (!status || (!C && nr > 0 && nc > 0)) return DMM_ERR_BAD_ARG;
    if (nr > DMM_MAX_TEMPLATES || nc > DMM_MAX_PROPOSALS || nr > nc) return DMM_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(dmm::lsap_kernel, dim3(B), dim3(64), (size_t)nr * nc * sizeof(float), (hipStream_t)stream, C, nr,
                       nc, rows_valid, cols_valid, X, col4row, status);
    return dmm::check_launch();
}

// dmm_hungarian_match_f32 proper (a one-hot row keeps its one under both logic rules: no is_test)
int dmm::hungarian_match_launch(const SolveIn &in, float score_weight, const SolveOut &out, int32_t *status,
                                dmm_stream_t stream) {
    if (in.B > 0 && in.N >= 0 && in.M == 0) return lsap_zero_status(status, in.B, stream);
    int is_test = 0;
    bool go;
    const int rc = solve_entry_check(in, out, 0, 0, false, &is_test, &go);
    if (!go) return rc;
    if (!status) return DMM_ERR_BAD_ARG;
    if (!in_fast_envelope(in.N, in.M)) return DMM_ERR_UNSUPPORTED;
    float w_feat, w_iou;
    sim_weights(score_weight, w_feat, w_iou);
    hipLaunchKernelGGL(hungarian_match_kernel, dim3(in.B), dim3(64), (size_t)in.M * padded_width(in.N, in.M) * sizeof(float),
                       (hipStream_t)stream, in.cos, in.inter, in.area_p, in.area_t, in.score_p, in.N, in.M, in.n_valid,
                       in.m_valid, w_feat, w_iou, out.sim, out.R, out.Rb, out.match_score, out.det_score, status);
    return check_launch();
}

extern "C" int dmm_hungarian_match_f32(const float *cos_in, const int32_t *inter, const int32_t *area_p,
                                       const int32_t *area_t, const float *score_p, int B, int N, int M,
                                       const int32_t *n_valid, const int32_t *m_valid, float score_weight, int is_test,
                                       float *sim_out, float *R_out, float *Rb_out, float *match_score,
                                       float *det_score, int32_t *status, dmm_stream_t stream) {
    (void)is_test;
    return dmm::hungarian_match_launch({cos_in, inter, area_p, area_t, score_p, B, N, M, n_valid, m_valid}, score_weight,
                                       {sim_out, R_out, Rb_out, match_score, det_score, nullptr, nullptr}, status, stream);
}
