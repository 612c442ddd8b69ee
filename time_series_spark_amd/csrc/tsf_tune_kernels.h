// tsf_tune_kernels.h -- the device side of tsf_tune (include/tsf.h) beyond the cross-validation kernels it shares with
// tsf_cross_validate (tsf_cv_kernels.h): one candidate's metric put into its column of the score matrix, the choice
// per series, and the gather of an aligned refit group.  Non-template __global__ functions: include from exactly one
// translation unit (tsf_api.hip).
#pragma once
#include "tsf_cv_kernels.h"

namespace tsf {

// Column c of score / cand_status [N][C] from one candidate's cv_metrics_kernel run with w = n rows: series n's single
// metric row (metric = the chosen one of that run's mse / rmse / mae / mape arrays) or NaN where it has none (a plan
// status), and the run's series status (the plan's, or TSF_CV_FIT_FAILED).  One thread per series.
__global__ __launch_bounds__(256) void tune_score_kernel(int64_t N, int32_t C, int32_t c, const double *__restrict__ metric,
                                                         const int64_t *__restrict__ m_off,
                                                         const int32_t *__restrict__ run_status,
                                                         double *__restrict__ score, int32_t *__restrict__ cand_status)
{
    const int64_t n = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (n >= N) return;
    const int64_t m0 = m_off[n];
    score[(size_t)n * C + c] = m_off[n + 1] > m0 ? metric[m0] : __builtin_nan("");
    cand_status[(size_t)n * C + c] = run_status[n];
}

constexpr int TUNE_SELECT_WAVES = 4;    // series per workgroup

// The choice rule (include/tsf.h): best[n] = the lowest c among the candidates with a finite score that attain the
// minimum; plan status kept (best -1); no finite score: TSF_TUNE_NO_SCORE (best -1).  One wave per series, lanes over
// the candidates: each lane keeps its first minimum over c = lane, lane + 64, ..., then a butterfly over (score, c)
// pairs ordered by score, then index -- the same pair wins whatever the order of the combines.
__global__ __launch_bounds__(TUNE_SELECT_WAVES * 64) void tune_select_kernel(int64_t N, int32_t C,
                                                                             const double *__restrict__ score,
                                                                             const int32_t *__restrict__ plan_status,
                                                                             int32_t *__restrict__ best,
                                                                             int32_t *__restrict__ series_status)
{
    const int wid = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6), lane = (int)threadIdx.x & 63;
    const int64_t n = (int64_t)blockIdx.x * TUNE_SELECT_WAVES + wid;
    if (n >= N) return;
    const double *row = score + (size_t)n * C;
    double v = __builtin_huge_val();
    int32_t k = C;                                  // C: no finite score seen
    for (int32_t c = lane; c < C; c += 64) {
        const double s = row[c];
        if (__builtin_isfinite(s) && (k == C || s < v)) { v = s; k = c; }
    }
    for (int d = 32; d >= 1; d >>= 1) {
        const double ov = __shfl_xor(v, d, 64);
        const int32_t ok = __shfl_xor(k, d, 64);
        if (ok < C && (k == C || ov < v || (ov == v && ok < k))) { v = ov; k = ok; }
    }
    if (lane == 0) {
        const int32_t p = plan_status[n];
        const int32_t st = p != TSF_CV_OK ? p : (k < C ? TSF_CV_OK : TSF_TUNE_NO_SCORE);
        series_status[n] = st;
        best[n] = st == TSF_CV_OK ? k : -1;
    }
}

// The rows of the series sel[0 .. G) of an aligned panel as a [G][T] panel (y in the caller's dtype), with their floor
// / cap: one aligned refit group.  One workgroup per series.
__global__ __launch_bounds__(256) void tune_gather_kernel(CvPanel p, int64_t G, const int32_t *__restrict__ sel,
                                                          const double *__restrict__ floor_, const double *__restrict__ cap,
                                                          void *__restrict__ dst_y, double *__restrict__ dst_floor,
                                                          double *__restrict__ dst_cap)
{
    for (int64_t g = blockIdx.x; g < G; g += gridDim.x) {
        const int64_t n = sel[g];
        const int64_t s0 = n * p.T, d0 = g * p.T;
        for (int64_t i = threadIdx.x; i < p.T; i += blockDim.x) {
            if (p.ysz == 8) ((uint64_t *)dst_y)[d0 + i] = ((const uint64_t *)p.y)[s0 + i];
            else ((uint32_t *)dst_y)[d0 + i] = ((const uint32_t *)p.y)[s0 + i];
        }
        if (threadIdx.x == 0) {
            if (floor_) dst_floor[g] = floor_[n];
            if (cap) dst_cap[g] = cap[n];
        }
    }
}

// Fit outputs of an aligned refit group (series sel[0 .. G), in launch order) to their series' positions; the group's
// one grid (every aligned group of a call builds the same one: same timestamps, same changepoint settings) to dst.grid[0].
// One wave per series.
__global__ __launch_bounds__(64) void tune_scatter_kernel(int64_t G, const int32_t *__restrict__ sel, int stride,
                                                          tsf_fit_out src, tsf_fit_out dst)
{
    const int64_t g = blockIdx.x;
    if (g >= G) return;
    const int64_t n = sel[g];
    for (int k = threadIdx.x; k < stride; k += 64) dst.theta[(size_t)n * stride + k] = src.theta[(size_t)g * stride + k];
    constexpr int GW = (int)(sizeof(tsf_grid_info) / 8);
    if (g == 0)
        for (int k = threadIdx.x; k < GW; k += 64) ((uint64_t *)dst.grid)[k] = ((const uint64_t *)src.grid)[k];
    if (threadIdx.x == 0) {
        dst.y_scale[n] = src.y_scale[g]; dst.fval[n] = src.fval[g]; dst.status[n] = src.status[g];
        dst.n_iter[n] = src.n_iter[g]; dst.n_eval[n] = src.n_eval[g];
    }
}

}  // namespace tsf
