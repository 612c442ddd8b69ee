// tsf_select_kernels.h -- the device side of tsf_select (include/tsf.h) beyond what it shares with tsf_tune
// (tsf_tune_kernels.h) and tsf_cross_validate (tsf_cv_kernels.h): the choice within a tolerance of the best score, and
// the scatter of a refit group's outputs from its candidate's theta stride into rows padded to the widest candidate's.
// Non-template __global__ functions: include from exactly one translation unit (tsf_api.hip).
#pragma once
#include "tsf_tune_kernels.h"

namespace tsf {

// The choice rule (include/tsf.h): m = the least finite score of the row; best[n] = the lowest c with a finite score
// <= m * (1.0 + tolerance); chosen[n] = best[n], or fallback where the series has no choice.  Statuses as
// tune_select_kernel's.  One wave per series, lanes over the candidates: each lane keeps the minimum over c = lane,
// lane + 64, ..., a min butterfly gives every lane m; each lane then keeps its first c under the threshold, and a
// second min butterfly over the indices gives the lowest.  The threshold is one rounded add and one rounded multiply
// (__dadd_rn / __dmul_rn: nothing for the compiler to contract), so tolerance = 0 compares against m itself and the
// rule is tune_select_kernel's first minimum.
__global__ __launch_bounds__(TUNE_SELECT_WAVES * 64) void select_choose_kernel(int64_t N, int32_t C, double tolerance,
                                                                               int32_t fallback,
                                                                               const double *__restrict__ score,
                                                                               const int32_t *__restrict__ plan_status,
                                                                               int32_t *__restrict__ best,
                                                                               int32_t *__restrict__ chosen,
                                                                               int32_t *__restrict__ series_status)
{
    const int wid = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6), lane = (int)threadIdx.x & 63;
    const int64_t n = (int64_t)blockIdx.x * TUNE_SELECT_WAVES + wid;
    if (n >= N) return;
    const double *row = score + (size_t)n * C;
    double m = __builtin_huge_val();                // (+inf: no finite score seen)
    for (int32_t c = lane; c < C; c += 64) {
        const double s = row[c];
        if (__builtin_isfinite(s) && s < m) m = s;
    }
    for (int d = 32; d >= 1; d >>= 1) {
        const double om = __shfl_xor(m, d, 64);
        if (om < m) m = om;
    }
    const double thr = __dmul_rn(m, __dadd_rn(1.0, tolerance));
    int32_t k = C;                                  // C: no candidate under the threshold
    if (__builtin_isfinite(m))
        for (int32_t c = lane; c < C; c += 64) {
            const double s = row[c];
            if (__builtin_isfinite(s) && s <= thr) { k = c; break; }
        }
    for (int d = 32; d >= 1; d >>= 1) {
        const int32_t ok = __shfl_xor(k, d, 64);
        if (ok < k) k = ok;
    }
    if (lane == 0) {
        const int32_t p = plan_status[n];
        const int32_t st = p != TSF_CV_OK ? p : (k < C ? TSF_CV_OK : TSF_TUNE_NO_SCORE);
        const int32_t b = st == TSF_CV_OK ? k : -1;
        series_status[n] = st;
        best[n] = b;
        chosen[n] = b >= 0 ? b : fallback;
    }
}

// The outputs of one candidate's refit group to the call's padded outputs.  src: the group's fits at their series'
// positions, theta rows of `stride` doubles (the candidate's); dst: theta rows of `stride_max` doubles, the first
// `stride` the fit's, the rest +0.0.  The grids: aligned panel (grid_c >= 0), the group's one grid src.grid[0] to
// dst.grid[grid_c]; ragged (grid_c < 0), src.grid[n] to dst.grid[n].  One wave per member sel[g].
__global__ __launch_bounds__(64) void select_scatter_kernel(int64_t G, const int32_t *__restrict__ sel, int stride,
                                                            int stride_max, int32_t grid_c, tsf_fit_out src, tsf_fit_out dst)
{
    const int64_t g = blockIdx.x;
    if (g >= G) return;
    const int64_t n = sel[g];
    for (int k = threadIdx.x; k < stride_max; k += 64)
        dst.theta[(size_t)n * stride_max + k] = k < stride ? src.theta[(size_t)n * stride + k] : 0.0;
    constexpr int GW = (int)(sizeof(tsf_grid_info) / 8);
    if (grid_c < 0) {
        for (int k = threadIdx.x; k < GW; k += 64) ((uint64_t *)(dst.grid + n))[k] = ((const uint64_t *)(src.grid + n))[k];
    } else if (g == 0) {
        for (int k = threadIdx.x; k < GW; k += 64) ((uint64_t *)(dst.grid + grid_c))[k] = ((const uint64_t *)src.grid)[k];
    }
    if (threadIdx.x == 0) {
        dst.y_scale[n] = src.y_scale[n]; dst.fval[n] = src.fval[n]; dst.status[n] = src.status[n];
        dst.n_iter[n] = src.n_iter[n]; dst.n_eval[n] = src.n_eval[n];
    }
}

}  // namespace tsf
