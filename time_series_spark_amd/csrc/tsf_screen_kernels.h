// tsf_screen_kernels.h -- outlier screening (include/tsf.h, "outlier screening"): tsf_screen_rows and the device side of
// tsf_fit_screened beyond the fit, predict and cross-validation kernels it shares.
//   screen_rows_kernel     one workgroup per series: the rule of include/tsf.h on (y, fitted, excluded).  Two bitonic
//                          sorts in ONE dynamic-LDS array of NSP doubles (NSP = the launch's row count rounded up to a
//                          power of two; padding and excluded rows enter as +inf): the residuals for the median, then --
//                          the residuals formed again from global memory, same operands, same bits -- the absolute
//                          deviations for the MAD and the budget's order statistic
//   screen_compact_kernel  cv_expand_kernel's cousin: the rows of the listed series that carry no flag, in row order, as
//                          one ragged panel at given offsets (a workgroup prefix scan over the keep bits: ballot counts
//                          per wave, the wave totals in LDS; no atomics)
//   screen_history_kernel  a ragged panel's own dates as the padded future panel [N][Tmax] predict_kernel reads
//   small ones             the scale floor per series, NaN over the fitted rows of a failed fit, one grid copied to N
// Exchanges move values and round nothing, so center, scale and the cut are functions of a series' multiset of
// residuals alone: neither the launch's NSP nor the rest of the batch can show.
// Non-template __global__ functions: include from exactly one translation unit (tsf_api.hip).
#pragma once
#include "tsf_cv_kernels.h"

namespace tsf {

struct ScreenArgs {
    const void *y;              // the caller's y, y_dtype: [N][T] aligned, [offsets[N]] ragged
    const double *fitted;       // y's layout (fit_ld == 0), or series n at n * fit_ld (tsf_fit_screened's padded predict)
    const uint8_t *excluded;    // y's layout, or nullptr
    const double *min_scale;    // [N] or nullptr (0)
    const int64_t *offsets;     // [N+1] ragged, nullptr aligned
    const int32_t *sel;         // the series of this launch (block b works on sel[b]), or nullptr (block b on series b)
    int64_t T, fit_ld;
    int y_dtype;
    int32_t min_rows;
    double threshold, max_share;
    uint8_t *flag;              // y's layout
    double *resid;              // y's layout, or nullptr
    double *center, *scale;     // [N] or nullptr
    int32_t *n_new, *n_flagged; // [N] or nullptr
    int32_t *status;            // [N]
};

constexpr size_t SCREEN_PART_BYTES = 16 * sizeof(int);

// sum over the workgroup's threads (any block size up to 1024 threads of whole waves); s: 16 ints of LDS; ends behind a
// barrier, and begins with one, so s may be used again at once
__device__ __forceinline__ int screen_block_sum(int v, int *s)
{
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d, 64);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) s[threadIdx.x >> 6] = v;
    __syncthreads();
    int t = 0;
    for (int w = 0; w < (int)(blockDim.x >> 6); ++w) t += s[w];
    return t;
}

// iv_load_sort's network (tsf_interval_kernels.h) over values already in LDS: begins and ends behind a barrier
__device__ __forceinline__ void screen_sort(double *v, int NSP)
{
    __syncthreads();
    for (int k = 2; k <= NSP; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int i = threadIdx.x; i < NSP; i += blockDim.x) {
                const int ixj = i ^ j;
                if (ixj > i) {
                    const bool asc = (i & k) == 0;
                    const double x = v[i], y = v[ixj];
                    if ((x > y) == asc) { v[i] = y; v[ixj] = x; }
                }
            }
            __syncthreads();
        }
}

__device__ __forceinline__ double screen_y(const ScreenArgs &a, int64_t i)
{
    if (a.y_dtype == TSF_Y_F64) return ((const double *)a.y)[i];
    if (a.y_dtype == TSF_Y_F32) return (double)((const float *)a.y)[i];
    return (double)((const int32_t *)a.y)[i];
}

// Every branch below the load is on values reduced over the workgroup, so every barrier is reached by all threads or
// by none.  A series longer than the launch's NSP (or than TSF_SCREEN_MAX_ROWS) never touches the sort array.
__global__ __launch_bounds__(256) void screen_rows_kernel(ScreenArgs a, int NSP)
{
    extern __shared__ __align__(16) unsigned char screen_smem[];      // NSP doubles, then SCREEN_PART_BYTES of wave sums
    double *v = reinterpret_cast<double *>(screen_smem);
    int *s_part = reinterpret_cast<int *>(screen_smem + sizeof(double) * (size_t)NSP);
    const int64_t n = a.sel ? a.sel[blockIdx.x] : (int64_t)blockIdx.x;
    const int64_t r0 = a.offsets ? a.offsets[n] : n * a.T;
    const int64_t m0 = a.offsets ? a.offsets[n + 1] - r0 : a.T;
    const double *fit = a.fit_ld > 0 ? a.fitted + (size_t)n * a.fit_ld : a.fitted + r0;
    const uint8_t *ex = a.excluded ? a.excluded + r0 : nullptr;
    const double NaN = __builtin_nan(""), inf = __builtin_huge_val();
    const bool too_long = m0 > (int64_t)TSF_SCREEN_MAX_ROWS || m0 > (int64_t)NSP;
    // residuals out, flag = excluded, the live rows into the sort array
    int live_n = 0, bad = 0;
    for (int64_t i = threadIdx.x; i < (too_long ? m0 : (int64_t)NSP); i += blockDim.x) {
        double r = inf;
        bool live = false;
        if (i < m0) {
            const uint8_t e = ex ? (uint8_t)(ex[i] != 0) : (uint8_t)0;
            r = screen_y(a, r0 + i) - fit[i];
            if (a.resid) a.resid[r0 + i] = r;
            a.flag[r0 + i] = e;
            live = e == 0;
            live_n += live ? 1 : 0;
            bad |= (live && !__builtin_isfinite(r)) ? 1 : 0;
        }
        if (!too_long) v[i] = live ? r : inf;
    }
    const int packed = screen_block_sum(live_n + (bad ? (1 << 20) : 0), s_part);     // (live_n <= 16384 per series)
    const int64_t m = packed & ((1 << 20) - 1), x = m0 - m;
    int st = TSF_SCREEN_OK;
    if (too_long) st = TSF_SCREEN_TOO_LONG;
    else if (m < (int64_t)a.min_rows) st = TSF_SCREEN_TOO_FEW;
    else if (packed >> 20) st = TSF_SCREEN_NONFINITE;
    if (st != TSF_SCREEN_OK) {
        if (threadIdx.x == 0) {
            a.status[n] = st;
            if (a.center) a.center[n] = NaN;
            if (a.scale) a.scale[n] = NaN;
            if (a.n_new) a.n_new[n] = 0;
            if (a.n_flagged) a.n_flagged[n] = (int32_t)x;
        }
        return;
    }
    screen_sort(v, NSP);
    const double center = 0.5 * (v[(m - 1) / 2] + v[m / 2]);
    __syncthreads();            // every thread has read the medians: the array is filled again
    for (int64_t i = threadIdx.x; i < (int64_t)NSP; i += blockDim.x) {
        double d = inf;
        if (i < m0 && !(ex && ex[i] != 0)) d = __builtin_fabs((screen_y(a, r0 + i) - fit[i]) - center);
        v[i] = d;
    }
    screen_sort(v, NSP);
    const double mad = 0.5 * (v[(m - 1) / 2] + v[m / 2]);
    const double scale = __builtin_fmax(1.4826 * mad, a.min_scale ? a.min_scale[n] : 0.0);
    const int64_t B = (int64_t)__builtin_floor(a.max_share * (double)m0) - x;
    int n_new = 0;
    if (B > 0) {
        const int64_t at = m - 1 - B;           // (>= 0 for max_share <= 0.5)
        const double cut = __builtin_fmax(a.threshold * scale, v[at > 0 ? at : 0]);
        for (int64_t i = threadIdx.x; i < m0; i += blockDim.x) {
            if (ex && ex[i] != 0) continue;
            const double d = __builtin_fabs((screen_y(a, r0 + i) - fit[i]) - center);
            if (d > cut) { a.flag[r0 + i] = 1; ++n_new; }
        }
    }
    n_new = screen_block_sum(n_new, s_part);
    if (threadIdx.x == 0) {
        a.status[n] = TSF_SCREEN_OK;
        if (a.center) a.center[n] = center;
        if (a.scale) a.scale[n] = scale;
        if (a.n_new) a.n_new[n] = n_new;
        if (a.n_flagged) a.n_flagged[n] = (int32_t)x + n_new;
    }
}

// The rows without a flag of the series sel[0 .. G) as one ragged panel: series sel[g]'s kept rows, in row order, at
// rows [dst_off[g], dst_off[g + 1]) of dst_ds / dst_y (the caller's dtype, bit-copied) / dst_extra ([n_extra][dst_total]),
// its floor / cap at [g].  flag: y's layout.  dst_off comes from the flag counts (n_flagged) on the host; a row past the
// series' destination range (flags that changed since) is dropped, never written.  One workgroup of four waves per
// series, 256 rows per step: a kept row's position = the kept rows of earlier steps + of earlier waves + of earlier lanes.
__global__ __launch_bounds__(256) void screen_compact_kernel(CvPanel p, int64_t G, const int32_t *__restrict__ sel,
                                                             const uint8_t *__restrict__ flag,
                                                             const int64_t *__restrict__ dst_off, int64_t dst_total,
                                                             const double *__restrict__ floor_, const double *__restrict__ cap,
                                                             int64_t *__restrict__ dst_ds, void *__restrict__ dst_y,
                                                             double *__restrict__ dst_extra, double *__restrict__ dst_floor,
                                                             double *__restrict__ dst_cap)
{
    __shared__ int s_wave[4];
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    for (int64_t g = blockIdx.x; g < G; g += gridDim.x) {
        const int64_t n = sel[g];
        const int64_t r0 = cv_row0(p, n), s0 = cv_ds0(p, n), es = cv_ex_stride(p);
        const int64_t rows = p.src_off ? p.src_off[n + 1] - r0 : p.T;
        const int64_t d0 = dst_off[g], room = dst_off[g + 1] - d0;
        int64_t base = 0;
        for (int64_t b = 0; b < rows; b += 256) {
            const int64_t i = b + threadIdx.x;
            const bool keep = i < rows && flag[r0 + i] == 0;
            const unsigned long long mask = __ballot(keep);
            __syncthreads();            // (the previous step's reads of s_wave are done)
            if (lane == 0) s_wave[wid] = __popcll(mask);
            __syncthreads();
            int before = 0, all = 0;
            for (int w = 0; w < 4; ++w) { before += w < wid ? s_wave[w] : 0; all += s_wave[w]; }
            const int64_t q = base + before + __popcll(mask & ((1ull << lane) - 1ull));
            if (keep && q < room) {
                dst_ds[d0 + q] = p.ds[s0 + i];
                if (p.ysz == 8) ((uint64_t *)dst_y)[d0 + q] = ((const uint64_t *)p.y)[r0 + i];
                else ((uint32_t *)dst_y)[d0 + q] = ((const uint32_t *)p.y)[r0 + i];
                for (int e = 0; e < p.n_extra; ++e) dst_extra[(size_t)e * dst_total + d0 + q] = p.extra[(size_t)e * es + s0 + i];
            }
            base += all;
        }
        if (threadIdx.x == 0) {
            if (floor_) dst_floor[g] = floor_[n];
            if (cap) dst_cap[g] = cap[n];
        }
    }
}

// A ragged panel's own dates as a padded future panel [N][Tmax] (rows past a series' last repeat it, as
// cv_holdout_kernel pads; a series without rows gets date 0 and is never read back), extra_future [N][n_extra][Tmax].
__global__ __launch_bounds__(256) void screen_history_kernel(CvPanel p, int64_t N, int32_t Tmax,
                                                             int64_t *__restrict__ ds_fut, double *__restrict__ ex_fut)
{
    for (int64_t n = blockIdx.x; n < N; n += gridDim.x) {
        const int64_t s0 = p.src_off[n], len = p.src_off[n + 1] - s0, es = p.src_total;
        for (int i = threadIdx.x; i < Tmax; i += blockDim.x) {
            const int64_t r = s0 + (i < len ? i : len - 1);
            ds_fut[(size_t)n * Tmax + i] = len > 0 ? p.ds[r] : 0;
            for (int e = 0; e < p.n_extra; ++e) ex_fut[((size_t)n * p.n_extra + e) * Tmax + i] = len > 0 ? p.extra[(size_t)e * es + r] : 0.0;
        }
    }
}

// min_scale[n] = rel * y_scale[n] (one product)
__global__ __launch_bounds__(256) void screen_scale_floor_kernel(int64_t N, double rel, const double *__restrict__ y_scale,
                                                                 double *__restrict__ min_scale)
{
    const int64_t n = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (n < N) min_scale[n] = rel * y_scale[n];
}

// A failed fit has no fitted values: NaN over its ld rows of fitted [N][ld], so the rule reports TSF_SCREEN_NONFINITE
// (or TSF_SCREEN_TOO_FEW) and flags nothing.
__global__ __launch_bounds__(256) void screen_mask_failed_kernel(int64_t N, int64_t ld, const int32_t *__restrict__ fit_status,
                                                                 double *__restrict__ fitted)
{
    for (int64_t n = blockIdx.x; n < N; n += gridDim.x) {
        if (fit_status[n] >= 0) continue;
        for (int64_t i = threadIdx.x; i < ld; i += blockDim.x) fitted[(size_t)n * ld + i] = __builtin_nan("");
    }
}

// grid[0] copied to grid[1 .. N): an aligned first fit's one grid as the grid-per-series form of tsf_fit_screened's output
__global__ __launch_bounds__(256) void screen_grid_fill_kernel(int64_t N, tsf_grid_info *__restrict__ grid)
{
    constexpr int64_t GW = (int64_t)(sizeof(tsf_grid_info) / 8);
    const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= (N - 1) * GW) return;
    ((uint64_t *)(grid + 1))[k] = ((const uint64_t *)grid)[k % GW];
}

}  // namespace tsf
