// tsf_component_kernels.h -- the forecast's decomposition (fbprophet 0.5 Prophet.predict_seasonal_components):
// every component the caller names as a set of design columns, for every future row of every series.
//
// fbprophet forms component c as X[:, cols(c)] . beta[cols(c)] (times y_scale for additive components) from the
// binary matrix regressor_column_matrix builds; here a component is a 64-bit mask over the original design columns
// (K <= TSF_MAX_K = 64).  Order contract (include/tsf.h, tsf_predict_components): an fma chain over the set columns in
// ascending original column order from 0.0, then the product with y_scale where the component is scaled -- on the
// design values predict_kernel uses (the shared table Xf of future_design_kernel, or dm_sincos + fourier_harmonics per
// row, and the caller's extra columns).  The trend and yhat come from predict_kernel itself (PredictArgs::trend_out).
//
// component_kernel: one wavefront per series, lanes over the future rows (as predict_kernel); the component loop and
// the loop over a component's set columns are wave-uniform (the table lives in device memory: scalar loads).  Per-series
// futures compute each seasonality's base pair once per row, held in registers (an array indexed by seasonality
// only, every index a compile-time constant); no per-lane array is indexed by component.
// Non-template __global__ function: include from exactly one translation unit (tsf_api.hip).
#pragma once
#include "tsf_aux_kernels.h"

namespace tsf {

struct ComponentArgs {
    const DevSpec *sp;
    int64_t N;
    int H, theta_stride, shared_future, n_comp;
    const double *theta, *y_scale;
    const int64_t *ds_future;
    const double *extra_future;
    const double *Xf;                   // shared future grid: [K][H] design values (future_design_kernel), else null
    const uint64_t *cols;               // [n_comp] column masks, bit j = original design column j
    const int32_t *scaled;              // [n_comp] 1: times y_scale
    double *comp;                       // [N][n_comp][H]
};

constexpr int COMP_WAVES = 4;           // series per workgroup

__global__ __launch_bounds__(COMP_WAVES * 64) void component_kernel(ComponentArgs a)
{
    const int wid = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6), lane = (int)threadIdx.x & 63;
    const int64_t n = (int64_t)blockIdx.x * COMP_WAVES + wid;
    if (n >= a.N) return;
    const DevSpec *sp = a.sp;
    const int H = a.H, C = a.n_comp, nf = sp->K - sp->n_extra, n_seas = sp->n_seas;
    const double *beta = a.theta + (size_t)n * a.theta_stride + 3 + sp->n_cp;
    const double ys = a.y_scale[n];
    for (int h = lane; h < H; h += 64) {
        const int64_t gid = n * (int64_t)H + h;
        const double *xe = a.extra_future + (a.shared_future ? (size_t)h : (size_t)n * sp->n_extra * H + h);
        double s1[TSF_MAX_SEAS], c1[TSF_MAX_SEAS];
        if (!a.Xf) {
            const int64_t dsv = a.ds_future[gid];
#pragma unroll
            for (int se = 0; se < TSF_MAX_SEAS; ++se) {
                s1[se] = 0.0; c1[se] = 0.0;
                if (se < n_seas) dm_sincos(fourier_base_arg(dsv, sp->seas_period[se]), s1[se], c1[se]);
            }
        }
        double *out = a.comp + (size_t)n * C * H + h;
        for (int c = 0; c < C; ++c) {
            const uint64_t mask = a.cols[c];
            double acc = 0.0;
            if (a.Xf) {
                for (uint64_t m = mask; m; m &= m - 1) {
                    const int col = __builtin_ctzll(m);
                    const double xv = (col < nf) ? a.Xf[(size_t)col * H + h] : xe[(size_t)(col - nf) * H];
                    acc = __builtin_fma(xv, beta[col], acc);
                }
            } else {
#pragma unroll
                for (int se = 0; se < TSF_MAX_SEAS; ++se) {
                    if (se >= n_seas) break;
                    const int col0 = sp->seas_col[se], order = sp->seas_order[se];
                    const uint64_t span = (order >= 32) ? ~0ull : ((1ull << (2 * order)) - 1);
                    if (!((mask >> col0) & span)) continue;
                    fourier_harmonics(s1[se], c1[se], order, [&](int hh, double sv, double cv) {
                        const int col = col0 + 2 * (hh - 1);
                        if ((mask >> col) & 1) acc = __builtin_fma(sv, beta[col], acc);
                        if ((mask >> (col + 1)) & 1) acc = __builtin_fma(cv, beta[col + 1], acc);
                    });
                }
                for (uint64_t m = (nf >= 64) ? 0 : (mask >> nf); m; m &= m - 1) {
                    const int e = __builtin_ctzll(m);
                    acc = __builtin_fma(xe[(size_t)e * H], beta[nf + e], acc);
                }
            }
            if (a.scaled[c]) acc = acc * ys;
            out[(size_t)c * H] = acc;
        }
    }
}

}  // namespace tsf
