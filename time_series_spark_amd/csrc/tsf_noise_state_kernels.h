// tsf_noise_state_kernels.h -- the AR(1) noise state of a fitted panel in one pass, and the corrected point forecast
// (include/tsf.h, "the noise state of a fitted panel": tsf_noise_state, tsf_predict_conditioned).
//   noise_state_kernel       one wave per series, aligned or ragged.  Lane l takes rows l, l + 64, ... of its series (the
//                            mapping of ar_series_kernel and predict_kernel).  Per row: the fitted value by
//                            predict_kernel's per-series-date arithmetic (the trend segments from the one recurrence per
//                            series, parked in LDS; the Fourier columns in place from dm_sincos + fourier_harmonics; the
//                            explicit columns in the fit's own layout), r = (double)y - fitted, and r into
//                            ar_series_kernel's arithmetic (the left neighbour's residual by shuffle, a carry across
//                            64-row steps, 64 partials combined by corr_wave_sum).  Each lane keeps its highest present
//                            row; the wave's highest is ar_last_kernel's last present row.  No [rows] buffer of fitted
//                            values exists at any point: y, ds and the explicit columns are read once, nothing is written
//                            but the nine numbers per series.
//   conditioned_shift_kernel one thread per (series, row) behind predict_kernel: yhat + m_h for the series with phi != 0
//                            (ar_start_shift_kernel's recursion), then the reference's post-step on the corrected value.
// The row evaluation restates predict_kernel's rather than sharing a function with it: the build is -ffp-contract=off, so
// the same expressions give the same bits, and predict_kernel's code stays what it was.
// Non-template __global__ functions: include from exactly one translation unit (tsf_api.hip), behind tsf_aux_kernels.h
// and tsf_ar_kernels.h.
#pragma once
#include "tsf_common.h"
#include "tsf_aux_kernels.h"
#include "tsf_ar_kernels.h"

namespace tsf {

struct NoiseStateArgs {
    const DevSpec *sp;
    int64_t N;
    int32_t T, y_dtype, theta_stride, n_grids, min_pairs;
    double phi_max;
    const int64_t *offsets;     // [N + 1], or null = aligned
    const int64_t *ds;          // [T] aligned, [total_rows] ragged
    const void *y;              // [N][T] or [total_rows] in y_dtype
    const uint8_t *excluded;    // y's layout (1 = the row is absent), or null
    const double *floor_, *cap; // [N] or null
    const double *extra;        // [n_extra][extra_stride]: the fit's own layout
    int64_t extra_stride;       // T aligned, total_rows ragged
    const double *theta, *y_scale;
    const tsf_grid_info *grid;  // [n_grids]
    const int32_t *fit_status;  // [N]: a negative status has no fitted values
    double *phi, *phi_raw;      // [N] each; phi_raw, n_pairs, scale, last_ds_ns may be null
    int64_t *n_pairs;
    double *scale;
    int32_t *status;
    double *last_resid;
    int32_t *last_gap, *last_status;
    int64_t *last_ds_ns;
};

constexpr int NS_WAVES = 4;     // series per workgroup

__global__ __launch_bounds__(NS_WAVES * 64) void noise_state_kernel(NoiseStateArgs a, int ok_status, int no_pairs_status,
                                                                    int no_row_status)
{
    __shared__ double seg_ks[NS_WAVES][TSF_MAX_S + 4], seg_mc[NS_WAVES][TSF_MAX_S + 4];
    const int wid = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6), lane = (int)threadIdx.x & 63;
    const int64_t n = (int64_t)blockIdx.x * NS_WAVES + wid;
    if (n >= a.N) return;       // (a whole wave: no lane of it reaches a shuffle or the wave barrier)
    const DevSpec *sp = a.sp;
    const int64_t r0 = a.offsets ? a.offsets[n] : n * (int64_t)a.T;
    const int64_t len = a.offsets ? a.offsets[n + 1] - r0 : (int64_t)a.T;
    const int64_t d0 = a.offsets ? r0 : 0;              // the series' first row in ds and in the explicit columns
    const double NaN = __builtin_nan("");
    const bool fitted_ok = a.fit_status[n] >= 0;        // (wave-uniform)
    double ss = 0.0, C = 0.0;
    int64_t cnt = 0, np = 0;
    int64_t top_t = -1;         // this lane's highest present row
    double top_r = 0.0;
    if (fitted_ok) {
        const tsf_grid_info &gi = a.grid[a.n_grids == 1 ? 0 : n];
        const int S = gi.S, K = sp->K, Ka = sp->Ka, n_cp = sp->n_cp;
        const double *th = a.theta + (size_t)n * a.theta_stride;
        const double *delta = th + 3, *beta = th + 3 + n_cp;
        const double ys = a.y_scale[n];
        const double fl = (sp->growth == TSF_GROWTH_LOGISTIC && a.floor_) ? a.floor_[n] : 0.0;
        const double capsc = (sp->growth == TSF_GROWTH_LOGISTIC) ? (a.cap[n] - fl) / ys : 0.0;
        // slope / offset of every trend segment: predict_kernel's recurrence, once per series
        double dl[(TSF_MAX_S + W - 1) / W], tl[(TSF_MAX_S + W - 1) / W];
        {
            double ks = th[0], mc = th[1];
            if (lane == 0) { seg_ks[wid][0] = ks; seg_mc[wid][0] = mc; }
#pragma unroll
            for (int s = 0; s < (TSF_MAX_S + W - 1) / W; ++s) {
                const int c = lane + s * W;
                dl[s] = c < S ? delta[c] : 0.0;
                tl[s] = c < S ? gi.t_change[c] : 0.0;
            }
            for (int c = 0; c < S; ++c) {
                double dj = 0.0, tcj = 0.0;
#pragma unroll
                for (int s = 0; s < (TSF_MAX_S + W - 1) / W; ++s)
                    if ((c >> 6) == s) { dj = readlane_f64(dl[s], c & 63); tcj = readlane_f64(tl[s], c & 63); }
                const double ksn = ks + dj;
                if (sp->growth == TSF_GROWTH_LINEAR) {
                    mc = mc + ((-tcj) * dj);
                } else {
                    const double gamma = (tcj - mc) * (1.0 - ks / ksn);
                    mc = mc + gamma;
                }
                ks = ksn;
                if (lane == 0) { seg_ks[wid][c + 1] = ks; seg_mc[wid][c + 1] = mc; }
            }
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        const int nf = K - sp->n_extra;
        double carry = NaN;     // the residual of the row before this step's first (row -1: absent)
        for (int64_t base = 0; base < len; base += 64) {    // (the bound is the wave's: every lane takes every step)
            const int64_t t_row = base + lane;
            const bool in = t_row < len;
            const int64_t row = in ? t_row : len - 1;       // (a lane past the end evaluates the final row and drops it)
            const int64_t dsv = a.ds[d0 + row];
            const double t = (double)(dsv - gi.start_ns) / (double)gi.t_scale_ns;
            int c = 0;
            for (int j = 0; j < S; ++j) {
                double tcj = 0.0;
#pragma unroll
                for (int s = 0; s < (TSF_MAX_S + W - 1) / W; ++s)
                    if ((j >> 6) == s) tcj = readlane_f64(tl[s], j & 63);
                c += (c == j && t >= tcj) ? 1 : 0;
            }
            const double ks = seg_ks[wid][c], mc = seg_mc[wid][c];
            double xa = 0.0, xm = 0.0;
            for (int pass = 0; pass < 2; ++pass) {
                double acc = 0.0;
                for (int se = 0; se < sp->n_seas; ++se) {
                    const int col0 = sp->seas_col[se];
                    if ((sp->inv_perm[col0] < Ka) != (pass == 0)) continue;       // (a seasonality's columns share one mode)
                    double s1, c1;
                    dm_sincos(fourier_base_arg(dsv, sp->seas_period[se]), s1, c1);
                    fourier_harmonics(s1, c1, sp->seas_order[se], [&](int hh, double sv, double cv) {
                        const int col = col0 + 2 * (hh - 1);
                        acc = __builtin_fma(sv, beta[col], acc);
                        acc = __builtin_fma(cv, beta[col + 1], acc);
                    });
                }
                for (int e = 0; e < sp->n_extra; ++e) {
                    const int col = nf + e;
                    if ((sp->inv_perm[col] < Ka) != (pass == 0)) continue;
                    acc = __builtin_fma(a.extra[(size_t)e * a.extra_stride + d0 + row], beta[col], acc);
                }
                if (pass == 0) xa = acc; else xm = acc;
            }
            double gtr;
            if (sp->growth == TSF_GROWTH_LINEAR) {
                gtr = __builtin_fma(ks, t, mc);
            } else {
                const double z = ks * (t - mc);
                gtr = capsc * (1.0 / (1.0 + dm_exp(-z)));
            }
            const double trend = gtr * ys + fl;
            const double yh = trend * (1.0 + xm) + xa * ys;
            const bool kept = in && !(a.excluded && a.excluded[r0 + row] != 0);
            const double r = kept ? load_y(a.y, a.y_dtype, r0 + row) - yh : NaN;
            // ar_series_kernel's arithmetic on r
            const double left = __shfl(r, (lane + 63) & 63, 64);
            const double prev = (lane == 0) ? carry : left;
            carry = __shfl(r, 63, 64);
            const bool present = __builtin_isfinite(r);
            const bool pair = present && __builtin_isfinite(prev);
            ss = ss + (present ? r * r : 0.0);
            C = C + (pair ? r * prev : 0.0);
            cnt += present ? 1 : 0;
            np += pair ? 1 : 0;
            if (present) { top_t = t_row; top_r = r; }
        }
    }
    ss = corr_wave_sum(ss);
    C = corr_wave_sum(C);
    cnt = corr_wave_sum(cnt);
    np = corr_wave_sum(np);
    // ar_last_kernel's last present row: the highest of the lanes' highest
    int64_t hi_t = top_t;
    for (int d = 1; d <= 32; d <<= 1) {
        const int64_t o = (int64_t)__shfl_xor((long long)hi_t, d, 64);
        hi_t = o > hi_t ? o : hi_t;
    }
    const unsigned long long holder = __ballot(hi_t >= 0 && top_t == hi_t);
    const double hi_r = __shfl(top_r, holder ? __builtin_ctzll(holder) : 0, 64);
    if (lane != 0) return;
    const bool none = np < (int64_t)a.min_pairs || ss == 0.0;
    const double var = ss / (double)cnt;
    const double raw = none ? NaN : (C / (double)np) / var;
    a.phi[n] = none ? 0.0 : __builtin_fmin(__builtin_fmax(raw, 0.0), a.phi_max);
    a.status[n] = none ? no_pairs_status : ok_status;
    if (a.phi_raw) a.phi_raw[n] = raw;
    if (a.n_pairs) a.n_pairs[n] = np;
    if (a.scale) a.scale[n] = (ss == 0.0) ? NaN : __builtin_sqrt(var);
    a.last_resid[n] = hi_t >= 0 ? hi_r : 0.0;
    a.last_gap[n] = (int32_t)(hi_t >= 0 ? len - 1 - hi_t : len);
    a.last_status[n] = hi_t >= 0 ? ok_status : no_row_status;
    if (a.last_ds_ns) a.last_ds_ns[n] = len > 0 ? a.ds[d0 + len - 1] : INT64_MIN;
}

// The corrected point forecast behind predict_kernel: yhat [N][H] gains m_h (m_0 = m0, m_h = phi * m_(h-1): one product
// each, tsf_noise_ar_mean's values) for the series with phi != 0, one add per cell; yhat_int, where wanted, is the
// reference's post-step on the value that now stands in yhat.  pm: [N][2] = (phi, m0).
struct ConditionedArgs {
    const double *pm;
    const double *floor_;       // [N] or null: the clamp of the integer column
    double *yhat;
    int32_t *yhat_int;          // [N][H] or null
    int64_t N;
    int H;
};

__global__ __launch_bounds__(256) void conditioned_shift_kernel(ConditionedArgs a)
{
    const int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= a.N * a.H) return;
    const int64_t n = g / a.H;
    const int h = (int)(g - n * a.H);
    const double phi = a.pm[2 * (size_t)n];
    double yh = a.yhat[g];
    if (phi != 0.0) {
        double m = a.pm[2 * (size_t)n + 1];
        for (int k = 0; k < h; ++k) m = phi * m;
        yh = yh + m;
        a.yhat[g] = yh;
    }
    if (a.yhat_int) a.yhat_int[g] = yhat_post_int(yh, a.floor_ ? a.floor_[n] : 0.0);
}

}  // namespace tsf
