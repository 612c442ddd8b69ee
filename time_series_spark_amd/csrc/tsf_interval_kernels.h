// tsf_interval_kernels.h -- uncertainty intervals of the forecast (yhat_lower / yhat_upper):
// fbprophet's Prophet.predict_uncertainty, which the reference runs inside model.predict(future_df)
// (/root/reference/src/jobs/prophet_scorer.py:70) and then drops (:86).  SURVEY.md 8f-3.
//
// fbprophet draws from numpy's unseeded global generator, so there is no output to match; parity
// is DEFINED by oracle cn_predict_intervals: a counter-based generator keyed by (seed, series key,
// sample, stream), deterministic transcendentals, the sampled changepoint times generated already
// sorted.  These kernels consume the same streams in the same order: bit-identical to the oracle.
//   interval_sample_kernel      one thread per (series, sample): sweeps the future rows, writes
//                               samples[series][row][sample] (and, where asked, the sampled trend alike); its
//                               <true> instance chains the noise of a sample's rows (tsf_set_noise_ar), which is
//                               this library's own and not the oracle's: tests/ar_ref.py restates it; its
//                               <true, true> instance starts that chain conditioned on the history's last residual
//                               (tsf_set_noise_ar_start; tests/ar_start_ref.py)
//   ar_start_shift_kernel       one thread per (series, row): the conditioned start's mean added to the chunk's additive piece
//                               and to yhat, behind predict_kernel and in front of the sample kernel
//   interval_percentile_kernel  one workgroup per (series, row): bitonic sort of the samples in LDS,
//                               the two percentiles by linear interpolation (np.nanpercentile)
//   quantile_kernel             the same sort once per (series, row), then any number of levels from the sorted
//                               row (tsf_predict_quantiles: one launch per sample buffer -- yhat, running sum, trend)
// Non-template __global__ functions (and one template that only tsf_api.hip instantiates): include from exactly one
// translation unit (tsf_api.hip).
#pragma once
#include "tsf_common.h"

namespace tsf {

__device__ __forceinline__ uint64_t iv_mix64(uint64_t z)
{
    z += 0x9E3779B97F4A7C15ULL;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ULL;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBULL;
    return z ^ (z >> 31);
}
__device__ __forceinline__ uint64_t iv_key(uint64_t seed, uint64_t series_key, uint64_t sample, uint64_t stream)
{
    return iv_mix64(iv_mix64(iv_mix64(iv_mix64(seed) ^ series_key) ^ sample) ^ stream);
}
// In (0, 1], not (0, 1): above 2^52 the sum with 0.5 is a tie that rounds to even, so the top 53-bit value gives
// exactly 1.0 (probability 2^-53).  Every consumer stays finite there: dm_log(2 (1 - u)) = dm_log(0) = -1023 ln 2,
// dm_log(u) / rem = 0, z = 0 (tests/test_sampler_ref.py).  Every seeded bit depends on this map: it is not to change.
__device__ __forceinline__ double iv_u01(uint64_t key, uint64_t ctr)
{
    const uint64_t x = iv_mix64(key + 0x9E3779B97F4A7C15ULL * ctr);
    return ((double)(x >> 11) + 0.5) * 1.1102230246251565e-16;
}
__device__ __forceinline__ int iv_poisson(double lam, uint64_t key, uint64_t &ctr)
{
    int n = 0;
    double rest = lam;
    while (rest > 0.0 && n < 100000) {
        const double piece = rest < 8.0 ? rest : 8.0;
        const double L = dm_exp(-piece);
        double p = 1.0;
        int k = 0;
        do { p = p * iv_u01(key, ctr++); ++k; } while (p > L);
        n += k - 1;
        rest = rest - piece;
    }
    return n;
}

struct IntervalArgs {
    const DevSpec *sp;
    int64_t n0, n_chunk;        // series [n0, n0 + n_chunk) of the call
    int H, theta_stride, n_grids, NS;
    const double *theta, *y_scale;
    const tsf_grid_info *grid;
    const double *floor_, *cap;
    const double *t, *xa, *opm; // [N][H] from predict_kernel: scaled time, additive term * y_scale, 1 + multiplicative term
    const int64_t *series_key;  // [N] or nullptr (then the series index)
    uint64_t seed;
    double lo_frac, hi_frac;    // (1 - width) / 2, (1 + width) / 2
    double *samples;            // [n_chunk][H][NS]
    double *trend_samples;      // optional [n_chunk][H][NS]: each sample's trend before noise (tsf_predict_components)
    double *lower, *upper;      // [N][H]
    double *cum_samples;        // optional [n_chunk][H][NS]: each sample's running sum over rows 0..h (tsf_predict_quantiles)
    const double *noise_ar;     // optional [N][2]: each series' (phi, sqrt(1 - phi^2)) of tsf_set_noise_ar (the AR instance only)
    const double *ar_start;     // optional [N][3]: each series' (p0, c0, m0) of tsf_set_noise_ar_start (the START instance only)
};

// AR: the instance that chains the observation noise of a sample's rows (tsf_set_noise_ar); the other instance is the
// independent draw, whose code knows nothing of the chain.  START (with AR): the chain starts conditioned on the
// history's last residual, e_0 = c0 z_0; the conditional mean is not this kernel's business: ar_start_shift_kernel has
// put it into xa (and yhat) before.
template <bool AR, bool START = false>
__global__ __launch_bounds__(256) void interval_sample_kernel(IntervalArgs a)
{
    const int64_t nl = blockIdx.x, n = a.n0 + nl;
    const int s = (int)(blockIdx.y * blockDim.x + threadIdx.x);
    if (nl >= a.n_chunk || s >= a.NS) return;
    const DevSpec *sp = a.sp;
    const tsf_grid_info &gi = a.grid[a.n_grids == 1 ? 0 : n];
    const int S = gi.S, n_cp = sp->n_cp, H = a.H;
    const double *th = a.theta + (size_t)n * a.theta_stride;
    const double *delta = th + 3;
    (void)n_cp;
    const double ys = a.y_scale[n];
    const double fl = (sp->growth == TSF_GROWTH_LOGISTIC && a.floor_) ? a.floor_[n] : 0.0;
    const double cap_sc = (sp->growth == TSF_GROWTH_LOGISTIC) ? (a.cap[n] - fl) / ys : 0.0;
    const double sigma = dm_exp(th[2]);
    const double *t = a.t + (size_t)n * H, *xa = a.xa + (size_t)n * H, *opm = a.opm + (size_t)n * H;
    double Tm = -__builtin_huge_val();
    for (int h = 0; h < H; ++h) if (t[h] > Tm) Tm = t[h];
    const int S_cp = S > 0 ? S : 1;
    double lam_sum = 0.0;
    for (int j = 0; j < S; ++j) lam_sum = lam_sum + __builtin_fabs(delta[j]);
    const double lambda_ = lam_sum / (double)S_cp + 1e-8;
    const double rate = (Tm > 1.0) ? (double)S_cp * (Tm - 1.0) : 0.0;
    const uint64_t skey = a.series_key ? (uint64_t)a.series_key[n] : (uint64_t)n;
    const uint64_t kcp = iv_key(a.seed, skey, (uint64_t)s, 0), knz = iv_key(a.seed, skey, (uint64_t)s, 1);
    const double INF = __builtin_huge_val();
    double wk = 0.0, wm = 0.0, u_prev = 0.0, next_t = INF, next_delta = 0.0, t_last = -INF;
    int ih = 0, inew = 0, n_new = 0;
    uint64_t ctr = 0;
    double *out = a.samples + (size_t)nl * H * a.NS + s;
    double csum = 0.0;          // the running sum of this sample's rows, in the caller's row order (never restarted)
    // the noise chain of this sample's rows, in the caller's row order (never restarted either): e_0 = z_0 (the
    // stationary start), e_h = phi e_{h-1} + c z_h, two products and one add, each rounded
    double ar_phi = 0.0, ar_c = 0.0, ar_e = 0.0;
    if (AR) { ar_phi = a.noise_ar[2 * (size_t)n]; ar_c = a.noise_ar[2 * (size_t)n + 1]; }
    double ar_c0 = 1.0;
    if (START) ar_c0 = a.ar_start[3 * (size_t)n + 1];
    for (int h = 0; h < H; ++h) {
        const double th_ = t[h];
        if (h == 0 || th_ < t_last) {       // (re)start the sweep: the stream is replayed from 0
            wk = th[0]; wm = th[1]; ih = 0; inew = 0; ctr = 0; u_prev = 0.0;
            n_new = (rate > 0.0) ? iv_poisson(rate, kcp, ctr) : 0;
            next_t = INF;
        }
        t_last = th_;
        while (ih < S && th_ >= gi.t_change[ih]) {
            const double dj = delta[ih], kn = wk + dj, tc = gi.t_change[ih];
            if (sp->growth == TSF_GROWTH_LINEAR) wm = wm + ((-tc) * dj);
            else wm = wm + (tc - wm) * (1.0 - wk / kn);
            wk = kn; ++ih;
        }
        for (;;) {
            if (next_t == INF && inew < n_new) {
                const double v = iv_u01(kcp, ctr++);
                const double rem = (double)(n_new - inew);
                const double pw = dm_exp(dm_log(v) / rem);
                u_prev = 1.0 - (1.0 - u_prev) * pw;
                next_t = 1.0 + u_prev * (Tm - 1.0);
                const double ul = iv_u01(kcp, ctr++);
                next_delta = (ul < 0.5) ? lambda_ * dm_log(2.0 * ul) : -(lambda_ * dm_log(2.0 * (1.0 - ul)));
            }
            if (!(next_t <= th_)) break;
            const double dj = next_delta, kn = wk + dj;
            if (sp->growth == TSF_GROWTH_LINEAR) wm = wm + ((-next_t) * dj);
            else wm = wm + (next_t - wm) * (1.0 - wk / kn);
            wk = kn; ++inew; next_t = INF;
        }
        double gtr;
        if (sp->growth == TSF_GROWTH_LINEAR) gtr = __builtin_fma(wk, th_, wm);
        else gtr = cap_sc * (1.0 / (1.0 + dm_exp(-(wk * (th_ - wm)))));
        const double trend = gtr * ys + fl;
        const double u1 = iv_u01(knz, 2 * (uint64_t)h), u2 = iv_u01(knz, 2 * (uint64_t)h + 1);
        double sn, cs;
        dm_sincos(6.283185307179586 * u2, sn, cs);
        double z = __builtin_sqrt(-2.0 * dm_log(u1)) * cs;
        if (AR) {
            // (a select, not 0 * e + 1 * z: a series with phi == 0 keeps the independent draw's bits)
            if (START && h == 0 && ar_phi != 0.0) z = ar_c0 * z;
            if (h > 0 && ar_phi != 0.0) z = ar_phi * ar_e + ar_c * z;
            ar_e = z;
        }
        const double val = trend * opm[h] + xa[h] + (z * sigma) * ys;
        out[(size_t)h * a.NS] = val;
        if (a.cum_samples) {
            csum = (h == 0) ? val : csum + val;
            a.cum_samples[(size_t)nl * H * a.NS + s + (size_t)h * a.NS] = csum;
        }
        if (a.trend_samples) a.trend_samples[(size_t)nl * H * a.NS + s + (size_t)h * a.NS] = trend;
    }
}

// The conditional mean of the conditioned start, in y units: m_0 = m0, m_h = phi * m_(h-1) (one product each, what
// tsf_noise_ar_mean forms), added to the additive piece xa [n_chunk][H] of the chunk (so every sample of the row is
// trend * opm + (xa + m_h) + noise) and to yhat [N][H] of the call (yhat + m_h, one add).  A series with phi == 0 is not
// touched.  One thread per (series, row) of the chunk: the thread of row h forms m_h by the h products of the recursion in
// registers (the same roundings as a serial walk over the rows, without its chain of dependent memory round trips), so
// neighbouring lanes touch neighbouring rows.
struct ArStartArgs {
    const double *noise_ar, *ar_start;      // [N][2], [N][3] of the call
    double *xa;                             // [n_chunk][H] of the chunk
    double *yhat;                           // [N][H] of the call
    int64_t n0, n_chunk;
    int H;
};

__global__ __launch_bounds__(256) void ar_start_shift_kernel(ArStartArgs a)
{
    const int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= a.n_chunk * a.H) return;
    const int64_t i = g / a.H;
    const int h = (int)(g - i * a.H);
    const int64_t n = a.n0 + i;
    const double phi = a.noise_ar[2 * (size_t)n];
    if (phi == 0.0) return;
    double m = a.ar_start[3 * (size_t)n + 2];
    for (int k = 0; k < h; ++k) m = phi * m;
    a.xa[g] = a.xa[g] + m;
    double *yh = a.yhat + (size_t)n * a.H + h;
    *yh = *yh + m;
}

// The sort of the per-row kernels (here, tsf_score_kernels.h and tsf_window_kernels.h): NSP values in LDS (a power of
// two; the padding behind the real ones is +inf) through a bitonic network of compare-exchanges, ascending; it starts
// from values every thread can see (a barrier behind the load) and ends behind a barrier.  Exchanges move values and
// round nothing, so the sorted row is a function of the row's multiset alone.
__device__ __forceinline__ void iv_sort_network(double *v, int NSP)
{
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

// The NS values of one row into LDS, padded to NSP with +inf, then the network.
__device__ __forceinline__ void iv_load_sort(double *v, const double *src, int NS, int NSP)
{
    for (int i = threadIdx.x; i < NSP; i += blockDim.x) v[i] = (i < NS) ? src[i] : __builtin_huge_val();
    __syncthreads();
    iv_sort_network(v, NSP);
}

// NSP: NS rounded up to a power of two (<= 4096), the padding sorts to the end as +inf
__global__ __launch_bounds__(256) void interval_percentile_kernel(IntervalArgs a, int NSP)
{
    extern __shared__ __align__(16) unsigned char iv_smem[];
    double *v = reinterpret_cast<double *>(iv_smem);
    const int64_t nl = blockIdx.x / a.H;
    const int h = (int)(blockIdx.x - nl * a.H);
    const double *src = a.samples + ((size_t)nl * a.H + h) * a.NS;
    iv_load_sort(v, src, a.NS, NSP);
    if (threadIdx.x < 2) {
        const double pos = (threadIdx.x ? a.hi_frac : a.lo_frac) * (double)(a.NS - 1);
        int lo = (int)__builtin_floor(pos);
        if (lo > a.NS - 1) lo = a.NS - 1;
        const int hi = lo + 1 < a.NS ? lo + 1 : a.NS - 1;
        const double val = v[lo] + (v[hi] - v[lo]) * (pos - (double)lo);
        double *dst = threadIdx.x ? a.upper : a.lower;
        dst[(size_t)(a.n0 + nl) * a.H + h] = val;
    }
}

// tsf_predict_quantiles: one (series, row) of a chunk's sample buffer sorted once, every level read from the sorted
// row.  The sort and the interpolation are interval_percentile_kernel's, expression for expression, so a level formed
// as that kernel's lo_frac / hi_frac gives its bits.  The levels travel by value (TSF_MAX_QUANT doubles of kernel
// arguments); LDS: NSP doubles (<= 32 KB), as there.
struct QuantileArgs {
    const double *src;          // [n_chunk][H][NS] of the chunk
    double *dst;                // [N][n_q][H] of the call
    int64_t n0;                 // first series of the chunk
    int H, NS, n_q;
    double level[TSF_MAX_QUANT];
};

__global__ __launch_bounds__(256) void quantile_kernel(QuantileArgs a, int NSP)
{
    extern __shared__ __align__(16) unsigned char iv_smem[];
    double *v = reinterpret_cast<double *>(iv_smem);
    const int64_t nl = blockIdx.x / a.H;
    const int h = (int)(blockIdx.x - nl * a.H);
    const double *src = a.src + ((size_t)nl * a.H + h) * a.NS;
    iv_load_sort(v, src, a.NS, NSP);
    for (int q = threadIdx.x; q < a.n_q; q += blockDim.x) {
        const double pos = a.level[q] * (double)(a.NS - 1);
        int lo = (int)__builtin_floor(pos);
        if (lo > a.NS - 1) lo = a.NS - 1;
        const int hi = lo + 1 < a.NS ? lo + 1 : a.NS - 1;
        const double val = v[lo] + (v[hi] - v[lo]) * (pos - (double)lo);
        a.dst[((size_t)(a.n0 + nl) * a.n_q + q) * a.H + h] = val;
    }
}

}  // namespace tsf
