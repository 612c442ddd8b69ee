// tsf_api.hip -- C-ABI of libtsf_amd.so (include/tsf.h): context, device workspace, kernel
// dispatch, host-pointer convenience wrappers.
//
// The entry points stand where the reference calls into fbprophet per series:
//   fit      /root/reference/src/jobs/prophet_modeler.py:56-66
//   predict  /root/reference/src/jobs/prophet_scorer.py:64-84
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>
#include <algorithm>
#include <chrono>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <functional>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <utility>
#include <atomic>
#include <vector>

#include "tsf_aux_kernels.h"
#include "tsf_interval_kernels.h"
#include "tsf_score_kernels.h"
#include "tsf_window_kernels.h"
#include "tsf_rollup_kernels.h"
#include "tsf_reconcile_kernels.h"
#include "tsf_tree_kernels.h"
#include "tsf_temporal_kernels.h"
#include "tsf_component_kernels.h"
#include "tsf_fit_kernels.h"
#include "tsf_quad_kernels.h"
#include "tsf_mfma_tabs.h"
#include "tsf_launch.h"
#include "tsf_cv_kernels.h"
#include "tsf_tune_kernels.h"
#include "tsf_select_kernels.h"
#include "tsf_screen_kernels.h"
#include "tsf_calib_kernels.h"
#include "tsf_corr_kernels.h"
#include "tsf_ar_kernels.h"
#include "tsf_noise_state_kernels.h"
#include "tsf_cond_kernels.h"
#include "tsf_cv_plan.h"
#include "tsf_fit_plan.h"
#include "tsf_shares.h"

using namespace tsf;

struct tsf_ctx {
    int device;
    std::string err;
    // cached device workspace (grown on demand, never shrunk)
    void *ws;
    size_t ws_bytes;
    DevSpec *d_spec;
    void *nb_ws;            // slot records of the several-series-per-wave Newton kernel (grown on demand)
    size_t nb_ws_bytes;
    double *fut_tab;        // design table of a shared future grid (predict): [K][H]
    size_t fut_tab_bytes;
    void *iv_ws;            // sample scratch (ensure_iv_ws: per-row pieces + samples of one chunk of draw_chunks; grown on demand, <= ~0.5 GB)
    size_t iv_ws_bytes;
    void *comp_tab;         // tsf_predict_components: the component table ([TSF_MAX_COMP] masks, then [TSF_MAX_COMP] flags)
    int32_t *order_dev[2];  // tsf_set_cost_hints: series in order of decreasing expected cost (two buffers, used in
    size_t order_cap[2];    // turn: a fit that is still running on its stream keeps reading the one it was given)
    int order_next;
    int64_t order_n;        // series count the pending hints are for (0: none pending)
    std::vector<int32_t> cost_host;   // the pending hints themselves: a ragged call cut into length classes hands every class its share
    hipEvent_t order_ev[2]; // recorded behind the launch that reads order_dev[b]: the buffer is rewritten only after it
    int order_busy[2];
    int n_cu;               // compute units of the device (persistent kernels: one workgroup each)
    const int *last_sp_flag;  // sparse-column route of the last fit call: its device flag (in the workspace), or null
    int opt[TSF_OPT_COUNT];   // tsf_set_option: route switches of THIS context (-1 = the library's default)
    int profiling;
    hipEvent_t ev0[TSF_PROFILE_RING], ev1[TSF_PROFILE_RING];
    int ev_created;
    long ev_count;          // profiled calls since profiling was enabled
    FitPlan last_plan;      // what the last run_fit call planned (tsf_last_fit_plan; its n_grids: the grid tables it built)
    int64_t cv_grids;       // tsf_last_cv_grids: grid tables / fit launches of the last tsf_cross_validate call
    int32_t cv_launches;
    int32_t tune_expand;    // tsf_last_tune_counts: fold panels cut / fit launches of the last tsf_tune call
    int32_t tune_fits;
    std::vector<double> ar_pending;   // tsf_set_noise_ar: the pending (phi, c) pairs, [n][2]; empty: none pending
    std::vector<double> ar_start_pending;   // tsf_set_noise_ar_start: the pending (p0, c0, m0), [n][3], beside ar_pending
    double *ar_dev;         // the pairs of the draw that took them, on the device (grown on demand); behind them its starts
    size_t ar_dev_bytes;
};

#define HIP_TRY(ctx, expr)                                                                   \
    do {                                                                                     \
        hipError_t e_ = (expr);                                                              \
        if (e_ != hipSuccess) {                                                              \
            (ctx)->err = std::string(#expr) + ": " + hipGetErrorString(e_);                  \
            return -2;                                                                       \
        }                                                                                    \
    } while (0)

static int fail(tsf_ctx *ctx, const char *msg)
{
    if (ctx) ctx->err = msg;
    return -1;
}

extern "C" int tsf_device_count(void)
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

extern "C" int tsf_create(int device_id, tsf_ctx **out)
{
    if (!out) return -1;
    *out = nullptr;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || device_id < 0 || device_id >= n) return -2;
    if (hipSetDevice(device_id) != hipSuccess) return -2;
    tsf_ctx *c = new tsf_ctx();
    c->device = device_id; c->ws = nullptr; c->ws_bytes = 0; c->d_spec = nullptr;
    c->fut_tab = nullptr; c->fut_tab_bytes = 0;
    c->nb_ws = nullptr; c->nb_ws_bytes = 0;
    c->iv_ws = nullptr; c->iv_ws_bytes = 0;
    c->comp_tab = nullptr;
    c->ar_dev = nullptr; c->ar_dev_bytes = 0;
    c->order_dev[0] = c->order_dev[1] = nullptr; c->order_cap[0] = c->order_cap[1] = 0; c->order_next = 0; c->order_n = 0;
    c->order_ev[0] = c->order_ev[1] = nullptr; c->order_busy[0] = c->order_busy[1] = 0;
    c->profiling = 0; c->ev_created = 0; c->ev_count = 0;
    c->last_sp_flag = nullptr;
    memset(&c->last_plan, 0, sizeof(c->last_plan)); c->cv_grids = 0; c->cv_launches = 0; c->tune_expand = 0; c->tune_fits = 0;
    for (int i = 0; i < TSF_OPT_COUNT; ++i) c->opt[i] = -1;
    if (hipMalloc((void **)&c->d_spec, sizeof(DevSpec)) != hipSuccess) { delete c; return -2; }
    {
        hipDeviceProp_t prop;
        c->n_cu = (hipGetDeviceProperties(&prop, device_id) == hipSuccess) ? prop.multiProcessorCount : 256;
    }
    // (No hipMallocAsync anywhere in this library, and the device's default memory pool is left as the process
    // set it: round 3 measured intermittently wrong Newton fits after gigabytes of stream-ordered scratch
    // (DESIGN 5b), cause not found; every scratch buffer is a cached hipMalloc block of the context.)
    *out = c;
    return 0;
}

namespace { void pool_trim(int device); }    // host-pointer buffer cache, below

extern "C" void tsf_destroy(tsf_ctx *ctx)
{
    if (!ctx) return;
    hipSetDevice(ctx->device);
    pool_trim(ctx->device);
    if (ctx->ws) hipFree(ctx->ws);
    if (ctx->d_spec) hipFree(ctx->d_spec);
    if (ctx->fut_tab) hipFree(ctx->fut_tab);
    if (ctx->nb_ws) hipFree(ctx->nb_ws);
    if (ctx->iv_ws) hipFree(ctx->iv_ws);
    if (ctx->comp_tab) hipFree(ctx->comp_tab);
    if (ctx->ar_dev) hipFree(ctx->ar_dev);
    for (int b = 0; b < 2; ++b) { if (ctx->order_dev[b]) hipFree(ctx->order_dev[b]); if (ctx->order_ev[b]) hipEventDestroy(ctx->order_ev[b]); }
    if (ctx->ev_created)
        for (int i = 0; i < TSF_PROFILE_RING; ++i) { hipEventDestroy(ctx->ev0[i]); hipEventDestroy(ctx->ev1[i]); }
    delete ctx;
}

extern "C" const char *tsf_last_error(const tsf_ctx *ctx) { return ctx ? ctx->err.c_str() : "null context"; }

extern "C" int tsf_set_option(tsf_ctx *ctx, int option, int value)
{
    if (!ctx) return -1;
    if (option < 0 || option >= TSF_OPT_COUNT) return fail(ctx, "unknown option");
    ctx->opt[option] = value;
    return 0;
}

extern "C" int tsf_get_option(const tsf_ctx *ctx, int option)
{
    if (!ctx || option < 0 || option >= TSF_OPT_COUNT) return -1;
    return ctx->opt[option];
}

extern "C" void tsf_spec_default(tsf_spec *s)
{
    memset(s, 0, sizeof(*s));
    s->growth = TSF_GROWTH_LINEAR; s->n_changepoints = 25; s->changepoint_range = 0.8;
    s->changepoint_prior_scale = 0.05;
    s->max_iter = 10000; s->history = 5; s->init_alpha = 1e-3; s->tol_obj = 1e-12;
    s->tol_rel_obj = 1e4; s->tol_grad = 1e-8; s->tol_rel_grad = 1e7; s->tol_param = 1e-8;
    s->eval_form = TSF_EVAL_AUTO;
    s->algorithm = TSF_ALGO_LBFGS;
    s->residual_kernel = TSF_RK_AUTO; s->recenter_every = 128; s->recenter_ratio = 1.0;
    s->coop_after = -1;
    s->converge = TSF_CONVERGE_STAN; s->map_max_iter = 10000; s->map_tol = 1e-7;
}

extern "C" int tsf_spec_size(void) { return (int)sizeof(tsf_spec); }
extern "C" int tsf_grid_info_size(void) { return (int)sizeof(tsf_grid_info); }

extern "C" int tsf_spec_K(const tsf_spec *s)
{
    int K = s->n_extra;
    for (int i = 0; i < s->n_seas; ++i) K += 2 * s->seas_order[i];
    return K;
}

extern "C" int tsf_theta_stride(const tsf_spec *s) { return 3 + s->n_changepoints + tsf_spec_K(s); }

// ---- spec validation + device form ---------------------------------------------------------

static int pick_KP(int K, int n_cp, int mixed)
{
    const int P = fit_P(n_cp, K);
    if (mixed || P > 64) return 64;
    if (K <= 8) return 8;
    if (K <= 16) return 16;
    if (K <= 28) return 28;
    return 64;
}

// (also asked by the panel jobs before they upload anything: they apply the optimiser rule to `algorithm` themselves)
static int check_algorithm(tsf_ctx *ctx, const tsf_spec *s)
{
    return s->algorithm < TSF_ALGO_LBFGS || s->algorithm > TSF_ALGO_AUTO ? fail(ctx, "bad algorithm") : 0;
}

static int build_devspec(tsf_ctx *ctx, const tsf_spec *s, DevSpec *d, int *mode_out)
{
    if (!s) return fail(ctx, "spec is NULL");
    if (s->growth != TSF_GROWTH_LINEAR && s->growth != TSF_GROWTH_LOGISTIC) return fail(ctx, "bad growth");
    if (s->n_seas < 0 || s->n_seas > TSF_MAX_SEAS || s->n_extra < 0 || s->n_extra > TSF_MAX_EXTRA)
        return fail(ctx, "too many seasonalities / extra columns");
    if (s->n_changepoints < 0 || s->n_changepoints > TSF_MAX_S) return fail(ctx, "n_changepoints out of range");
    if (s->changepoints_specified != 0 && s->changepoints_specified != 1) return fail(ctx, "changepoints_specified must be 0 or 1");
    // (fbprophet ignores changepoint_range when the dates are given)
    if (!s->changepoints_specified && !(s->changepoint_range >= 0.0 && s->changepoint_range <= 1.0)) return fail(ctx, "changepoint_range must be in [0,1]");
    if (s->changepoints_specified)
        for (int j = 1; j < s->n_changepoints; ++j)
            if (s->changepoint_ns[j] <= s->changepoint_ns[j - 1]) return fail(ctx, "changepoint_ns must be strictly ascending");
    if (!(s->changepoint_prior_scale > 0.0)) return fail(ctx, "changepoint_prior_scale must be > 0");
    if (s->history < 1 || s->history > MAXH) return fail(ctx, "history must be in [1,8]");
    if (s->eval_form < TSF_EVAL_AUTO || s->eval_form > TSF_EVAL_QUADRATIC) return fail(ctx, "bad eval_form");
    if (int rc = check_algorithm(ctx, s)) return rc;
    if (s->residual_kernel < TSF_RK_AUTO || s->residual_kernel > TSF_RK_COOP) return fail(ctx, "bad residual_kernel");
    if (s->converge != TSF_CONVERGE_STAN && s->converge != TSF_CONVERGE_MAP) return fail(ctx, "bad converge");
    if (s->converge == TSF_CONVERGE_MAP && (s->map_max_iter < 1 || !(s->map_tol > 0.0))) return fail(ctx, "map_max_iter must be >= 1 and map_tol > 0");
    if (s->eval_form != TSF_EVAL_RESIDUAL && (s->recenter_every < 1 || !(s->recenter_ratio > 0.0)))
        return fail(ctx, "recenter_every must be >= 1 and recenter_ratio > 0");
    const int K = tsf_spec_K(s);
    if (K < 1) return fail(ctx, "model needs at least one design column (fbprophet adds a zero column; pass one extra column of zeros)");
    if (K > TSF_MAX_K || fit_P(s->n_changepoints, K) > TSF_MAX_P) return fail(ctx, "too many parameters (3+S+K must be <= 128, K <= 64)");
    memset(d, 0, sizeof(*d));
    int mode[TSF_MAX_P];
    double pr[TSF_MAX_P];
    int col = 0, np = 0;
    for (int i = 0; i < s->n_seas; ++i) {
        if (s->seas_order[i] < 1) return fail(ctx, "fourier order must be >= 1");
        if (!(s->seas_prior_scale[i] > 0.0) || !(s->seas_period[i] > 0.0)) return fail(ctx, "bad seasonality prior scale / period");
        d->seas_period[i] = s->seas_period[i]; d->seas_order[i] = s->seas_order[i]; d->seas_col[i] = col;
        for (int h = 0; h < s->seas_order[i]; ++h) {
            np++;
            mode[col] = s->seas_mode[i]; pr[col] = s->seas_prior_scale[i]; col++;
            mode[col] = s->seas_mode[i]; pr[col] = s->seas_prior_scale[i]; col++;
        }
    }
    for (int e = 0; e < s->n_extra; ++e) {
        if (!(s->extra_prior_scale[e] > 0.0)) return fail(ctx, "bad extra prior scale");
        mode[col] = s->extra_mode[e]; pr[col] = s->extra_prior_scale[e]; col++;
    }
    int n = 0;
    for (int j = 0; j < K; ++j) if (mode[j] == TSF_MODE_ADDITIVE) { d->perm[n] = j; d->inv_perm[j] = n; d->prior[n] = pr[j]; n++; }
    const int Ka = n;
    for (int j = 0; j < K; ++j) if (mode[j] != TSF_MODE_ADDITIVE) { d->perm[n] = j; d->inv_perm[j] = n; d->prior[n] = pr[j]; n++; }
    for (int j = K; j < TSF_MAX_P; ++j) d->prior[j] = 1.0;
    const int m = (Ka == K) ? 0 : (Ka == 0 ? 1 : 2);
    d->growth = s->growth; d->n_cp = s->n_changepoints; d->K = K; d->Ka = Ka;
    d->KP = pick_KP(K, s->n_changepoints, m == 2);
    d->n_seas = s->n_seas; d->n_extra = s->n_extra; d->n_pairs = np;
    d->max_iter = s->max_iter; d->history = s->history;
    // harmonic structure (harm_code): one column mode (then the internal column order is fbprophet's: the seasonalities'
    // Fourier columns first, in order) and at most three seasonalities; whether a kernel is compiled for it is the
    // launch function's business (tsf_inst.inc)
    d->harm = 0;
    if (m != 2 && s->n_seas >= 1 && s->n_seas <= 3) {
        bool ok = true;
        for (int i = 0; i < s->n_seas; ++i) ok = ok && s->seas_order[i] <= 255;
        if (ok) d->harm = harm_code(s->seas_order[0], s->n_seas > 1 ? s->seas_order[1] : 0, s->n_seas > 2 ? s->seas_order[2] : 0);
    }
    d->cp_range = s->changepoint_range; d->tau = s->changepoint_prior_scale;
    d->cp_spec = s->changepoints_specified;
    if (d->cp_spec) {
        d->cp_range = 0.0;
        for (int j = 0; j < s->n_changepoints; ++j) d->cp_ns[j] = s->changepoint_ns[j];
    }
    d->init_alpha = s->init_alpha; d->tol_obj = s->tol_obj; d->tol_rel_obj = s->tol_rel_obj;
    d->tol_grad = s->tol_grad; d->tol_rel_grad = s->tol_rel_grad; d->tol_param = s->tol_param;
    *mode_out = m;
    return 0;
}

// ---- workspace ------------------------------------------------------------------------------

struct WsLayout {
    size_t gtab, stab, tw, cw, Xw, yw, Mg, Mslot, rbuf, counter, uw, Xu, spm, spp, Bw;
    size_t mXF, mXB, mXT, mtq, mcq, mcpof, myq, mhist;      // matrix-core path (tsf_mfma_kernels.h)
    size_t clist, cslots;                                   // cooperative tail (tsf_coop_kernels.h)
    size_t total;
};

// bytes of cached Newton slot records (tsf_ctx::nb_ws) that may outlive a call that does not use them
constexpr size_t TSF_NB_KEEP = (size_t)1 << 30;

static size_t align_up(size_t x) { return (x + 255) & ~(size_t)255; }

static WsLayout ws_layout(int64_t N, const FitPlan &p, int KP)
{
    const int64_t n_grids = p.n_grids, lat_U = p.lat_U;
    const int NTmax = p.NTmax, bw_ns = p.bw_ns;
    WsLayout l;
    size_t off = 0;
    l.gtab = off; off = align_up(off + sizeof(GridTab) * (size_t)n_grids);
    l.stab = off; off = align_up(off + sizeof(SeriesTab) * (size_t)N);
    l.tw = off; off = align_up(off + sizeof(double) * (size_t)n_grids * NTmax * W);
    l.cw = off; off = align_up(off + sizeof(uint16_t) * (size_t)n_grids * NTmax * W);
    // lattice panels (lat_U > 0) keep one shared table Xu and a row index per series row
    // instead of a design matrix per grid
    l.Xw = off; off = align_up(off + (lat_U > 0 ? 0 : sizeof(double) * (size_t)n_grids * NTmax * KP * W));
    l.yw = off; off = align_up(off + (p.raw_y ? 0 : sizeof(double) * (size_t)N * NTmax * W));
    // one Gram matrix for an aligned panel; quad_pre of them for a ragged panel whose series share timestamp vectors
    l.Mg = off; off = align_up(off + sizeof(double) * (size_t)p.qp.P4 * 2 * W * (size_t)(p.quad_pre > 0 ? p.quad_pre : 1));
    l.Mslot = off; off = align_up(off + (p.quad_ragged ? sizeof(double) * (size_t)p.qp.slots * p.qp.P4 * 2 * W : 0));
    l.rbuf = off; off = align_up(off + sizeof(double) * (size_t)p.qp.slots * NTmax * W);
    l.counter = off; off = align_up(off + 256);
    // sparse indicator columns (SP_* in tsf_fit_kernels.h): the lanes' entries and the columns' fold programs per grid
    l.spm = off; off = align_up(off + (p.sparse_try ? sizeof(uint32_t) * (size_t)n_grids * SP_M * W : 0));
    l.spp = off; off = align_up(off + (p.sparse_try ? sizeof(unsigned long long) * (size_t)n_grids * SP_MAXC : 0));
    // base pairs of the Fourier columns (fit_kernel<..., HARM>): two doubles per seasonality and row
    // (a panel on a timestamp lattice: per lattice POINT, one table for every series -- FitArgs::Bu)
    l.Bw = off; off = align_up(off + sizeof(double) * (lat_U > 0 ? (size_t)lat_U * bw_ns * 2 : (size_t)n_grids * NTmax * bw_ns * 2 * W));
    l.uw = off; off = align_up(off + (lat_U > 0 ? sizeof(int32_t) * (size_t)n_grids * NTmax * W : 0));
    l.Xu = off; off = align_up(off + (lat_U > 0 ? sizeof(double) * (size_t)lat_U * KP : 0));
    const MfmaPlan &mp = p.mp;
    const size_t tiles = mp.on ? (size_t)W * mp.NG : 0;
    l.mXF = off; off = align_up(off + (mp.on ? sizeof(double) * tiles * mp.KF * W : 0));
    l.mXB = off; off = align_up(off + (mp.on ? sizeof(double) * tiles * 4 * mp.NCB * W : 0));
    l.mXT = off; off = align_up(off + (mp.on ? sizeof(double) * tiles * 4 * W : 0));
    l.mtq = off; off = align_up(off + (mp.on ? sizeof(double) * tiles * 16 : 0));
    l.mcq = off; off = align_up(off + (mp.on ? sizeof(uint16_t) * tiles * 16 : 0));
    l.mcpof = off; off = align_up(off + (mp.on ? (size_t)W * 8 : 0));
    l.myq = off; off = align_up(off + (mp.on ? sizeof(double) * (size_t)N * tiles * 16 : 0));
    l.mhist = off; off = align_up(off + (mp.on ? sizeof(double) * (size_t)mp.blocks * MT_NS * 2 * MAXH * W : 0));
    l.clist = off; off = align_up(off + sizeof(int32_t) * (size_t)p.coop_slots);
    l.cslots = off; off = align_up(off + sizeof(double) * (size_t)p.coop_slots * p.coop_stride);
    l.total = off;
    return l;
}

static int ensure_ws(tsf_ctx *ctx, size_t bytes, int64_t N = 0, int NTmax = 0, int ragged = 0)
{
    if (ctx->ws_bytes >= bytes) return 0;
    {
        // a ragged panel pads EVERY series' tables to the longest series of the call: say so instead of
        // failing inside hipMalloc
        size_t free_b = 0, total_b = 0;
        if (hipMemGetInfo(&free_b, &total_b) == hipSuccess && bytes > free_b + ctx->ws_bytes && (ctx->nb_ws || ctx->iv_ws)) {
            // the cached scratch of other entry points (Newton slot records: up to 6 GB; interval samples) gives way
            if (ctx->nb_ws) { (void)hipFree(ctx->nb_ws); ctx->nb_ws = nullptr; ctx->nb_ws_bytes = 0; }
            if (ctx->iv_ws) { (void)hipFree(ctx->iv_ws); ctx->iv_ws = nullptr; ctx->iv_ws_bytes = 0; }
            (void)hipMemGetInfo(&free_b, &total_b);
        }
        if (free_b + total_b > 0 && bytes > free_b + ctx->ws_bytes) {
            char msg[384];
            snprintf(msg, sizeof(msg), "workspace of %.1f GB does not fit the device (%.1f GB free): %lld series, the longest has "
                     "%d rows%s", bytes / 1e9, (free_b + ctx->ws_bytes) / 1e9, (long long)N, NTmax * W,
                     ragged ? " and every series of a ragged call is padded to it -- split the call by series length" : "");
            ctx->err = msg;
            return -2;
        }
        (void)hipGetLastError();
    }
    ctx->last_sp_flag = nullptr;       // (it points into the workspace that goes away here)
    if (ctx->ws) { HIP_TRY(ctx, hipFree(ctx->ws)); ctx->ws = nullptr; ctx->ws_bytes = 0; }
    HIP_TRY(ctx, hipMalloc(&ctx->ws, bytes));
    ctx->ws_bytes = bytes;
    return 0;
}

typedef int (*launch_t)(int, const FitArgs &, int, hipStream_t);
typedef int (*launch_newton_t)(int, const FitArgs &, int, hipStream_t);
static launch_newton_t pick_newton_launch(int growth, int mode)
{
    static const launch_newton_t tab[2][3] = {{launch_newton_g0m0, launch_newton_g0m1, launch_newton_g0m2},
                                              {launch_newton_g1m0, launch_newton_g1m1, launch_newton_g1m2}};
    return tab[growth][mode];
}

typedef int (*launch_map_t)(int, const FitArgs &, hipStream_t);
static launch_map_t pick_map_launch(int growth, int mode)
{
    static const launch_map_t tab[2][3] = {{launch_map_g0m0, launch_map_g0m1, launch_map_g0m2},
                                           {launch_map_g1m0, launch_map_g1m1, launch_map_g1m2}};
    return tab[growth][mode];
}

static launch_t pick_launch(int growth, int mode)
{
    static const launch_t tab[2][3] = {{launch_g0m0, launch_g0m1, launch_g0m2},
                                       {launch_g1m0, launch_g1m1, launch_g1m2}};
    return tab[growth][mode];
}

// ---- the fit driver -------------------------------------------------------------------------

// One fit (or evaluation) launch on device pointers: what an entry point hands to run_fit.
struct FitCall {
    // the panel: aligned [N][T] on one timestamp vector ds [T], or ragged rows [offsets[n], offsets[n + 1]) of
    // ds / y [total_rows], the longest series max_T rows
    int64_t N;
    int aligned;
    int32_t T;
    const int64_t *offsets;
    int64_t total_rows;
    int32_t max_T;
    const int64_t *ds;
    const void *y;
    int32_t y_dtype;
    const double *floor, *cap, *extra;
    // evaluation only (tsf_eval: theta_in, grad_out; tsf_eval_quadratic: around theta_ref too)
    const double *theta_in;
    double *grad_out;
    const double *theta_ref;
    // ragged panel on a timestamp lattice base + u * step, u < U (lat_step 0: none)
    int64_t lat_base, lat_step, lat_U;
    // ragged panel whose series share timestamp vectors: class of each series [N], (first row, rows) per class
    // [n_distinct][2], the order in which the launch starts the series [N], rows of a class's tables to keep (CV)
    const int32_t *grid_of;
    const int64_t *grid_rows;
    int64_t n_distinct;
    const int32_t *grid_order, *grid_keep;
    hipStream_t stream;
};

// what the steps of one run_fit call share
struct FitRun {
    tsf_ctx *ctx;
    const tsf_spec *spec;
    const FitCall *c;
    DevSpec hs;
    int mode;
    FitPlan p;
    WsLayout l;
    char *ws;
    const int32_t *grid_of;     // the call's calendar classes where the plan uses them, else null
    const int64_t *grid_rows;
    int slot;                   // profiling ring slot of this call
};

static int fit_validate(tsf_ctx *ctx, const tsf_spec *spec, const FitCall &c, const tsf_fit_out *out, DevSpec *hs, int *mode)
{
    if (c.N <= 0) return fail(ctx, "N must be > 0");
    if (!c.ds || !c.y || !out) return fail(ctx, "NULL input");
    if (c.y_dtype < TSF_Y_F64 || c.y_dtype > TSF_Y_I32) return fail(ctx, "bad y_dtype");
    int rc = build_devspec(ctx, spec, hs, mode);
    if (rc) return rc;
    if (hs->n_extra > 0 && !c.extra) return fail(ctx, "extra columns declared but extra is NULL");
    if (hs->growth == TSF_GROWTH_LOGISTIC && !c.cap) return fail(ctx, "logistic growth needs cap");
    return 0;
}

static tsf_fit_shape fit_shape(const FitCall &c)
{
    tsf_fit_shape sh;
    memset(&sh, 0, sizeof(sh));
    sh.N = c.N; sh.aligned = c.aligned; sh.Tm = c.aligned ? c.T : c.max_T;
    sh.call = !c.theta_in ? TSF_CALL_FIT : (c.theta_ref ? TSF_CALL_EVAL_QUADRATIC : TSF_CALL_EVAL);
    sh.classes = c.grid_of && c.grid_rows; sh.n_distinct = c.n_distinct;
    sh.lat_step = c.lat_step; sh.lat_U = c.lat_U;
    return sh;
}

// plan_fit's memory query: what is free now + the context's own cached workspace
static int64_t ctx_mem_avail(void *arg)
{
    const tsf_ctx *ctx = (const tsf_ctx *)arg;
    size_t free_b = 0, total_b = 0;
    if (hipMemGetInfo(&free_b, &total_b) == hipSuccess) return (int64_t)(free_b + ctx->ws_bytes);
    (void)hipGetLastError();
    return -1;
}

// the set-up launches: the spec, the grids' tables (lattice / per grid), the sparse-column programs, the series' rows
static int fit_setup(const FitRun &r)
{
    tsf_ctx *ctx = r.ctx;
    const FitCall &c = *r.c;
    const FitPlan &p = r.p;
    const WsLayout &l = r.l;
    const DevSpec &hs = r.hs;
    char *ws = r.ws;
    hipStream_t st = c.stream;
    const int64_t n_grids = p.n_grids, lat_U = p.lat_U;
    const int NTmax = p.NTmax, bw_ns = p.bw_ns;
    GridTab *gtab = (GridTab *)(ws + l.gtab);
    double *Xw = (double *)(ws + l.Xw);
    HIP_TRY(ctx, hipMemcpyAsync(ctx->d_spec, &hs, sizeof(hs), hipMemcpyHostToDevice, st));
    if (lat_U > 0) {
        double *Xu = (double *)(ws + l.Xu);
        HIP_TRY(ctx, hipMemsetAsync(Xu, 0, sizeof(double) * (size_t)lat_U * hs.KP, st));
        // (rows a lane's chunk does not have point at lattice point 0: the base-pair kernels gather before they mask)
        HIP_TRY(ctx, hipMemsetAsync(ws + l.uw, 0, sizeof(int32_t) * (size_t)n_grids * NTmax * W, st));
        const int64_t work = lat_U * (hs.n_seas > 0 ? hs.n_seas : 1);
        hipLaunchKernelGGL(setup_lattice_kernel, dim3((unsigned)((work + 255) / 256 > 65535 ? 65535 : (work + 255) / 256)),
                           dim3(256), 0, st, ctx->d_spec, lat_U, c.lat_base, c.lat_step, Xu, bw_ns ? (double *)(ws + l.Bw) : (double *)nullptr);
        HIP_TRY(ctx, hipGetLastError());
    } else {
        HIP_TRY(ctx, hipMemsetAsync(Xw, 0, sizeof(double) * (size_t)n_grids * NTmax * hs.KP * W, st));
        // (the base pairs too: rows past a chunk's end are (0, 0) -- every harmonic 0 --, never stale bits that could be
        // NaN or Inf under an `fma(x, 0, acc)` that relies on finite x; round-5 advice)
        if (bw_ns) HIP_TRY(ctx, hipMemsetAsync(ws + l.Bw, 0, sizeof(double) * (size_t)n_grids * NTmax * bw_ns * 2 * W, st));
    }
    HIP_TRY(ctx, hipMemsetAsync(gtab, 0, sizeof(GridTab) * (size_t)n_grids, st));
    hipLaunchKernelGGL(setup_grid_kernel, dim3((unsigned)n_grids), dim3(256), 0, st, ctx->d_spec,
                       (int)n_grids, c.aligned ? nullptr : c.offsets, c.T, c.ds, c.extra,
                       c.aligned ? (int64_t)c.T : c.total_rows, NTmax, gtab, (double *)(ws + l.tw), (uint16_t *)(ws + l.cw), Xw,
                       (int32_t *)(ws + l.uw), c.lat_base, lat_U > 0 ? c.lat_step : (int64_t)0, r.grid_rows,
                       (bw_ns && lat_U == 0) ? (double *)(ws + l.Bw) : (double *)nullptr, c.grid_keep);
    HIP_TRY(ctx, hipGetLastError());
    if (p.sparse_try) {
        int *sp_bad = (int *)(ws + l.counter) + 8;
        HIP_TRY(ctx, hipMemsetAsync(sp_bad, 0, sizeof(int), st));
        hipLaunchKernelGGL(sparse_extra_kernel, dim3((unsigned)n_grids), dim3(64), 0, st, ctx->d_spec, gtab, Xw, NTmax,
                           (uint32_t *)(ws + l.spm), (unsigned long long *)(ws + l.spp), sp_bad);
        HIP_TRY(ctx, hipGetLastError());
    }
    // (raw_y: the quadratic-form fit kernel derives the scale and the initial values from the caller's rows itself --
    // series_tab_wave, tsf_quad_kernels.h -- and no kernel of that route reads SeriesTab or yw)
    if (!p.raw_y) {
        hipLaunchKernelGGL(setup_series_kernel, dim3((unsigned)c.N), dim3(64), 0, st, ctx->d_spec, c.N,
                           c.aligned ? nullptr : c.offsets, c.T, c.ds, c.y, c.y_dtype, c.floor, c.cap, NTmax, gtab,
                           c.aligned, (SeriesTab *)(ws + l.stab), (double *)(ws + l.yw), r.grid_of);
        HIP_TRY(ctx, hipGetLastError());
    }
    return 0;
}

// the fit kernels' arguments (the route's own additions are its launch step's)
static FitArgs fit_args(const FitRun &r, const tsf_fit_out *out)
{
    const tsf_ctx *ctx = r.ctx;
    const FitCall &c = *r.c;
    const FitPlan &p = r.p;
    const WsLayout &l = r.l;
    const DevSpec &hs = r.hs;
    char *ws = r.ws;
    const int64_t lat_U = p.lat_U;
    const int bw_ns = p.bw_ns, harm = p.harm;
    FitArgs a;
    memset(&a, 0, sizeof(a));
    a.sp = ctx->d_spec; a.N = c.N; a.aligned = c.aligned; a.NTmax = p.NTmax;
    a.theta_stride = tsf_theta_stride(r.spec);
    {
        const double eps = 2.220446049250313e-16;
        a.opt.init_alpha = hs.init_alpha; a.opt.tol_obj = hs.tol_obj;
        a.opt.tol_rel_obj_eps = hs.tol_rel_obj * eps; a.opt.tol_grad = hs.tol_grad;
        a.opt.tol_rel_grad_eps = hs.tol_rel_grad * eps; a.opt.tol_param = hs.tol_param;
        a.opt.max_iter = hs.max_iter; a.opt.history = hs.history;
    }
    a.gtab = (GridTab *)(ws + l.gtab); a.stab = (SeriesTab *)(ws + l.stab); a.tw = (double *)(ws + l.tw);
    a.yw = p.raw_y ? (double *)nullptr : (double *)(ws + l.yw); a.Xw = (double *)(ws + l.Xw); a.cw = (uint16_t *)(ws + l.cw);
    a.theta = out->theta; a.y_scale = out->y_scale; a.fval = out->fval; a.status = out->status;
    a.n_iter = out->n_iter; a.n_eval = out->n_eval; a.grid_out = out->grid;
    a.theta_in = c.theta_in; a.grad_out = c.grad_out;
    if (p.raw_y) { a.y_raw = c.y; a.y_raw_dtype = c.y_dtype; a.y_offsets = c.aligned ? nullptr : c.offsets; a.y_T = c.T; }
    a.uw = (const int32_t *)(ws + l.uw); a.Xu = (const double *)(ws + l.Xu); a.xidx = lat_U > 0 ? 1 : 0;
    a.grid_of = r.grid_of;
    a.Bw = (bw_ns && lat_U == 0) ? (const double *)(ws + l.Bw) : nullptr; a.bw_ns = bw_ns; a.harm = harm;
    a.Bu = (bw_ns && lat_U > 0) ? (const double *)(ws + l.Bw) : nullptr;
    a.coop_harm = (harm != 0 && hs.K == harm_kf(harm) && r.mode != 2) ? 1 : 0;
    {
        // rows of the one-wave base-pair kernel from HBM?  (tables per grid: segment words, t, base pairs; y per series)
        const size_t row_tabs = (size_t)p.n_grids * p.NTmax * W * (sizeof(double) + sizeof(uint16_t) + sizeof(double) * 2 * (size_t)bw_ns) +
                                (size_t)c.N * p.NTmax * W * sizeof(double);
        const int oh = ctx->opt[TSF_OPT_HARM];
        a.harm_pf = (harm != 0 && (oh == 2 || (oh != 1 && !c.aligned && row_tabs > ((size_t)256 << 20)))) ? 1 : 0;
        if (harm != 0 && lat_U > 0) a.harm_pf = 1;         // (the lattice form exists with the row prefetch only)
    }
    a.opt_coop_sparse = ctx->opt[TSF_OPT_SPARSE_EXTRA] != 2 ? 1 : 0;     // (2: the sparse fit kernel with the 64-column tail, for A/B runs)
    if (p.sparse_try) {
        a.sp_meta = (const uint32_t *)(ws + l.spm); a.sp_prog = (const unsigned long long *)(ws + l.spp);
        a.sp_flag = (int *)(ws + l.counter) + 8;
    }
    return a;
}

// scheduling hints of tsf_set_cost_hints: for this call if they were given for this many series; used once.
// Returns the hint buffer the launch reads, or -1.
static int take_order_hints(tsf_ctx *ctx, const FitCall &c, FitArgs *a)
{
    const int order_buf = (ctx->order_n == c.N && !c.theta_in) ? (ctx->order_next ^ 1) : -1;
    if (order_buf >= 0) a->order = ctx->order_dev[order_buf];
    else if (c.grid_order && ctx->opt[TSF_OPT_GRID_ORDER] != 0) a->order = c.grid_order;       // series grouped by shared grid (fit_host_one)
    ctx->order_n = 0;
    return order_buf;
}

// what every quadratic-form launch shares
static QuadArgs quad_args(const FitRun &r, const FitArgs &a)
{
    QuadArgs qa;
    memset(&qa, 0, sizeof(qa));
    qa.f = a; qa.Mg = (const double *)(r.ws + r.l.Mg); qa.rbuf = (double *)(r.ws + r.l.rbuf);
    qa.counter = (int *)(r.ws + r.l.counter); qa.P4 = r.p.qp.P4;
    return qa;
}

static int launch_route_newton_quad(const FitRun &r, const FitArgs &a, int *lrc)
{
    tsf_ctx *ctx = r.ctx;
    const DevSpec &hs = r.hs;
    hipStream_t st = r.c->stream;
    QuadArgs qa = quad_args(r, a);
    qa.Mslot = (double *)(r.ws + r.l.Mslot);
    if (r.c->aligned && !(ctx->opt[TSF_OPT_DEBUG_ASYNC_SCRATCH] > 0 && (ctx->opt[TSF_OPT_DEBUG_ASYNC_SCRATCH] & 1))) {
        const size_t need = newton_batch_scratch_bytes(hs.KP, fit_P(hs.n_cp, hs.K) | 1, r.c->N, r.p.NTmax, ctx->n_cu, ctx->opt);
        if (need > ctx->nb_ws_bytes) {
            if (ctx->nb_ws) { HIP_TRY(ctx, hipFree(ctx->nb_ws)); ctx->nb_ws = nullptr; ctx->nb_ws_bytes = 0; }
            if (hipMalloc(&ctx->nb_ws, need) == hipSuccess) ctx->nb_ws_bytes = need;
            else { ctx->nb_ws = nullptr; (void)hipGetLastError(); }       // no room: the one-series-per-wave kernel
        }
        qa.nb_buf = ctx->nb_ws; qa.nb_bytes = ctx->nb_ws_bytes;
    }
    HIP_TRY(ctx, hipMemsetAsync(qa.counter, 0, sizeof(int), st));
    *lrc = launch_newton_quad(hs.KP, r.p.qp, qa, (double *)(r.ws + r.l.Mg), fit_P(hs.n_cp, hs.K) | 1, ctx->n_cu, st);
    // (-1: this shape does not fit the quadratic-form Newton kernel's LDS -- the residual-form kernel has no such limit)
    if (*lrc == -1) *lrc = pick_newton_launch(hs.growth, r.mode)(hs.KP, a, fit_P(hs.n_cp, hs.K), st);
    return 0;
}

static int launch_route_quad(const FitRun &r, const FitArgs &a, int *lrc, bool *map_done)
{
    tsf_ctx *ctx = r.ctx;
    const tsf_spec *spec = r.spec;
    const DevSpec &hs = r.hs;
    const FitPlan &p = r.p;
    hipStream_t st = r.c->stream;
    QuadArgs qa = quad_args(r, a);
    qa.Mslot = (double *)(r.ws + r.l.Mslot);
    qa.recenter_every = spec->recenter_every; qa.recenter_ratio = spec->recenter_ratio;
    qa.Mpre = p.quad_pre ? qa.Mg : nullptr; qa.n_pre = p.quad_pre;
    qa.gram_harm = p.gram_harm; qa.resid_harm = p.resid_harm;
    HIP_TRY(ctx, hipMemsetAsync(qa.counter, 0, sizeof(int), st));
    *lrc = -1;
    if (spec->converge == TSF_CONVERGE_MAP && p.qp.PPL == 1 && ctx->opt[TSF_OPT_MAP_DIRECT] != 0) {
        // converge = MAP where the posterior is a quadratic form in everything but sigma: the estimate itself by
        // alternating exact minimisations (tsf_map_quad.h) -- no L-BFGS trajectory, no continuation
        qa.f.map_max_iter = spec->map_max_iter; qa.f.map_tol = spec->map_tol;
        *lrc = launch_map_quad(hs.KP, p.qp, qa, (double *)(r.ws + r.l.Mg), fit_P(hs.n_cp, hs.K) | 1, st);
        if (*lrc == 0) *map_done = true;
    }
    if (*lrc == -1) *lrc = launch_quad(hs.KP, p.qp, qa, (double *)(r.ws + r.l.Mg), st);
    return 0;
}

static int launch_route_mfma(const FitRun &r, const FitArgs &a, int *lrc)
{
    tsf_ctx *ctx = r.ctx;
    const DevSpec &hs = r.hs;
    const MfmaPlan &mp = r.p.mp;
    const WsLayout &l = r.l;
    char *ws = r.ws;
    hipStream_t st = r.c->stream;
    MfmaTabs mt;
    memset(&mt, 0, sizeof(mt));
    int *flags = (int *)(ws + l.counter);        // [0] work queue head, [1] changepoint-row overflow
    HIP_TRY(ctx, hipMemsetAsync(flags, 0, 2 * sizeof(int), st));
    mt.XF = (const double *)(ws + l.mXF); mt.XB = (const double *)(ws + l.mXB);
    mt.XT = (const double *)(ws + l.mXT); mt.tq = (const double *)(ws + l.mtq);
    mt.cq = (const uint16_t *)(ws + l.mcq); mt.cpof = (const int8_t *)(ws + l.mcpof);
    mt.yq = (const double *)(ws + l.myq); mt.hist = (double *)(ws + l.mhist);
    mt.counter = flags; mt.overflow = flags + 1;
    mt.NG = mp.NG; mt.KF = mp.KF; mt.NCB = mp.NCB; mt.rr0 = mp.rr0; mt.run_if_overflow = 0;
    *lrc = launch_mfma_layout(a, hs.KP, mt, (double *)(ws + l.mXF), (double *)(ws + l.mXB),
                              (double *)(ws + l.mXT), (double *)(ws + l.mtq), (uint16_t *)(ws + l.mcq),
                              (int8_t *)(ws + l.mcpof), (double *)(ws + l.myq), flags + 1, st);
    if (*lrc == 0) {
        if (ctx->profiling) HIP_TRY(ctx, hipEventRecord(ctx->ev0[r.slot], st));   // the fit kernel proper
        *lrc = launch_mfma(hs.KP, hs.growth, r.mode, a, mt, mp.blocks, st);
    }
    if (*lrc == 0) {
        // fallback, decided on the device: runs only if the layout kernel found a chunk with more
        // changepoint rows than the trend block holds (long runs of equal timestamps)
        FitArgs fb = a;
        fb.run_flag = flags + 1; fb.run_if = 1;
        *lrc = pick_launch(hs.growth, r.mode)(hs.KP, fb, 0, st);
    }
    return 0;
}

// the one-wave residual kernel (a fit, or tsf_eval's single evaluation) with its cooperative tail
static int launch_route_wave(const FitRun &r, FitArgs &a, int *lrc)
{
    tsf_ctx *ctx = r.ctx;
    const FitPlan &p = r.p;
    hipStream_t st = r.c->stream;
    if (p.coop) {
        a.coop_ctl = (int *)(r.ws + r.l.counter);
        a.coop_list = (int32_t *)(r.ws + r.l.clist);
        a.coop_slots = (double *)(r.ws + r.l.cslots);
        a.coop_max = p.coop_slots; a.coop_stride = p.coop_stride;
        a.coop_after = p.coop_after;
        a.coop_blocks = ctx->n_cu;
        {
            // Hand-over point of the tail rule: the one-wave kernel's waves run alone on their SIMDs by then (13.6 us per
            // evaluation) and a cooperative workgroup needs 5.05: up to ~2.7 fits per CU the cooperative kernel has
            // the higher aggregate rate even though they queue for its workgroups.  Default 2 per CU.
            const int pct = ctx->opt[TSF_OPT_COOP_TAIL] > 0 ? ctx->opt[TSF_OPT_COOP_TAIL] : 200;
            a.coop_tail_at = (int)((int64_t)ctx->n_cu * (pct > 400 ? 400 : pct) / 100);
            if (a.coop_tail_at < 1) a.coop_tail_at = 1;
        }
        HIP_TRY(ctx, hipMemsetAsync(a.coop_ctl, 0, 4 * sizeof(int), st));
    }
    *lrc = pick_launch(r.hs.growth, r.mode)(r.hs.KP, a, r.c->theta_in != nullptr, st);
    return 0;
}

// the planned route's kernels; *lrc: the launch function's code, *map_done: the route computed the MAP estimate itself
static int launch_route(const FitRun &r, FitArgs &a, int *lrc, bool *map_done)
{
    const DevSpec &hs = r.hs;
    hipStream_t st = r.c->stream;
    switch (r.p.route) {
    case TSF_ROUTE_NEWTON_QUAD:
        return launch_route_newton_quad(r, a, lrc);
    case TSF_ROUTE_NEWTON:
        *lrc = pick_newton_launch(hs.growth, r.mode)(hs.KP, a, fit_P(hs.n_cp, hs.K), st);
        return 0;
    case TSF_ROUTE_QUAD_EVAL: {
        QuadArgs qa = quad_args(r, a);
        qa.resid_harm = r.p.resid_harm;
        *lrc = launch_eval_quad(hs.KP, r.p.qp, qa, (double *)(r.ws + r.l.Mg), r.c->theta_ref, st);
        return 0;
    }
    case TSF_ROUTE_QUAD_LBFGS:
        return launch_route_quad(r, a, lrc, map_done);
    case TSF_ROUTE_MFMA:
        return launch_route_mfma(r, a, lrc);
    default:
        return launch_route_wave(r, a, lrc);
    }
}

// converge = MAP: from where the optimiser's own tests stopped every fit on to the maximum a posteriori estimate
// (tsf_map_kernels.h), on the same stream behind whichever kernels ran the fit; inside the profiled interval
static int launch_map_continuation(const FitRun &r, FitArgs &a)
{
    const FitPlan &p = r.p;
    a.map_max_iter = r.spec->map_max_iter; a.map_tol = r.spec->map_tol; a.map_harm = p.map_harm;
    if (p.map_harm && p.lat_U == 0) a.Bw = (const double *)(r.ws + r.l.Bw);
    if (p.map_harm && p.lat_U > 0) a.Bu = (const double *)(r.ws + r.l.Bw);
    a.order = nullptr; a.run_flag = nullptr;
    return pick_map_launch(r.hs.growth, r.mode)(r.hs.KP, a, r.c->stream);
}

// Common driver: setup kernels + fit (or eval-only) kernel on device pointers.  plan_fit (tsf_fit_plan.h) decides
// what runs; the steps below only carry it out.
static int run_fit(tsf_ctx *ctx, const tsf_spec *spec, const FitCall &c, tsf_fit_out *out)
{
    if (!ctx) return -1;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    FitRun r;
    r.ctx = ctx; r.spec = spec; r.c = &c;
    int rc = fit_validate(ctx, spec, c, out, &r.hs, &r.mode);
    if (rc) return rc;
    const MemQuery mem = {ctx_mem_avail, ctx};
    r.p = plan_fit(r.hs, r.mode, spec, fit_shape(c), ctx->opt, ctx->n_cu, mem);
    const FitPlan &p = r.p;
    ctx->last_plan = p;
    if (p.rc) return fail(ctx, fit_plan_message(p.err));
    // the slot records of the several-series-per-wave Newton kernel are cached between Newton calls, but at most
    // TSF_NB_KEEP bytes of them outlive a call that does not use them
    if (!(p.route == TSF_ROUTE_NEWTON_QUAD && c.aligned) && ctx->nb_ws_bytes > TSF_NB_KEEP) {
        HIP_TRY(ctx, hipFree(ctx->nb_ws));
        ctx->nb_ws = nullptr; ctx->nb_ws_bytes = 0;
    }
    r.l = ws_layout(c.N, p, r.hs.KP);
    rc = ensure_ws(ctx, r.l.total, c.N, p.NTmax, !c.aligned);
    if (rc) return rc;
    r.ws = (char *)ctx->ws;
    r.grid_of = p.shared_grids ? c.grid_of : nullptr;
    r.grid_rows = p.shared_grids ? c.grid_rows : nullptr;
    rc = fit_setup(r);
    if (rc) return rc;
    FitArgs a = fit_args(r, out);
    ctx->last_sp_flag = a.sp_flag;
    const int order_buf = take_order_hints(ctx, c, &a);
    r.slot = (int)(ctx->ev_count % TSF_PROFILE_RING);
    if (ctx->profiling) HIP_TRY(ctx, hipEventRecord(ctx->ev0[r.slot], c.stream));
    int lrc = 0;
    bool map_done = false;
    rc = launch_route(r, a, &lrc, &map_done);
    if (rc) return rc;
    if (lrc == 0 && spec->converge == TSF_CONVERGE_MAP && c.theta_in == nullptr && !map_done) lrc = launch_map_continuation(r, a);
    if (ctx->profiling) { HIP_TRY(ctx, hipEventRecord(ctx->ev1[r.slot], c.stream)); ctx->ev_count++; }
    if (order_buf >= 0) {       // the launch above reads the hint buffer: tsf_set_cost_hints waits for this before rewriting it
        if (!ctx->order_ev[order_buf]) HIP_TRY(ctx, hipEventCreateWithFlags(&ctx->order_ev[order_buf], hipEventDisableTiming));
        HIP_TRY(ctx, hipEventRecord(ctx->order_ev[order_buf], c.stream));
        ctx->order_busy[order_buf] = 1;
    }
    if (lrc != 0) {
        ctx->err = std::string("kernel launch failed: ") + (lrc > 0 ? hipGetErrorString((hipError_t)lrc) : "no kernel for this shape");
        return -2;
    }
    return 0;
}

extern "C" int tsf_fit_plan_info_size(void) { return (int)sizeof(tsf_fit_plan_info); }
extern "C" const char *tsf_fit_plan_error(int32_t err) { return fit_plan_message(err); }

static int64_t given_mem_avail(void *arg) { return *(const int64_t *)arg; }

extern "C" int tsf_fit_plan(const tsf_spec *spec, const tsf_fit_shape *shape, const int *opt, int n_cu, int64_t mem_avail,
                            tsf_fit_plan_info *out)
{
    if (!spec || !shape || !opt || !out || shape->N <= 0 || n_cu < 1) return -1;
    memset(out, 0, sizeof(*out));
    DevSpec hs;
    int mode = 0;
    int rc = build_devspec(nullptr, spec, &hs, &mode);
    if (rc) return rc;
    const MemQuery mem = {given_mem_avail, &mem_avail};
    const FitPlan p = plan_fit(hs, mode, spec, *shape, opt, n_cu, mem);
    fit_plan_info(p, out);
    return p.rc;
}

extern "C" int tsf_last_fit_plan(const tsf_ctx *ctx, tsf_fit_plan_info *out)
{
    if (!ctx || !out) return -1;
    fit_plan_info(ctx->last_plan, out);
    return 0;
}

static bool fit_out_complete(const tsf_fit_out &f)
{
    return f.theta && f.y_scale && f.fval && f.status && f.n_iter && f.n_eval && f.grid;
}

extern "C" int tsf_fit_aligned_dev(tsf_ctx *ctx, const tsf_spec *spec, int64_t N, int32_t T,
                                   const int64_t *ds, const void *y, int32_t y_dtype,
                                   const double *floor_, const double *cap, const double *extra,
                                   tsf_fit_out *out, void *stream)
{
    if (!ctx) return -1;
    if (!out || !fit_out_complete(*out)) return fail(ctx, "tsf_fit_out has NULL members");
    FitCall c = {};
    c.N = N; c.aligned = 1; c.T = T; c.max_T = T;
    c.ds = ds; c.y = y; c.y_dtype = y_dtype; c.floor = floor_; c.cap = cap; c.extra = extra;
    c.stream = (hipStream_t)stream;
    return run_fit(ctx, spec, c, out);
}

extern "C" int tsf_fit_ragged_dev(tsf_ctx *ctx, const tsf_spec *spec, int64_t N,
                                  const int64_t *offsets, int64_t total_rows, int32_t max_T,
                                  const int64_t *ds, const void *y, int32_t y_dtype,
                                  const double *floor_, const double *cap, const double *extra,
                                  tsf_fit_out *out, void *stream)
{
    if (!ctx) return -1;
    if (!offsets) return fail(ctx, "offsets is NULL");
    if (!out || !fit_out_complete(*out)) return fail(ctx, "tsf_fit_out has NULL members");
    FitCall c = {};
    c.N = N; c.offsets = offsets; c.total_rows = total_rows; c.max_T = max_T;
    c.ds = ds; c.y = y; c.y_dtype = y_dtype; c.floor = floor_; c.cap = cap; c.extra = extra;
    c.stream = (hipStream_t)stream;
    return run_fit(ctx, spec, c, out);
}

// ---- host-pointer wrappers --------------------------------------------------------------------

namespace {
// Device buffers of the host-pointer entry points come from a small per-process cache
// (power-of-two size classes, per device, at most 2 GiB kept): the DataFrame layer calls these
// entry points once per group of series, and a hipMalloc + hipFree (which synchronises the
// device) per buffer per call costs more than a small group's fit.
struct PoolEntry { void *p; size_t bytes; int device; };
std::mutex g_pool_mu;
std::vector<PoolEntry> g_pool;
size_t g_pool_bytes = 0;
constexpr size_t POOL_LIMIT = (size_t)2 << 30;

size_t pool_class(size_t n)
{
    size_t c = 256;
    while (c < n) c <<= 1;
    return c;
}

void pool_trim(int device)
{
    std::lock_guard<std::mutex> lk(g_pool_mu);
    for (size_t i = 0; i < g_pool.size();) {
        if (g_pool[i].device == device) {
            hipFree(g_pool[i].p);
            g_pool_bytes -= g_pool[i].bytes;
            g_pool[i] = g_pool.back();
            g_pool.pop_back();
        } else {
            ++i;
        }
    }
}

struct DevBuf {
    void *p = nullptr;
    size_t bytes = 0;
    int device = 0;
    DevBuf() = default;
    DevBuf(const DevBuf &) = delete;            // (the destructor hands p to the pool: one owner)
    DevBuf &operator=(const DevBuf &) = delete;
    ~DevBuf()
    {
        if (!p) return;
        std::lock_guard<std::mutex> lk(g_pool_mu);
        if (g_pool_bytes + bytes <= POOL_LIMIT) { g_pool.push_back({p, bytes, device}); g_pool_bytes += bytes; }
        else hipFree(p);
    }
    hipError_t alloc(size_t n)
    {
        bytes = pool_class(n ? n : 8);
        hipGetDevice(&device);
        {
            std::lock_guard<std::mutex> lk(g_pool_mu);
            for (size_t i = 0; i < g_pool.size(); ++i) {
                if (g_pool[i].device == device && g_pool[i].bytes == bytes) {
                    p = g_pool[i].p;
                    g_pool_bytes -= bytes;
                    g_pool[i] = g_pool.back();
                    g_pool.pop_back();
                    return hipSuccess;
                }
            }
        }
        return hipMalloc(&p, bytes);
    }
    // alloc + the n bytes at the host pointer src copied in (n = 0: the buffer alone, nothing is copied)
    hipError_t put(const void *src, size_t n)
    {
        const hipError_t e = alloc(n);
        return e != hipSuccess || n == 0 ? e : hipMemcpy(p, src, n, hipMemcpyHostToDevice);
    }
    template <class T> T *as() const { return (T *)p; }
};

// The optional outputs of a host entry on the device and their way back: per output one `want` (the host pointer and its
// size, said once), then one `fetch` behind the entry's synchronisation.  It lives in the entry's scope: the buffers go
// back to the pool when it does.  (A deque: it never moves the DevBufs it holds.)
struct HostOuts {
    struct Pair { void *host; const void *dev; size_t bytes; };
    std::deque<DevBuf> bufs;
    std::vector<Pair> pairs;
    hipError_t err = hipSuccess;        // the first failed allocation: every later want is null, ready and fetch report it

    // a pooled device buffer of `bytes` for the output the caller wants at `host`; null, and no buffer, where host is null
    template <class T> T *want(T *host, size_t bytes)
    {
        if (!host || err != hipSuccess) return nullptr;
        bufs.emplace_back();
        if ((err = bufs.back().alloc(bytes)) != hipSuccess) return nullptr;
        return adopt(host, bufs.back().as<T>(), bytes);
    }
    // an output that is on the device already: dev is copied to host with the others
    template <class T> T *adopt(T *host, T *dev, size_t bytes)
    {
        if (!host) return nullptr;
        pairs.push_back({host, dev, bytes});
        return dev;
    }
    // after the last want, before anything is launched
    int ready(tsf_ctx *ctx) const
    {
        if (err == hipSuccess) return 0;
        ctx->err = std::string("HostOuts::want: ") + hipGetErrorString(err);
        return -2;
    }
    // every output asked for, in the order asked for, to its host pointer
    int fetch(tsf_ctx *ctx) const
    {
        if (int rc = ready(ctx)) return rc;
        for (const Pair &o : pairs)
            if (o.bytes) HIP_TRY(ctx, hipMemcpy(o.host, o.dev, o.bytes, hipMemcpyDeviceToHost));
        return 0;
    }
};

// Device memory a handle owns for its lifetime: plain hipMalloc / hipFree of the exact size (not the pool, whose
// power-of-two classes would nearly double a large buffer), zero-filled where asked.  Reads as the pointer it holds.
template <class T>
struct OwnedDev {
    T *p = nullptr;
    OwnedDev() = default;
    OwnedDev(const OwnedDev &) = delete;
    OwnedDev &operator=(const OwnedDev &) = delete;
    ~OwnedDev() { if (p) (void)hipFree(p); }
    hipError_t alloc(size_t n, bool zero = false)
    {
        const hipError_t e = hipMalloc((void **)&p, sizeof(T) * n);
        return e != hipSuccess || !zero ? e : hipMemset(p, 0, sizeof(T) * n);
    }
    void swap(OwnedDev &o) { std::swap(p, o.p); }
    operator T *() const { return p; }
};

// the first HIP error of a sequence of calls ends the function that holds them with that error
#define HIP_OK(expr)                                                                         \
    do {                                                                                     \
        const hipError_t e_ = (expr);                                                        \
        if (e_ != hipSuccess) return e_;                                                     \
    } while (0)

size_t ysize(int dt) { return dt == TSF_Y_F64 ? 8 : 4; }

// What a DevFitOut holds when alloc returns: the pool does not clear its buffers, and what no launch writes the caller
// reads, so each site names the contents it relies on.
enum FitOutInit {
    FIT_OUT_RAW,        // nothing: a launch writes every element before it is read (every fold of a plan is fitted)
    FIT_OUT_LAUNCH,     // status, n_iter, n_eval and the grids zero: the outputs of one fit launch (run_fit)
    FIT_OUT_UNFITTED    // everything zero, status TSF_ST_TOO_FEW: a destination no launch may reach (a series without rows)
};

// The device side of a tsf_fit_out over n series: a fit launch's outputs, or the destination the launches of a panel job
// scatter to.  The one place a tsf_fit_out of device pointers is put together (view) and copied back (download).
struct DevFitOut {
    DevBuf theta, y_scale, fval, status, n_iter, n_eval, grid;
    size_t n = 0, stride = 0;

    int alloc(tsf_ctx *ctx, int64_t n_series, int theta_stride, int64_t n_grids, FitOutInit init)
    {
        n = (size_t)n_series; stride = (size_t)theta_stride;
        const size_t grid_bytes = sizeof(tsf_grid_info) * (size_t)n_grids;
        HIP_TRY(ctx, theta.alloc(8 * n * stride)); HIP_TRY(ctx, y_scale.alloc(8 * n)); HIP_TRY(ctx, fval.alloc(8 * n));
        HIP_TRY(ctx, status.alloc(4 * n)); HIP_TRY(ctx, n_iter.alloc(4 * n)); HIP_TRY(ctx, n_eval.alloc(4 * n));
        HIP_TRY(ctx, grid.alloc(grid_bytes));
        if (init == FIT_OUT_RAW) return 0;
        if (init == FIT_OUT_UNFITTED) {
            HIP_TRY(ctx, hipMemset(theta.p, 0, 8 * n * stride)); HIP_TRY(ctx, hipMemset(y_scale.p, 0, 8 * n));
            HIP_TRY(ctx, hipMemset(fval.p, 0, 8 * n));
        } else {
            HIP_TRY(ctx, hipMemset(status.p, 0, 4 * n));
        }
        HIP_TRY(ctx, hipMemset(n_iter.p, 0, 4 * n)); HIP_TRY(ctx, hipMemset(n_eval.p, 0, 4 * n));
        HIP_TRY(ctx, hipMemset(grid.p, 0, grid_bytes));
        if (init == FIT_OUT_UNFITTED) {
            const std::vector<int32_t> st(n, TSF_ST_TOO_FEW);
            HIP_TRY(ctx, hipMemcpy(status.p, st.data(), 4 * n, hipMemcpyHostToDevice));
        }
        return 0;
    }
    tsf_fit_out view() const
    {
        tsf_fit_out o;
        o.theta = theta.as<double>(); o.y_scale = y_scale.as<double>(); o.fval = fval.as<double>();
        o.status = status.as<int32_t>(); o.n_iter = n_iter.as<int32_t>(); o.n_eval = n_eval.as<int32_t>();
        o.grid = grid.as<tsf_grid_info>();
        return o;
    }
    // to the host arrays of `out`, the first n_grids grids (an aligned fit has one)
    int download(tsf_ctx *ctx, const tsf_fit_out &out, int64_t n_grids) const
    {
        HIP_TRY(ctx, hipMemcpy(out.theta, theta.p, 8 * n * stride, hipMemcpyDeviceToHost));
        HIP_TRY(ctx, hipMemcpy(out.y_scale, y_scale.p, 8 * n, hipMemcpyDeviceToHost));
        HIP_TRY(ctx, hipMemcpy(out.fval, fval.p, 8 * n, hipMemcpyDeviceToHost));
        HIP_TRY(ctx, hipMemcpy(out.status, status.p, 4 * n, hipMemcpyDeviceToHost));
        HIP_TRY(ctx, hipMemcpy(out.n_iter, n_iter.p, 4 * n, hipMemcpyDeviceToHost));
        HIP_TRY(ctx, hipMemcpy(out.n_eval, n_eval.p, 4 * n, hipMemcpyDeviceToHost));
        HIP_TRY(ctx, hipMemcpy(out.grid, grid.p, sizeof(tsf_grid_info) * (size_t)n_grids, hipMemcpyDeviceToHost));
        return 0;
    }
};
}  // namespace

// Which of N timestamp vectors -- vector n = ds[start[n] .. start[n] + len[n]) -- are IDENTICAL (hash of the bytes, then
// memcmp against the class's first member): gof[n] = class of vector n, classes numbered in order of their first member,
// reps[k] = the first member of class k.  The one producer of the calendar classes of a ragged fit (fit_host_one) and of
// the folds of a ragged cross-validation (tsf_cross_validate, where the vectors are prefixes of the caller's series).
static void calendar_classes(const int64_t *ds, const int64_t *start, const int64_t *len, int64_t N,
                             std::vector<int32_t> *gof_out, std::vector<int64_t> *reps_out)
{
    struct Key { int64_t len; uint64_t h; int64_t n; };
    std::vector<Key> keys((size_t)N);
    {
        int hw = (int)std::thread::hardware_concurrency();
        const int nt = hw < 1 ? 1 : (hw > 16 ? 16 : hw);
        std::atomic<int64_t> next(0);
        auto work = [&]() {
            for (;;) {
                const int64_t b = next.fetch_add(256);
                if (b >= N) break;
                for (int64_t n = b; n < N && n < b + 256; ++n) {
                    const int64_t l = len[n];
                    const uint64_t *p = (const uint64_t *)(ds + start[n]);
                    uint64_t h = 0x9e3779b97f4a7c15ull ^ (uint64_t)l;
                    for (int64_t i = 0; i < l; ++i) { h ^= p[i]; h *= 0xff51afd7ed558ccdull; h ^= h >> 32; }
                    keys[(size_t)n] = Key{l, h, n};
                }
            }
        };
        if (nt <= 1 || N < 1024) work();
        else {
            std::vector<std::thread> th;
            for (int i = 0; i < nt; ++i) th.emplace_back(work);
            for (auto &x : th) x.join();
        }
    }
    std::sort(keys.begin(), keys.end(), [](const Key &a, const Key &b) {
        return a.len != b.len ? a.len < b.len : (a.h != b.h ? a.h < b.h : a.n < b.n);
    });
    std::vector<int64_t> rep((size_t)N);            // first member of the class of vector n
    for (size_t i = 0; i < keys.size();) {
        size_t j = i;
        while (j < keys.size() && keys[j].len == keys[i].len && keys[j].h == keys[i].h) ++j;
        // members of one (length, hash) run: classes by memcmp against the representatives found so far
        std::vector<int64_t> reps;
        for (size_t k = i; k < j; ++k) {
            const int64_t n = keys[k].n;
            int64_t r = -1;
            for (int64_t c : reps)
                if (memcmp(ds + start[c], ds + start[n], (size_t)keys[k].len * 8) == 0) { r = c; break; }
            if (r < 0) { reps.push_back(n); r = n; }
            rep[(size_t)n] = r;
        }
        i = j;
    }
    std::vector<int32_t> &gof = *gof_out, id_of((size_t)N, -1);
    gof.assign((size_t)N, 0);
    reps_out->clear();
    for (int64_t n = 0; n < N; ++n) {
        const int64_t r = rep[(size_t)n];
        if (id_of[(size_t)r] < 0) {
            id_of[(size_t)r] = (int32_t)reps_out->size();
            reps_out->push_back(r);
        }
        gof[(size_t)n] = id_of[(size_t)r];
    }
}

// The order in which a launch over calendar classes starts its series: grouped by grid, and the grouped list cut into 8
// segments dealt out one position each in turn -- block b of a one-wave launch runs on XCD b % 8 (observed,
// MI355X_MICROARCH: for speed only), so every XCD works its way through ITS segment and its 4 MB of L2 hold the two or
// three grids its resident blocks are on, instead of a share of all of them (10 000 series on 91 grids, the reference's
// model: 205 -> 172 ms, tools/bench_ragged.py).  Used when the caller gave no cost hints; results do not depend on the
// order.
static void calendar_start_order(const std::vector<int32_t> &gof, int64_t n_distinct, std::vector<int32_t> *ord_out)
{
    const int64_t N = (int64_t)gof.size();
    std::vector<int32_t> byg((size_t)N), &ord = *ord_out;
    ord.assign((size_t)N, 0);
    std::vector<int64_t> start((size_t)n_distinct + 1, 0);
    for (int64_t n = 0; n < N; ++n) start[(size_t)gof[(size_t)n] + 1]++;
    for (int64_t g = 0; g < n_distinct; ++g) start[(size_t)g + 1] += start[(size_t)g];
    for (int64_t n = 0; n < N; ++n) byg[(size_t)start[(size_t)gof[(size_t)n]]++] = (int32_t)n;
    const int64_t seg = (N + 7) / 8;
    int64_t q = 0;
    for (int64_t i = 0; i < seg; ++i)
        for (int x = 0; x < 8; ++x) { const int64_t k = (int64_t)x * seg + i; if (k < N) ord[(size_t)q++] = byg[(size_t)k]; }
}

// The shared-calendar tables of a ragged launch over gof.size() series on the classes of calendar_classes: gof (the
// class of every series), the rows (first, count) of each class's first member reps[k] in the launch's panel (off: its
// offsets) and the start order.  *n_distinct = the number of classes, or 0 -- nothing uploaded, a grid per series --
// where no two series share a calendar.  The one producer of FitCall::grid_of / grid_rows / grid_order.
static int upload_calendar_tables(tsf_ctx *ctx, const std::vector<int32_t> &gof, const std::vector<int64_t> &reps,
                                  const int64_t *off, DevBuf *d_gof, DevBuf *d_grows, DevBuf *d_gord, int64_t *n_distinct)
{
    *n_distinct = 0;
    if (reps.size() >= gof.size()) return 0;
    std::vector<int64_t> grows;
    for (int64_t r : reps) { grows.push_back(off[r]); grows.push_back(off[r + 1] - off[r]); }
    std::vector<int32_t> ord;
    calendar_start_order(gof, (int64_t)reps.size(), &ord);
    HIP_TRY(ctx, d_gof->put(gof.data(), 4 * gof.size()));
    HIP_TRY(ctx, d_grows->put(grows.data(), 8 * grows.size()));
    HIP_TRY(ctx, d_gord->put(ord.data(), 4 * ord.size()));
    *n_distinct = (int64_t)reps.size();
    return 0;
}

static int fit_host_one(tsf_ctx *ctx, const tsf_spec *spec, int64_t N, int aligned, int32_t T,
                        const int64_t *offsets, const int64_t *ds, const void *y, int32_t y_dtype,
                        const double *floor_, const double *cap, const double *extra,
                        tsf_fit_out *out, const double *theta_in, double *f_out, double *grad_out,
                        const double *theta_ref = nullptr)
{
    if (!ctx) return -1;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (N <= 0) return fail(ctx, "N must be > 0");
    if (!spec) return fail(ctx, "spec is NULL");
    if (y_dtype < TSF_Y_F64 || y_dtype > TSF_Y_I32) return fail(ctx, "bad y_dtype");
    const int stride = tsf_theta_stride(spec);
    int64_t total = 0;
    int32_t max_T = 0;
    if (aligned) {
        total = (int64_t)N * T; max_T = T;
    } else {
        if (!offsets) return fail(ctx, "offsets is NULL");
        total = offsets[N] - offsets[0];
        if (offsets[0] != 0) return fail(ctx, "offsets[0] must be 0");
        for (int64_t n = 0; n < N; ++n) {
            const int64_t len = offsets[n + 1] - offsets[n];
            if (len < 0 || len > (int64_t)TSF_MAX_T) return fail(ctx, "series length out of range (0 .. TSF_MAX_T rows)");
            if (len > max_T) max_T = (int32_t)len;
        }
    }
    if (max_T < 1) return fail(ctx, "no rows");
    if (max_T > TSF_MAX_T) return fail(ctx, "series too long (TSF_MAX_T rows per series)");
    const int64_t n_ds = aligned ? T : total;
    const int64_t n_grids = aligned ? 1 : N;
    // TSF_HOST_TIMING=1 (dev): wall-clock of the phases of this entry point on stderr
    static const bool host_timing = getenv("TSF_HOST_TIMING") != nullptr;
    auto now = [] { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); };
    const double t_start = host_timing ? now() : 0.0;
    double t_h2d = 0.0, t_fit = 0.0;
    DevBuf d_ds, d_y, d_off, d_floor, d_cap, d_extra, d_thin, d_grad, d_thref;
    HIP_TRY(ctx, d_ds.put(ds, 8 * n_ds));
    HIP_TRY(ctx, d_y.put(y, ysize(y_dtype) * total));
    if (!aligned) HIP_TRY(ctx, d_off.put(offsets, 8 * (N + 1)));
    if (floor_) HIP_TRY(ctx, d_floor.put(floor_, 8 * N));
    if (cap) HIP_TRY(ctx, d_cap.put(cap, 8 * N));
    if (spec->n_extra > 0) {
        if (!extra) return fail(ctx, "extra columns declared but extra is NULL");
        HIP_TRY(ctx, d_extra.put(extra, 8 * (size_t)spec->n_extra * n_ds));
    }
    DevFitOut fo;
    if (int rc = fo.alloc(ctx, N, stride, n_grids, FIT_OUT_LAUNCH)) return rc;
    tsf_fit_out dout = fo.view();
    if (theta_in) {
        HIP_TRY(ctx, d_thin.put(theta_in, 8 * (size_t)N * stride));
        HIP_TRY(ctx, d_grad.alloc(8 * (size_t)N * stride));
        if (theta_ref) HIP_TRY(ctx, d_thref.put(theta_ref, 8 * (size_t)N * stride));
    }
    // ragged panel: do all timestamps lie on one lattice base + u*step (the usual case: one
    // sampling grid, different start dates / lengths)?  Then the design rows are computed once
    // for the lattice and shared by every series instead of being stored per series.
    int64_t lat_base = 0, lat_step = 0, lat_U = 0;
    if (!aligned && !theta_in && spec->n_extra == 0 && total > 0) {
        int64_t lo = ds[0], hi = ds[0];
        for (int64_t i = 1; i < total; ++i) { lo = ds[i] < lo ? ds[i] : lo; hi = ds[i] > hi ? ds[i] : hi; }
        uint64_t g = 0;
        for (int64_t i = 0; i < total && g != 1; ++i) {
            uint64_t v = (uint64_t)(ds[i] - lo);
            while (v) { const uint64_t r = g % v; g = v; v = r; }      // gcd(g, v), gcd(0, v) = v
        }
        if (g > 0) {
            const uint64_t U = (uint64_t)(hi - lo) / g + 1;
            if (U <= (uint64_t)1 << 18) { lat_base = lo; lat_step = (int64_t)g; lat_U = (int64_t)U; }
        }
    }
    // ragged panel: which series SHARE a timestamp vector (the usual case: many series observed on a few calendars)?
    // Their grid tables -- scaled time, changepoint segments, the design matrix: 172 KB for two years of daily data --
    // are then built once per distinct vector and shared as on an aligned panel (FitArgs::grid_of), and the
    // quadratic-form path builds Z^T Z once per vector instead of once per series.  Identical vectors only (hash of
    // the bytes, then memcmp against the class's first member); models with explicit columns are left alone (their
    // columns are per row, not per timestamp).  TSF_GRID_SHARE=0 turns it off (tests compare both).
    DevBuf d_gof, d_grows, d_gord;
    int64_t n_distinct = 0;
    if (!aligned && !theta_in && spec->n_extra == 0 && N >= 2 && ctx->opt[TSF_OPT_GRID_SHARE] != 0) {
        std::vector<int64_t> vstart((size_t)N), vlen((size_t)N), reps;
        for (int64_t n = 0; n < N; ++n) { vstart[(size_t)n] = offsets[n]; vlen[(size_t)n] = offsets[n + 1] - offsets[n]; }
        std::vector<int32_t> gof;
        calendar_classes(ds, vstart.data(), vlen.data(), N, &gof, &reps);
        if (int rc = upload_calendar_tables(ctx, gof, reps, offsets, &d_gof, &d_grows, &d_gord, &n_distinct)) return rc;
    }
    if (host_timing) t_h2d = now();
    FitCall c = {};
    c.N = N; c.aligned = aligned; c.T = T; c.offsets = d_off.as<int64_t>(); c.total_rows = total; c.max_T = max_T;
    c.ds = d_ds.as<int64_t>(); c.y = d_y.p; c.y_dtype = y_dtype;
    if (floor_) c.floor = d_floor.as<double>();
    if (cap) c.cap = d_cap.as<double>();
    if (spec->n_extra > 0) c.extra = d_extra.as<double>();
    if (theta_in) { c.theta_in = d_thin.as<double>(); c.grad_out = d_grad.as<double>(); }
    if (theta_in && theta_ref) c.theta_ref = d_thref.as<double>();
    c.lat_base = lat_base; c.lat_step = lat_step; c.lat_U = lat_U;
    if (n_distinct > 0) { c.grid_of = d_gof.as<int32_t>(); c.grid_rows = d_grows.as<int64_t>(); c.grid_order = d_gord.as<int32_t>(); }
    c.n_distinct = n_distinct;
    int rc = run_fit(ctx, spec, c, &dout);
    if (rc) return rc;
    HIP_TRY(ctx, hipDeviceSynchronize());
    if (host_timing) t_fit = now();
    if (theta_in) {
        HIP_TRY(ctx, hipMemcpy(f_out, fo.fval.p, 8 * N, hipMemcpyDeviceToHost));
        HIP_TRY(ctx, hipMemcpy(grad_out, d_grad.p, 8 * (size_t)N * stride, hipMemcpyDeviceToHost));
        return 0;
    }
    rc = fo.download(ctx, *out, n_grids);
    if (rc) return rc;
    if (host_timing)
        fprintf(stderr, "[host-timing] N %lld: alloc + H2D + clears %.3f ms, fit (launch .. device idle) %.3f ms, D2H %.3f ms\n",
                (long long)N, t_h2d - t_start, t_fit - t_h2d, now() - t_fit);
    return 0;
}


// Ragged panels by length.  The device tables of a ragged call are laid out [series][NTmax] (NTmax = steps of
// the LONGEST series of the call: every other series' rows are padding), so one 100 000-row series among
// 10 000 series of 700 rows would ask for ~224 GB.  When the padding is more than half of the layout (and the
// layout is not small anyway) the host entry point therefore cuts the call into length classes -- the longest
// series and every series at least half as long, then the same again for the rest: at most ~11 classes, each
// padded by < 2 x -- and runs one fit call per class on the gathered rows: workspace proportional to the rows
// that exist.  Every series is fitted by itself, so the results do not depend on the grouping (GPU test:
// bit-identical to the single call).  Scheduling hints (tsf_set_cost_hints) given for the whole call are handed to
// the classes series by series.  tsf_fit_ragged_dev (device pointers: the lengths are not on the host) leaves
// this to its caller.
static int fit_host(tsf_ctx *ctx, const tsf_spec *spec, int64_t N, int aligned, int32_t T,
                    const int64_t *offsets, const int64_t *ds, const void *y, int32_t y_dtype,
                    const double *floor_, const double *cap, const double *extra,
                    tsf_fit_out *out, const double *theta_in, double *f_out, double *grad_out,
                    const double *theta_ref = nullptr)
{
    if (!ctx) return -1;
    // (anything fit_host_one rejects -- NULL inputs, offsets that do not start at 0 -- goes to it for the error: the
    // split below indexes ds / y / extra with the caller's offsets; round-4 advice)
    if (aligned || theta_in || !offsets || !spec || N < 2 || y_dtype < TSF_Y_F64 || y_dtype > TSF_Y_I32 ||
        !ds || !y || !out || offsets[0] != 0 || (spec->n_extra > 0 && !extra))
        return fit_host_one(ctx, spec, N, aligned, T, offsets, ds, y, y_dtype, floor_, cap, extra, out, theta_in,
                            f_out, grad_out, theta_ref);
    int64_t sum_nt = 0, nt_max = 0;
    for (int64_t n = 0; n < N; ++n) {
        const int64_t len = offsets[n + 1] - offsets[n];
        if (len < 0 || len > (int64_t)TSF_MAX_T)
            return fit_host_one(ctx, spec, N, aligned, T, offsets, ds, y, y_dtype, floor_, cap, extra, out,
                                theta_in, f_out, grad_out, theta_ref);      // (reports the error)
        const int64_t nt = (len + W - 1) / W;
        sum_nt += nt;
        if (nt > nt_max) nt_max = nt;
    }
    const int force = ctx->opt[TSF_OPT_RAGGED_SPLIT];       // 0: never, 1: whenever the padding rule says so (tests)
    const double padded = (double)N * (double)nt_max;
    const bool small = padded * 512.0 * (3 + tsf_spec_K(spec)) < 256e6;
    if (force == 0 || padded <= 2.0 * (double)sum_nt || (small && force != 1))
        return fit_host_one(ctx, spec, N, aligned, T, offsets, ds, y, y_dtype, floor_, cap, extra, out, theta_in,
                            f_out, grad_out, theta_ref);
    std::vector<int64_t> order((size_t)N);
    for (int64_t n = 0; n < N; ++n) order[(size_t)n] = n;
    std::stable_sort(order.begin(), order.end(), [&](int64_t a, int64_t b) {
        return offsets[a + 1] - offsets[a] > offsets[b + 1] - offsets[b];
    });
    const int stride = tsf_theta_stride(spec);
    const size_t ys = (y_dtype == TSF_Y_F64) ? 8 : 4;
    const int64_t total = offsets[N] - offsets[0];
    // scheduling hints given for this call (tsf_set_cost_hints with N entries): every class gets its series' share
    // (round-4 advice: they used to be dropped on this path without a word)
    std::vector<int32_t> hints;
    if (ctx->order_n == N && (int64_t)ctx->cost_host.size() == N) hints = ctx->cost_host;
    ctx->order_n = 0;
    std::vector<int32_t> hb;
    for (int64_t b0 = 0; b0 < N;) {
        const int64_t top = (offsets[order[(size_t)b0] + 1] - offsets[order[(size_t)b0]] + W - 1) / W;
        int64_t b1 = b0;
        while (b1 < N && 2 * ((offsets[order[(size_t)b1] + 1] - offsets[order[(size_t)b1]] + W - 1) / W) >= top) ++b1;
        const int64_t nb = b1 - b0;
        // the class in the caller's order (stable: neighbours stay neighbours)
        std::vector<int64_t> idx(order.begin() + b0, order.begin() + b1);
        std::sort(idx.begin(), idx.end());
        std::vector<int64_t> off((size_t)nb + 1, 0);
        for (int64_t i = 0; i < nb; ++i) off[(size_t)i + 1] = off[(size_t)i] + (offsets[idx[(size_t)i] + 1] - offsets[idx[(size_t)i]]);
        const int64_t rows = off[(size_t)nb];
        std::vector<int64_t> dsb((size_t)rows);
        std::vector<char> yb((size_t)rows * ys);
        std::vector<double> flb, cpb, exb;
        if (floor_) flb.resize((size_t)nb);
        if (cap) cpb.resize((size_t)nb);
        if (spec->n_extra > 0 && extra) exb.resize((size_t)spec->n_extra * (size_t)rows);
        for (int64_t i = 0; i < nb; ++i) {
            const int64_t n = idx[(size_t)i], r0 = offsets[n], len = offsets[n + 1] - r0;
            if (len > 0) {
                memcpy(dsb.data() + off[(size_t)i], ds + r0, (size_t)len * 8);
                memcpy(yb.data() + (size_t)off[(size_t)i] * ys, (const char *)y + (size_t)r0 * ys, (size_t)len * ys);
                for (int e = 0; e < spec->n_extra && !exb.empty(); ++e)
                    memcpy(exb.data() + (size_t)e * rows + off[(size_t)i], extra + (size_t)e * total + r0, (size_t)len * 8);
            }
            if (floor_) flb[(size_t)i] = floor_[n];
            if (cap) cpb[(size_t)i] = cap[n];
        }
        std::vector<double> th((size_t)nb * stride), ysc((size_t)nb), fv((size_t)nb);
        std::vector<int32_t> st((size_t)nb), it((size_t)nb), ev((size_t)nb);
        std::vector<tsf_grid_info> gr((size_t)nb);
        tsf_fit_out ob;
        ob.theta = th.data(); ob.y_scale = ysc.data(); ob.fval = fv.data(); ob.status = st.data();
        ob.n_iter = it.data(); ob.n_eval = ev.data(); ob.grid = gr.data();
        if (!hints.empty()) {
            hb.resize((size_t)nb);
            for (int64_t i = 0; i < nb; ++i) hb[(size_t)i] = hints[(size_t)idx[(size_t)i]];
            const int hrc = tsf_set_cost_hints(ctx, hb.data(), nb);
            if (hrc) return hrc;
        }
        const int rc = fit_host_one(ctx, spec, nb, 0, 0, off.data(), dsb.data(), yb.data(), y_dtype,
                                    floor_ ? flb.data() : nullptr, cap ? cpb.data() : nullptr,
                                    exb.empty() ? (spec->n_extra > 0 ? extra : nullptr) : exb.data(), &ob, nullptr, nullptr, nullptr);
        if (rc) return rc;
        for (int64_t i = 0; i < nb; ++i) {
            const int64_t n = idx[(size_t)i];
            memcpy(out->theta + (size_t)n * stride, th.data() + (size_t)i * stride, sizeof(double) * stride);
            out->y_scale[n] = ysc[(size_t)i]; out->fval[n] = fv[(size_t)i]; out->status[n] = st[(size_t)i];
            out->n_iter[n] = it[(size_t)i]; out->n_eval[n] = ev[(size_t)i]; out->grid[n] = gr[(size_t)i];
        }
        b0 = b1;
    }
    return 0;
}

extern "C" int tsf_fit_aligned(tsf_ctx *ctx, const tsf_spec *spec, int64_t N, int32_t T,
                               const int64_t *ds, const void *y, int32_t y_dtype,
                               const double *floor_, const double *cap, const double *extra,
                               tsf_fit_out *out)
{
    if (!ctx) return -1;
    if (!ds || !y || !out) return fail(ctx, "NULL input");
    return fit_host(ctx, spec, N, 1, T, nullptr, ds, y, y_dtype, floor_, cap, extra, out, nullptr,
                    nullptr, nullptr);
}

extern "C" int tsf_fit_ragged(tsf_ctx *ctx, const tsf_spec *spec, int64_t N, const int64_t *offsets,
                              const int64_t *ds, const void *y, int32_t y_dtype,
                              const double *floor_, const double *cap, const double *extra,
                              tsf_fit_out *out)
{
    if (!ctx) return -1;
    if (!ds || !y || !out) return fail(ctx, "NULL input");
    return fit_host(ctx, spec, N, 0, 0, offsets, ds, y, y_dtype, floor_, cap, extra, out, nullptr,
                    nullptr, nullptr);
}

extern "C" int tsf_eval(tsf_ctx *ctx, const tsf_spec *spec, int64_t N, int32_t T, const int64_t *ds,
                        const void *y, int32_t y_dtype, const double *floor_, const double *cap,
                        const double *extra, const double *theta, double *f_out, double *grad_out)
{
    if (!ctx) return -1;
    if (!ds || !y || !theta || !f_out || !grad_out) return fail(ctx, "NULL input");
    tsf_fit_out dummy;
    memset(&dummy, 0, sizeof(dummy));
    return fit_host(ctx, spec, N, 1, T, nullptr, ds, y, y_dtype, floor_, cap, extra, &dummy, theta,
                    f_out, grad_out);
}

extern "C" int tsf_eval_quadratic(tsf_ctx *ctx, const tsf_spec *spec, int64_t N, int32_t T, const int64_t *ds,
                                  const void *y, int32_t y_dtype, const double *extra, const double *theta_ref,
                                  const double *theta, double *f_out, double *grad_out)
{
    if (!ctx) return -1;
    if (!ds || !y || !theta || !theta_ref || !f_out || !grad_out) return fail(ctx, "NULL input");
    tsf_fit_out dummy;
    memset(&dummy, 0, sizeof(dummy));
    return fit_host(ctx, spec, N, 1, T, nullptr, ds, y, y_dtype, nullptr, nullptr, extra, &dummy, theta,
                    f_out, grad_out, theta_ref);
}

// ---- predict ----------------------------------------------------------------------------------

// The grids a host-memory predict entry is handed are caller data (model blobs read back from storage):
// checked before anything is copied or launched.  S beyond the spec's n_changepoints would read beta as
// delta; beyond TSF_MAX_S the kernel's LDS segment tables overflow.
// fit_status (tsf_noise_state: one per series, n_grids = 1 or their count N): the grid of a series whose status is
// negative is not read by the kernel and not checked; a shared grid is checked where any series uses it.
static int check_grids(tsf_ctx *ctx, const tsf_spec *spec, const tsf_grid_info *grid, int32_t n_grids,
                       const int32_t *fit_status = nullptr, int64_t N = 0)
{
    if (fit_status && n_grids == 1 && std::none_of(fit_status, fit_status + N, [](int32_t s) { return s >= 0; })) return 0;
    for (int32_t g = 0; g < n_grids; ++g) {
        const tsf_grid_info &gi = grid[g];
        if (fit_status && n_grids != 1 && fit_status[g] < 0) continue;
        const char *why = nullptr;
        if (gi.S < 0) why = "S < 0";
        else if (gi.S > spec->n_changepoints) why = "S > the spec's n_changepoints";
        else if (gi.S > TSF_MAX_S) why = "S > TSF_MAX_S";
        else if (gi.t_scale_ns <= 0) why = "t_scale_ns <= 0";
        if (why) {
            char msg[160];
            snprintf(msg, sizeof(msg), "grid[%d]: %s (S = %d, t_scale_ns = %lld)", (int)g, why, (int)gi.S,
                     (long long)gi.t_scale_ns);
            return fail(ctx, msg);
        }
    }
    return 0;
}

// What a forecast is computed from: the arguments every predict entry shares.  Host pointers in a host entry, device
// pointers behind it (ForecastUpload turns the first into the second) and in a `_dev` entry.
struct ForecastIn {
    int64_t N;
    int32_t H;
    const double *theta, *y_scale;
    const tsf_grid_info *grid;
    int32_t n_grids;
    const int64_t *ds_future;
    int32_t shared_future;
    const double *floor_, *cap, *extra_future;
    const int64_t *series_key;
};

// The opening checks of the predict entries.  outs_ok: the entry's other required pointers are there.  Nothing is
// dereferenced: in a `_dev` entry the arrays are device memory (check_grids is for the host entries).
static int check_forecast_in(tsf_ctx *ctx, const ForecastIn &f, bool outs_ok)
{
    if (f.N <= 0 || f.H <= 0) return fail(ctx, "N and H must be > 0");
    if (!f.theta || !f.y_scale || !f.grid || !f.ds_future || !outs_ok) return fail(ctx, "NULL input");
    if (f.n_grids != 1 && f.n_grids != f.N) return fail(ctx, "n_grids must be 1 or N");
    return 0;
}

// A host entry's inputs in pooled device buffers.  It lives in the entry's scope: the buffers go back to the pool when
// it does, after the entry has copied its results out.
struct ForecastUpload {
    DevBuf th, ys, grid, ds, fl, cap, ex, key;
    ForecastIn dev;

    // ds_on_device: h.ds_future is device memory already (the roll-up's calendar) and is used as it is
    int upload(tsf_ctx *ctx, const tsf_spec *spec, const ForecastIn &h, bool ds_on_device = false)
    {
        if (spec->n_extra > 0 && !h.extra_future) return fail(ctx, "extra_future is NULL");
        const size_t N = (size_t)h.N, nfut = h.shared_future ? (size_t)h.H : N * h.H;
        dev = h;
        if (int rc = put(ctx, &th, h.theta, 8 * N * tsf_theta_stride(spec), &dev.theta)) return rc;
        if (int rc = put(ctx, &ys, h.y_scale, 8 * N, &dev.y_scale)) return rc;
        if (int rc = put(ctx, &grid, h.grid, sizeof(tsf_grid_info) * h.n_grids, &dev.grid)) return rc;
        if (!ds_on_device)
            if (int rc = put(ctx, &ds, h.ds_future, 8 * nfut, &dev.ds_future)) return rc;
        if (int rc = put(ctx, &fl, h.floor_, 8 * N, &dev.floor_)) return rc;
        if (int rc = put(ctx, &cap, h.cap, 8 * N, &dev.cap)) return rc;
        if (int rc = put(ctx, &key, h.series_key, 8 * N, &dev.series_key)) return rc;
        if (spec->n_extra == 0) dev.extra_future = nullptr;
        else if (int rc = put(ctx, &ex, h.extra_future, 8 * (size_t)spec->n_extra * nfut, &dev.extra_future)) return rc;
        return 0;
    }

    // *d = the device copy of the `bytes` at src, or null where src is
    template <class T>
    static int put(tsf_ctx *ctx, DevBuf *b, const T *src, size_t bytes, const T **d)
    {
        *d = nullptr;
        if (!src) return 0;
        HIP_TRY(ctx, b->put(src, bytes));
        *d = b->as<T>();
        return 0;
    }
};

// The spec built and checked against the forecast's inputs (host work alone).
static int forecast_spec(tsf_ctx *ctx, const tsf_spec *spec, const ForecastIn &f, DevSpec *hs)
{
    int mode = 0;
    if (int rc = build_devspec(ctx, spec, hs, &mode)) return rc;
    if (hs->n_extra > 0 && !f.extra_future) return fail(ctx, "extra_future is NULL");
    if (hs->growth == TSF_GROWTH_LOGISTIC && !f.cap) return fail(ctx, "logistic growth needs cap");
    return 0;
}

// What every forecast starts with on the device: forecast_spec, then the spec sent to the context's copy in stream order.
static int forecast_prologue(tsf_ctx *ctx, const tsf_spec *spec, const ForecastIn &f, hipStream_t st, DevSpec *hs)
{
    if (int rc = forecast_spec(ctx, spec, f, hs)) return rc;
    HIP_TRY(ctx, hipMemcpyAsync(ctx->d_spec, hs, sizeof(*hs), hipMemcpyHostToDevice, st));
    return 0;
}

// predict_kernel's arguments for the whole call (launch_predict narrows them to a chunk); the optional outputs
// (yhat_int, trend_out, the per-row pieces) are the caller's to set.
static PredictArgs predict_args(const tsf_ctx *ctx, const tsf_spec *spec, const ForecastIn &f, double *yhat)
{
    PredictArgs p;
    memset(&p, 0, sizeof(p));
    p.sp = ctx->d_spec; p.N = f.N; p.H = f.H; p.theta_stride = tsf_theta_stride(spec);
    p.n_grids = f.n_grids; p.shared_future = f.shared_future; p.theta = f.theta; p.y_scale = f.y_scale;
    p.grid = f.grid; p.ds_future = f.ds_future; p.floor_ = f.floor_; p.cap = f.cap;
    p.extra_future = f.extra_future; p.yhat = yhat;
    return p;
}

// The context's sample scratch (one cached block, like the fit workspace: grown on demand by a plain hipMalloc, which
// waits for the device only on the call that grows it) is at least `need` bytes.
static int ensure_iv_ws(tsf_ctx *ctx, size_t need)
{
    if (ctx->iv_ws_bytes < need) {
        if (ctx->iv_ws) { HIP_TRY(ctx, hipFree(ctx->iv_ws)); ctx->iv_ws = nullptr; ctx->iv_ws_bytes = 0; }
        HIP_TRY(ctx, hipMalloc(&ctx->iv_ws, need));
        ctx->iv_ws_bytes = need;
    }
    return 0;
}

// predict_kernel on the series [n0, n0 + n) of the caller's arrays.  A shared future grid gets its
// design table built first (once per call: tab_ready), in the context's own buffer.
static int launch_predict(tsf_ctx *ctx, const DevSpec &hs, PredictArgs a, int64_t n0, int64_t n, bool *tab_ready,
                          hipStream_t st)
{
    if (a.shared_future) {
        const size_t need = sizeof(double) * (size_t)(hs.K > 0 ? hs.K : 1) * a.H;
        if (ctx->fut_tab_bytes < need) {
            // (grows only: a buffer an earlier call on another stream may still read is never freed here
            // without the device being idle -- hipFree synchronises)
            if (ctx->fut_tab) { HIP_TRY(ctx, hipFree(ctx->fut_tab)); ctx->fut_tab = nullptr; ctx->fut_tab_bytes = 0; }
            HIP_TRY(ctx, hipMalloc((void **)&ctx->fut_tab, need));
            ctx->fut_tab_bytes = need;
        }
        if (!*tab_ready && hs.n_seas > 0) {
            const int work = a.H * hs.n_seas;
            hipLaunchKernelGGL(future_design_kernel, dim3((unsigned)((work + 255) / 256)), dim3(256), 0, st,
                               ctx->d_spec, a.H, a.ds_future, ctx->fut_tab);
            HIP_TRY(ctx, hipGetLastError());
        }
        *tab_ready = true;
        a.Xf = ctx->fut_tab;
    }
    const int64_t g = a.n_grids == 1 ? 0 : n0;
    a.N = n;
    a.theta += (size_t)n0 * a.theta_stride; a.y_scale += n0; a.grid += g;
    if (!a.shared_future) a.ds_future += (size_t)n0 * a.H;
    if (a.floor_) a.floor_ += n0;
    if (a.cap) a.cap += n0;
    if (a.extra_future && !a.shared_future) a.extra_future += (size_t)n0 * hs.n_extra * a.H;
    a.yhat += (size_t)n0 * a.H;
    if (a.trend_out) a.trend_out += (size_t)n0 * a.H;
    if (a.yhat_int) a.yhat_int += (size_t)n0 * a.H;
    hipLaunchKernelGGL(predict_kernel, dim3((unsigned)((n + PREDICT_WAVES - 1) / PREDICT_WAVES)), dim3(PREDICT_WAVES * 64), 0, st, a);
    HIP_TRY(ctx, hipGetLastError());
    return 0;
}

extern "C" int tsf_predict_dev(tsf_ctx *ctx, const tsf_spec *spec, int64_t N, int32_t H,
                               const double *theta, const double *y_scale,
                               const tsf_grid_info *grid, int32_t n_grids, const int64_t *ds_future,
                               int32_t shared_future, const double *floor_, const double *cap,
                               const double *extra_future, double *yhat, int32_t *yhat_int,
                               void *stream)
{
    if (!ctx) return -1;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const ForecastIn f = {N, H, theta, y_scale, grid, n_grids, ds_future, shared_future, floor_, cap, extra_future, nullptr};
    if (int rc = check_forecast_in(ctx, f, yhat != nullptr)) return rc;
    hipStream_t st = (hipStream_t)stream;
    DevSpec hs;
    if (int rc = forecast_prologue(ctx, spec, f, st, &hs)) return rc;
    PredictArgs a = predict_args(ctx, spec, f, yhat);
    a.yhat_int = yhat_int;
    bool tab_ready = false;
    return launch_predict(ctx, hs, a, 0, N, &tab_ready, st);
}

extern "C" int tsf_predict(tsf_ctx *ctx, const tsf_spec *spec, int64_t N, int32_t H,
                           const double *theta, const double *y_scale, const tsf_grid_info *grid,
                           int32_t n_grids, const int64_t *ds_future, int32_t shared_future,
                           const double *floor_, const double *cap, const double *extra_future,
                           double *yhat, int32_t *yhat_int)
{
    if (!ctx) return -1;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const ForecastIn h = {N, H, theta, y_scale, grid, n_grids, ds_future, shared_future, floor_, cap, extra_future, nullptr};
    if (int rc = check_forecast_in(ctx, h, spec && yhat)) return rc;
    if (int rc = check_grids(ctx, spec, grid, n_grids)) return rc;
    ForecastUpload up;
    if (int rc = up.upload(ctx, spec, h)) return rc;
    const ForecastIn &d = up.dev;
    DevBuf d_yh, d_yi;
    HIP_TRY(ctx, d_yh.alloc(8 * (size_t)N * H));
    if (yhat_int) HIP_TRY(ctx, d_yi.alloc(4 * (size_t)N * H));
    int rc = tsf_predict_dev(ctx, spec, N, H, d.theta, d.y_scale, d.grid, n_grids, d.ds_future, shared_future, d.floor_,
                             d.cap, d.extra_future, d_yh.as<double>(), yhat_int ? d_yi.as<int32_t>() : nullptr, nullptr);
    if (rc) return rc;
    HIP_TRY(ctx, hipDeviceSynchronize());
    HIP_TRY(ctx, hipMemcpy(yhat, d_yh.p, 8 * (size_t)N * H, hipMemcpyDeviceToHost));
    if (yhat_int) HIP_TRY(ctx, hipMemcpy(yhat_int, d_yi.p, 4 * (size_t)N * H, hipMemcpyDeviceToHost));
    return 0;
}

// ---- the chunked draw -------------------------------------------------------------------------------

// The one draw loop behind the intervals, the components' intervals, the quantiles, the scores and the roll-ups, on
// device-resident inputs: per chunk of series launch_predict (yhat and the three per-row pieces), then
// interval_sample_kernel, then `after(n0, nc, bufs)` on the same stream -- what the caller does with the chunk's draws
// before the next chunk overwrites them.  Series are processed in chunks sized so that ALL scratch of a chunk -- the
// per-row pieces of the point forecast (t, additive term, 1 + multiplicative term) and every sample buffer the call
// needs (yhat always; the running sums with want_cum; the trend with want_trend) -- stays within 512 MB.  The scratch
// is the context's cached block (ensure_iv_ws); the chunks of a call and successive calls reuse it in stream order, so
// in the steady state nothing here waits for the device, as the `_dev` contract (include/tsf.h) promises.  (Round 3
// used hipMallocAsync / hipFreeAsync here; see tsf_create.)  As with the workspace: one stream at a time per context.
struct DrawBufs {
    double *samp, *cum, *trend;     // [n_chunk][H][n_samples] each; cum / trend null where not asked for
};

// What a draw is asked for beyond the forecast's inputs.  yhat [N][H] is always written; trend_out [N][H] (the point
// forecast's trend) where not null.
struct DrawSpec {
    int32_t n_samples;
    uint64_t seed;
    bool want_cum, want_trend;
    double *yhat, *trend_out;
    bool takes_ar;          // the entry takes a pending tsf_set_noise_ar; false: it refuses while one is pending
};

// The one-shot rule of tsf_set_noise_ar.  An entry that draws holds a NoiseArOnce from its first line, so the setting
// is gone when the entry returns, whatever it returns; draw_chunks takes the setting or refuses it by DrawSpec's flag,
// and the drawing entries that reach draw_chunks through another public entry refuse it themselves (refuse_noise_ar).
struct NoiseArOnce {
    tsf_ctx *ctx;
    explicit NoiseArOnce(tsf_ctx *c) : ctx(c) {}
    ~NoiseArOnce() { if (ctx) { ctx->ar_pending.clear(); ctx->ar_start_pending.clear(); } }
    NoiseArOnce(const NoiseArOnce &) = delete;
    NoiseArOnce &operator=(const NoiseArOnce &) = delete;
};

static int refuse_noise_ar(tsf_ctx *ctx, const char *who)
{
    if (ctx->ar_pending.empty()) return 0;
    ctx->ar_pending.clear();
    ctx->ar_start_pending.clear();
    ctx->err = std::string(who) + ": a tsf_set_noise_ar setting is pending and this entry does not take it (the setting is cleared)";
    return -1;
}

// a pending setting is for N series, or the call fails (and the setting is cleared)
static int check_noise_ar_count(tsf_ctx *ctx, int64_t N)
{
    const int64_t n = (int64_t)(ctx->ar_pending.size() / 2);
    if (n == 0 || n == N) return 0;
    ctx->ar_pending.clear();
    ctx->ar_start_pending.clear();
    char msg[160];
    snprintf(msg, sizeof(msg), "tsf_set_noise_ar was given %lld series and this call has N = %lld (the setting is cleared)",
             (long long)n, (long long)N);
    return fail(ctx, msg);
}

// The pending pairs onto the device for a draw of N series on st; *dev: the pairs, or null where nothing is pending;
// *dev_start: the (p0, c0, m0) of a pending conditioned start (tsf_set_noise_ar_start: only ever beside pairs of the same
// count), behind the pairs in the same block, or null.
static int take_noise_ar(tsf_ctx *ctx, int64_t N, hipStream_t st, const double **dev, const double **dev_start)
{
    *dev = nullptr;
    *dev_start = nullptr;
    if (int rc = check_noise_ar_count(ctx, N)) return rc;
    if (ctx->ar_pending.empty()) return 0;
    std::vector<double> pairs, start;
    pairs.swap(ctx->ar_pending);
    start.swap(ctx->ar_start_pending);
    const size_t need = 8 * (pairs.size() + start.size());
    // (an earlier draw on this stream may still read the buffer)
    HIP_TRY(ctx, hipStreamSynchronize(st));
    if (ctx->ar_dev_bytes < need) {
        if (ctx->ar_dev) { HIP_TRY(ctx, hipFree(ctx->ar_dev)); ctx->ar_dev = nullptr; ctx->ar_dev_bytes = 0; }
        HIP_TRY(ctx, hipMalloc((void **)&ctx->ar_dev, need));
        ctx->ar_dev_bytes = need;
    }
    HIP_TRY(ctx, hipMemcpy(ctx->ar_dev, pairs.data(), 8 * pairs.size(), hipMemcpyHostToDevice));
    *dev = ctx->ar_dev;
    if (!start.empty()) {
        HIP_TRY(ctx, hipMemcpy(ctx->ar_dev + pairs.size(), start.data(), 8 * start.size(), hipMemcpyHostToDevice));
        *dev_start = ctx->ar_dev + pairs.size();
    }
    return 0;
}

// series per chunk: n_buf sample buffers and the three per-row pieces of a chunk within 512 MB
static int64_t draw_chunk_series(int64_t N, int32_t H, int32_t n_samples, size_t n_buf)
{
    const size_t per_series = (size_t)H * 8 * (3 + n_buf * (size_t)n_samples);
    int64_t chunk = (int64_t)(((size_t)512 << 20) / per_series);
    if (chunk < 1) chunk = 1;
    if (chunk > N) chunk = N;
    return chunk;
}

// bytes of scratch draw_chunks carves for chunks of `chunk` series
static size_t draw_scratch_bytes(int64_t chunk, int32_t H, int32_t n_samples, size_t n_buf)
{
    return 8 * (size_t)chunk * H * (3 + n_buf * (size_t)n_samples);
}

// the sort width of the percentile / quantile / score kernels: the power of two at or above the sample count
static int sort_width(int32_t n_samples)
{
    int NSP = 2;
    while (NSP < n_samples) NSP <<= 1;
    return NSP;
}

// One model's draw of a call: what is set up once (the spec, the launch arguments over the chunk's scratch) and what runs
// per chunk (launch_predict for yhat and the three per-row pieces, then interval_sample_kernel).  draw_chunks runs one of
// them over the context's scratch; tsf_predict_temporal runs two side by side, each chunk's daily and period draws.
struct ModelDraw {
    DevSpec hs;
    PredictArgs p;
    IntervalArgs a;
    double *d_t, *d_xa, *d_opm;
    bool tab_ready;

    // the launch arguments: pieces [3][chunk][H] and the sample buffers `b` of a chunk; d_ar: the series' (phi, c) pairs
    // on the device or null; d_start: beside d_ar, the series' (p0, c0, m0) of a conditioned start, or null.  Nothing is
    // launched.
    void bind(const tsf_ctx *ctx, const tsf_spec *spec, const ForecastIn &f, const DrawSpec &d, const double *d_ar,
              double *pieces, size_t nh, const DrawBufs &b, const double *d_start = nullptr)
    {
        d_t = pieces; d_xa = d_t + nh; d_opm = d_xa + nh;
        p = predict_args(ctx, spec, f, d.yhat);
        p.trend_out = d.trend_out;
        p.t_out = d_t; p.xa_out = d_xa; p.opm_out = d_opm;
        memset(&a, 0, sizeof(a));
        a.sp = ctx->d_spec; a.H = f.H; a.theta_stride = tsf_theta_stride(spec); a.n_grids = f.n_grids; a.NS = d.n_samples;
        a.theta = f.theta; a.y_scale = f.y_scale; a.grid = f.grid; a.floor_ = f.floor_; a.cap = f.cap;
        a.series_key = f.series_key; a.seed = d.seed;
        a.samples = b.samp; a.trend_samples = b.trend; a.cum_samples = b.cum;
        a.noise_ar = d_ar;
        a.ar_start = d_ar ? d_start : nullptr;
        tab_ready = false;
    }
    // the context's device spec (and with it a shared future grid's design table) made this model's, in stream order
    int send_spec(tsf_ctx *ctx, hipStream_t st)
    {
        HIP_TRY(ctx, hipMemcpyAsync(ctx->d_spec, &hs, sizeof(hs), hipMemcpyHostToDevice, st));
        tab_ready = false;
        return 0;
    }
    // the series [n0, n0 + nc) of the call drawn into the chunk's scratch
    int chunk(tsf_ctx *ctx, int64_t n0, int64_t nc, hipStream_t st)
    {
        // the point forecast of the chunk and its per-row pieces (chunk-local scratch: rows of series n0 + i at [i][H])
        if (int prc = launch_predict(ctx, hs, p, n0, nc, &tab_ready, st)) return prc;
        const int H = a.H;
        a.n0 = n0; a.n_chunk = nc;
        a.t = d_t - (size_t)n0 * H; a.xa = d_xa - (size_t)n0 * H; a.opm = d_opm - (size_t)n0 * H;
        const dim3 sgrid((unsigned)nc, (unsigned)((a.NS + 255) / 256));
        if (a.ar_start) {
            // the conditioned start: its mean into the chunk's additive piece and into yhat (p.yhat: the call's [N][H]),
            // behind predict_kernel in stream order; then the instance whose chain starts at e_0 = c0 z_0
            const ArStartArgs sa = {a.noise_ar, a.ar_start, d_xa, p.yhat, n0, nc, H};
            hipLaunchKernelGGL(ar_start_shift_kernel, dim3((unsigned)((nc * H + 255) / 256)), dim3(256), 0, st, sa);
            hipLaunchKernelGGL((interval_sample_kernel<true, true>), sgrid, dim3(256), 0, st, a);
        }
        else if (a.noise_ar) hipLaunchKernelGGL(interval_sample_kernel<true>, sgrid, dim3(256), 0, st, a);
        else hipLaunchKernelGGL(interval_sample_kernel<false>, sgrid, dim3(256), 0, st, a);
        HIP_TRY(ctx, hipGetLastError());
        return 0;
    }
};

template <class After>
static int draw_chunks(tsf_ctx *ctx, const tsf_spec *spec, const ForecastIn &f, const DrawSpec &d, hipStream_t st,
                       After &&after)
{
    if (!d.takes_ar)
        if (int rc = refuse_noise_ar(ctx, "this drawing entry")) return rc;
    const double *d_ar = nullptr, *d_start = nullptr;
    if (int rc = take_noise_ar(ctx, f.N, st, &d_ar, &d_start)) return rc;
    ModelDraw m;
    if (int rc = forecast_spec(ctx, spec, f, &m.hs)) return rc;
    if (int rc = m.send_spec(ctx, st)) return rc;
    const int64_t N = f.N;
    const int32_t H = f.H, n_samples = d.n_samples;
    const size_t n_buf = 1 + (size_t)d.want_cum + (size_t)d.want_trend;
    const int64_t chunk = draw_chunk_series(N, H, n_samples, n_buf);
    const size_t nh = (size_t)chunk * H;
    if (int rc = ensure_iv_ws(ctx, draw_scratch_bytes(chunk, H, n_samples, n_buf))) return rc;
    double *d_samp = (double *)ctx->iv_ws + 3 * nh;
    double *d_next = d_samp + nh * n_samples;
    double *d_cum = nullptr, *d_tsamp = nullptr;
    if (d.want_cum) { d_cum = d_next; d_next += nh * n_samples; }
    if (d.want_trend) d_tsamp = d_next;
    const DrawBufs bufs = {d_samp, d_cum, d_tsamp};
    m.bind(ctx, spec, f, d, d_ar, (double *)ctx->iv_ws, nh, bufs, d_start);
    for (int64_t n0 = 0; n0 < N; n0 += chunk) {
        const int64_t nc = (N - n0 < chunk) ? N - n0 : chunk;
        if (int rc = m.chunk(ctx, n0, nc, st)) return rc;
        if (int arc = after(n0, nc, bufs)) return arc;
    }
    return 0;
}

// interval_percentile_kernel on one sample buffer of a chunk: the two percentiles of `width` per row into lower / upper
// [N][H].  (Of its IntervalArgs the kernel reads the buffer, H, NS, n0, the two fractions and the two outputs.)
struct Percentiles {
    int32_t H, n_samples;
    double width;
    hipStream_t st;

    int launch(tsf_ctx *ctx, double *samples, int64_t n0, int64_t nc, double *lower, double *upper) const
    {
        const int NSP = sort_width(n_samples);
        IntervalArgs a;
        memset(&a, 0, sizeof(a));
        a.samples = samples; a.H = H; a.NS = n_samples; a.n0 = n0; a.n_chunk = nc;
        a.lo_frac = (1.0 - width) / 2.0; a.hi_frac = (1.0 + width) / 2.0;
        a.lower = lower; a.upper = upper;
        hipLaunchKernelGGL(interval_percentile_kernel, dim3((unsigned)(nc * H)), dim3(256), sizeof(double) * NSP, st, a,
                           NSP);
        HIP_TRY(ctx, hipGetLastError());
        return 0;
    }
};

// ---- uncertainty intervals ------------------------------------------------------------------------

extern "C" int tsf_predict_intervals_dev(tsf_ctx *ctx, const tsf_spec *spec, int64_t N, int32_t H,
                                         const double *theta, const double *y_scale,
                                         const tsf_grid_info *grid, int32_t n_grids,
                                         const int64_t *ds_future, int32_t shared_future,
                                         const double *floor_, const double *cap,
                                         const double *extra_future, const int64_t *series_key,
                                         int32_t n_samples, double interval_width, uint64_t seed,
                                         double *yhat, double *yhat_lower, double *yhat_upper, void *stream)
{
    if (!ctx) return -1;
    NoiseArOnce ar_once(ctx);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const ForecastIn f = {N, H, theta, y_scale, grid, n_grids, ds_future, shared_future, floor_, cap, extra_future, series_key};
    if (int rc = check_forecast_in(ctx, f, spec && yhat && yhat_lower && yhat_upper)) return rc;
    if (n_samples < 2 || n_samples > 4096) return fail(ctx, "n_samples must be in [2, 4096]");
    if (!(interval_width > 0.0 && interval_width < 1.0)) return fail(ctx, "interval_width must be in (0, 1)");
    hipStream_t st = (hipStream_t)stream;
    const Percentiles pc = {H, n_samples, interval_width, st};
    const DrawSpec d = {n_samples, seed, false, false, yhat, nullptr, true};
    return draw_chunks(ctx, spec, f, d, st, [&](int64_t n0, int64_t nc, const DrawBufs &b) -> int {
        return pc.launch(ctx, b.samp, n0, nc, yhat_lower, yhat_upper);
    });
}

extern "C" int tsf_predict_intervals(tsf_ctx *ctx, const tsf_spec *spec, int64_t N, int32_t H,
                                     const double *theta, const double *y_scale,
                                     const tsf_grid_info *grid, int32_t n_grids,
                                     const int64_t *ds_future, int32_t shared_future,
                                     const double *floor_, const double *cap,
                                     const double *extra_future, const int64_t *series_key,
                                     int32_t n_samples, double interval_width, uint64_t seed,
                                     double *yhat, double *yhat_lower, double *yhat_upper)
{
    if (!ctx) return -1;
    NoiseArOnce ar_once(ctx);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const ForecastIn h = {N, H, theta, y_scale, grid, n_grids, ds_future, shared_future, floor_, cap, extra_future, series_key};
    if (int rc = check_forecast_in(ctx, h, spec && yhat && yhat_lower && yhat_upper)) return rc;
    if (int rc = check_grids(ctx, spec, grid, n_grids)) return rc;
    ForecastUpload up;
    if (int rc = up.upload(ctx, spec, h)) return rc;
    const ForecastIn &d = up.dev;
    const size_t nh = 8 * (size_t)N * H;
    HostOuts outs;
    double *d_yh = outs.want(yhat, nh), *d_lo = outs.want(yhat_lower, nh), *d_hi = outs.want(yhat_upper, nh);
    if (int rc = outs.ready(ctx)) return rc;
    int rc = tsf_predict_intervals_dev(ctx, spec, N, H, d.theta, d.y_scale, d.grid, n_grids, d.ds_future, shared_future,
                                       d.floor_, d.cap, d.extra_future, d.series_key, n_samples, interval_width, seed,
                                       d_yh, d_lo, d_hi, nullptr);
    if (rc) return rc;
    HIP_TRY(ctx, hipDeviceSynchronize());
    return outs.fetch(ctx);
}

// ---- forecast components ------------------------------------------------------------------------------

// What both component entries check before anything is launched: the component table (host data in both, like the
// spec) against the spec's K, and the interval arguments (iv_outs: the four interval outputs are all there).
static int check_component_args(tsf_ctx *ctx, const tsf_spec *spec, int32_t n_comp, const uint64_t *comp_cols,
                                const int32_t *comp_scaled, const double *comp, int32_t n_samples,
                                double interval_width, bool iv_outs)
{
    if (n_comp < 0 || n_comp > TSF_MAX_COMP) return fail(ctx, "n_comp must be in [0, TSF_MAX_COMP]");
    if (n_comp > 0 && (!comp_cols || !comp_scaled || !comp)) return fail(ctx, "NULL component table or output");
    const int K = tsf_spec_K(spec);
    for (int32_t c = 0; c < n_comp; ++c)
        if (K < 64 && (comp_cols[c] >> (K > 0 ? K : 0)) != 0) {
            char msg[120];
            snprintf(msg, sizeof(msg), "comp_cols[%d]: a column at or above K = %d", (int)c, K);
            return fail(ctx, msg);
        }
    if (n_samples != 0) {
        if (n_samples < 2 || n_samples > 4096) return fail(ctx, "n_samples must be 0 or in [2, 4096]");
        if (!(interval_width > 0.0 && interval_width < 1.0)) return fail(ctx, "interval_width must be in (0, 1)");
        if (!iv_outs) return fail(ctx, "NULL interval output");
    }
    return 0;
}

extern "C" int tsf_predict_components_dev(tsf_ctx *ctx, const tsf_spec *spec, int64_t N, int32_t H,
                                          const double *theta, const double *y_scale, const tsf_grid_info *grid,
                                          int32_t n_grids, const int64_t *ds_future, int32_t shared_future,
                                          const double *floor_, const double *cap, const double *extra_future,
                                          int32_t n_comp, const uint64_t *comp_cols, const int32_t *comp_scaled,
                                          const int64_t *series_key, int32_t n_samples, double interval_width,
                                          uint64_t seed, double *yhat, double *trend, double *comp,
                                          double *yhat_lower, double *yhat_upper, double *trend_lower,
                                          double *trend_upper, void *stream)
{
    if (!ctx) return -1;
    NoiseArOnce ar_once(n_samples != 0 ? ctx : nullptr);        // (without samples the entry draws nothing)
    if (n_samples != 0)
        if (int rc = refuse_noise_ar(ctx, "tsf_predict_components")) return rc;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const ForecastIn f = {N, H, theta, y_scale, grid, n_grids, ds_future, shared_future, floor_, cap, extra_future, series_key};
    if (int rc = check_forecast_in(ctx, f, spec && yhat && trend)) return rc;
    if (int rc = check_component_args(ctx, spec, n_comp, comp_cols, comp_scaled, comp, n_samples, interval_width,
                                      yhat_lower && yhat_upper && trend_lower && trend_upper))
        return rc;
    hipStream_t st = (hipStream_t)stream;
    // the component table (host data): sent ahead of the predict launches, and so ahead of the prologue, which with
    // samples is draw_chunks'; only a HIP error can come between
    const size_t tab_flags = sizeof(uint64_t) * TSF_MAX_COMP;
    if (n_comp > 0) {
        if (!ctx->comp_tab) HIP_TRY(ctx, hipMalloc(&ctx->comp_tab, tab_flags + sizeof(int32_t) * TSF_MAX_COMP));
        HIP_TRY(ctx, hipMemcpyAsync(ctx->comp_tab, comp_cols, sizeof(uint64_t) * n_comp, hipMemcpyHostToDevice, st));
        HIP_TRY(ctx, hipMemcpyAsync((char *)ctx->comp_tab + tab_flags, comp_scaled, sizeof(int32_t) * n_comp,
                                    hipMemcpyHostToDevice, st));
    }
    if (n_samples == 0) {
        DevSpec hs;
        if (int rc = forecast_prologue(ctx, spec, f, st, &hs)) return rc;
        PredictArgs p = predict_args(ctx, spec, f, yhat);
        p.trend_out = trend;
        bool tab_ready = false;
        if (int prc = launch_predict(ctx, hs, p, 0, N, &tab_ready, st)) return prc;
    } else {
        // a second sample buffer (the sampled trend), and the percentiles of both
        const Percentiles pc = {H, n_samples, interval_width, st};
        const DrawSpec d = {n_samples, seed, false, true, yhat, trend, false};
        int rc = draw_chunks(ctx, spec, f, d, st, [&](int64_t n0, int64_t nc, const DrawBufs &b) -> int {
            if (int prc = pc.launch(ctx, b.samp, n0, nc, yhat_lower, yhat_upper)) return prc;
            return pc.launch(ctx, b.trend, n0, nc, trend_lower, trend_upper);
        });
        if (rc) return rc;
    }
    if (n_comp > 0) {
        // behind the predict launches: a shared future grid's design table is built
        ComponentArgs c;
        memset(&c, 0, sizeof(c));
        c.sp = ctx->d_spec; c.N = N; c.H = H; c.theta_stride = tsf_theta_stride(spec);
        c.shared_future = shared_future; c.n_comp = n_comp; c.theta = theta; c.y_scale = y_scale;
        c.ds_future = ds_future; c.extra_future = extra_future; c.Xf = shared_future ? ctx->fut_tab : nullptr;
        c.cols = (const uint64_t *)ctx->comp_tab;
        c.scaled = (const int32_t *)((const char *)ctx->comp_tab + tab_flags);
        c.comp = comp;
        hipLaunchKernelGGL(component_kernel, dim3((unsigned)((N + COMP_WAVES - 1) / COMP_WAVES)), dim3(COMP_WAVES * 64),
                           0, st, c);
        HIP_TRY(ctx, hipGetLastError());
    }
    return 0;
}

extern "C" int tsf_predict_components(tsf_ctx *ctx, const tsf_spec *spec, int64_t N, int32_t H,
                                      const double *theta, const double *y_scale, const tsf_grid_info *grid,
                                      int32_t n_grids, const int64_t *ds_future, int32_t shared_future,
                                      const double *floor_, const double *cap, const double *extra_future,
                                      int32_t n_comp, const uint64_t *comp_cols, const int32_t *comp_scaled,
                                      const int64_t *series_key, int32_t n_samples, double interval_width,
                                      uint64_t seed, double *yhat, double *trend, double *comp,
                                      double *yhat_lower, double *yhat_upper, double *trend_lower, double *trend_upper)
{
    if (!ctx) return -1;
    NoiseArOnce ar_once(n_samples != 0 ? ctx : nullptr);        // (without samples the entry draws nothing)
    if (n_samples != 0)
        if (int rc = refuse_noise_ar(ctx, "tsf_predict_components")) return rc;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const bool iv = n_samples != 0;
    // (the keys matter to the draws only)
    const ForecastIn h = {N, H, theta, y_scale, grid, n_grids, ds_future, shared_future, floor_, cap, extra_future,
                          iv ? series_key : nullptr};
    if (int rc = check_forecast_in(ctx, h, spec && yhat && trend)) return rc;
    if (int rc = check_grids(ctx, spec, grid, n_grids)) return rc;
    if (int rc = check_component_args(ctx, spec, n_comp, comp_cols, comp_scaled, comp, n_samples, interval_width,
                                      yhat_lower && yhat_upper && trend_lower && trend_upper))
        return rc;
    ForecastUpload up;
    if (int rc = up.upload(ctx, spec, h)) return rc;
    const ForecastIn &d = up.dev;
    // (comp without components and the interval outputs without samples are not outputs of the call: no buffer, no copy)
    HostOuts outs;
    const size_t nh = 8 * (size_t)N * H;
    double *d_yh = outs.want(yhat, nh), *d_tr = outs.want(trend, nh);
    double *d_co = n_comp > 0 ? outs.want(comp, nh * n_comp) : nullptr;
    double *d_lo = iv ? outs.want(yhat_lower, nh) : nullptr, *d_hi = iv ? outs.want(yhat_upper, nh) : nullptr;
    double *d_tlo = iv ? outs.want(trend_lower, nh) : nullptr, *d_thi = iv ? outs.want(trend_upper, nh) : nullptr;
    if (int rc = outs.ready(ctx)) return rc;
    int rc = tsf_predict_components_dev(ctx, spec, N, H, d.theta, d.y_scale, d.grid, n_grids, d.ds_future, shared_future,
                                        d.floor_, d.cap, d.extra_future, n_comp, comp_cols, comp_scaled, d.series_key,
                                        n_samples, interval_width, seed, d_yh, d_tr, d_co, d_lo, d_hi, d_tlo, d_thi, nullptr);
    if (rc) return rc;
    HIP_TRY(ctx, hipDeviceSynchronize());
    return outs.fetch(ctx);
}

// ---- forecast quantiles, cumulative quantiles, predictive samples ----------------------------------------

// The sample count and the levels of the quantile, score and window entries (host data in every variant, like the spec).
static int check_samples_and_levels(tsf_ctx *ctx, int32_t n_samples, int32_t n_q, const double *quantiles)
{
    if (n_samples < 2 || n_samples > 4096) return fail(ctx, "n_samples must be in [2, 4096]");
    if (n_q < 0 || n_q > TSF_MAX_QUANT) return fail(ctx, "n_q must be in [0, TSF_MAX_QUANT]");
    if (n_q > 0 && !quantiles) return fail(ctx, "NULL quantiles");
    for (int32_t i = 0; i < n_q; ++i)
        if (!(quantiles[i] >= 0.0 && quantiles[i] <= 1.0)) {       // (NaN fails both comparisons)
            char msg[120];
            snprintf(msg, sizeof(msg), "quantiles[%d] = %g: a level must be finite and in [0, 1]", (int)i, quantiles[i]);
            return fail(ctx, msg);
        }
    return 0;
}

// What both quantile entries check before anything is launched: the sample count, the levels (host data in both, like
// the spec) and that the call asks for something.
static int check_quantile_args(tsf_ctx *ctx, int32_t n_samples, int32_t n_q, const double *quantiles,
                               const tsf_quantile_out *out)
{
    if (!out || !out->yhat) return fail(ctx, "NULL output (tsf_quantile_out and its yhat are required)");
    if (int rc = check_samples_and_levels(ctx, n_samples, n_q, quantiles)) return rc;
    const bool want_q = out->q || out->cum_q || out->trend_q, want_s = out->samples || out->trend_samples;
    if (!want_q && !want_s) return fail(ctx, "nothing requested: q, cum_q, trend_q, samples and trend_samples are all NULL");
    if (n_q == 0 && want_q) return fail(ctx, "n_q = 0 with a quantile output requested");
    if (n_q == 0 && !want_s) return fail(ctx, "n_q = 0 is legal only with a sample output");
    return 0;
}

// What the quantile and score entries are asked for beyond the forecast's inputs: the draw and the levels (host data).
struct QuantileCall {
    int32_t n_samples;
    uint64_t seed;
    int32_t n_q;
    const double *quantiles;
};

// quantile_kernel with the levels of one call: the n_q quantiles of each of `count` * H rows of S sorted draws at src
// (series or groups, the first of them number n0 of the call) into dst [..][n_q][H].  The one launch site of the kernel:
// the forecast's chunks and the roll-up's group ranges.
struct QuantilePass {
    QuantileArgs q;
    int NSP;

    QuantilePass(int32_t H, int32_t S, int32_t n_q, const double *quantiles) : NSP(sort_width(S))
    {
        memset(&q, 0, sizeof(q));
        q.H = H; q.NS = S; q.n_q = n_q;
        for (int32_t i = 0; i < n_q; ++i) q.level[i] = quantiles[i];
    }
    int launch(tsf_ctx *ctx, const double *src, double *dst, int64_t n0, int64_t count, hipStream_t st) const
    {
        QuantileArgs a = q;
        a.src = src; a.dst = dst; a.n0 = n0;
        hipLaunchKernelGGL(quantile_kernel, dim3((unsigned)(count * a.H)), dim3(256), sizeof(double) * NSP, st, a, NSP);
        HIP_TRY(ctx, hipGetLastError());
        return 0;
    }
};

// The work of both quantile entries on device-resident inputs.  The quantile outputs of `o` are device pointers; its
// two sample outputs are copied out of the chunk's scratch in stream order with `kind` (device to device for the _dev
// entry, device to host for the host entry, which therefore never holds N * H * n_samples values on the device).
static int predict_quantiles_run(tsf_ctx *ctx, const tsf_spec *spec, const ForecastIn &f, const QuantileCall &c,
                                 const tsf_quantile_out &o, hipMemcpyKind kind, hipStream_t st)
{
    const int32_t H = f.H, n_samples = c.n_samples;
    const QuantilePass qp(H, n_samples, c.n_q, c.quantiles);
    auto after = [&](int64_t n0, int64_t nc, const DrawBufs &b) -> int {
        const struct { const double *src; double *dst; } sorts[3] = {{b.samp, o.q}, {b.cum, o.cum_q}, {b.trend, o.trend_q}};
        for (const auto &so : sorts)
            if (so.dst)
                if (int rc = qp.launch(ctx, so.src, so.dst, n0, nc, st)) return rc;
        // the raw draws leave the scratch before the next chunk overwrites it (stream order)
        const size_t off = (size_t)n0 * H * n_samples, nb = 8 * (size_t)nc * H * n_samples;
        if (o.samples) HIP_TRY(ctx, hipMemcpyAsync(o.samples + off, b.samp, nb, kind, st));
        if (o.trend_samples) HIP_TRY(ctx, hipMemcpyAsync(o.trend_samples + off, b.trend, nb, kind, st));
        return 0;
    };
    const DrawSpec d = {n_samples, c.seed, o.cum_q != nullptr, o.trend_q || o.trend_samples, o.yhat, nullptr, true};
    return draw_chunks(ctx, spec, f, d, st, after);
}

extern "C" int tsf_predict_quantiles_dev(tsf_ctx *ctx, const tsf_spec *spec, int64_t N, int32_t H,
                                         const double *theta, const double *y_scale, const tsf_grid_info *grid,
                                         int32_t n_grids, const int64_t *ds_future, int32_t shared_future,
                                         const double *floor_, const double *cap, const double *extra_future,
                                         const int64_t *series_key, int32_t n_samples, uint64_t seed, int32_t n_q,
                                         const double *quantiles, tsf_quantile_out *out, void *stream)
{
    if (!ctx) return -1;
    NoiseArOnce ar_once(ctx);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const ForecastIn f = {N, H, theta, y_scale, grid, n_grids, ds_future, shared_future, floor_, cap, extra_future, series_key};
    if (int rc = check_forecast_in(ctx, f, spec != nullptr)) return rc;
    if (int rc = check_quantile_args(ctx, n_samples, n_q, quantiles, out)) return rc;
    return predict_quantiles_run(ctx, spec, f, {n_samples, seed, n_q, quantiles}, *out, hipMemcpyDeviceToDevice,
                                 (hipStream_t)stream);
}

extern "C" int tsf_predict_quantiles(tsf_ctx *ctx, const tsf_spec *spec, int64_t N, int32_t H,
                                     const double *theta, const double *y_scale, const tsf_grid_info *grid,
                                     int32_t n_grids, const int64_t *ds_future, int32_t shared_future,
                                     const double *floor_, const double *cap, const double *extra_future,
                                     const int64_t *series_key, int32_t n_samples, uint64_t seed, int32_t n_q,
                                     const double *quantiles, tsf_quantile_out *out)
{
    if (!ctx) return -1;
    NoiseArOnce ar_once(ctx);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const ForecastIn h = {N, H, theta, y_scale, grid, n_grids, ds_future, shared_future, floor_, cap, extra_future, series_key};
    if (int rc = check_forecast_in(ctx, h, spec != nullptr)) return rc;
    if (int rc = check_grids(ctx, spec, grid, n_grids)) return rc;
    if (int rc = check_quantile_args(ctx, n_samples, n_q, quantiles, out)) return rc;
    ForecastUpload up;
    if (int rc = up.upload(ctx, spec, h)) return rc;
    HostOuts outs;
    const size_t nh = 8 * (size_t)N * H, nqh = nh * (size_t)n_q;
    tsf_quantile_out o;
    o.yhat = outs.want(out->yhat, nh);
    o.q = outs.want(out->q, nqh); o.cum_q = outs.want(out->cum_q, nqh); o.trend_q = outs.want(out->trend_q, nqh);
    o.samples = out->samples; o.trend_samples = out->trend_samples;      // host: filled chunk by chunk
    if (int rc = outs.ready(ctx)) return rc;
    int rc = predict_quantiles_run(ctx, spec, up.dev, {n_samples, seed, n_q, quantiles}, o, hipMemcpyDeviceToHost, nullptr);
    if (rc) return rc;
    HIP_TRY(ctx, hipDeviceSynchronize());
    return outs.fetch(ctx);
}

// ---- scoring observed values against the predictive distribution -------------------------------------------

extern "C" int tsf_score_out_size(void) { return (int)sizeof(tsf_score_out); }

// What both score entries check before anything is launched (after the grid check): tsf_predict_quantiles' checks of the
// sample count and the levels, then what the outputs need.
static int check_score_args(tsf_ctx *ctx, int32_t n_samples, int32_t n_q, const double *quantiles, const double *y_obs,
                            const tsf_score_out *out)
{
    if (!out || !out->yhat) return fail(ctx, "NULL output (tsf_score_out and its yhat are required)");
    if (!y_obs) return fail(ctx, "NULL y_obs");
    if (int rc = check_samples_and_levels(ctx, n_samples, n_q, quantiles)) return rc;
    const bool want_q = out->q || out->pinball || out->mean_pinball || out->coverage;
    if (!want_q && !out->pit && !out->crps && !out->n_obs && !out->mean_crps)
        return fail(ctx, "nothing requested: every output of tsf_score_out beyond yhat is NULL");
    if (n_q == 0 && want_q) return fail(ctx, "n_q = 0 with q, pinball, mean_pinball or coverage requested");
    return 0;
}

// The work of both score entries on device-resident inputs; every pointer of `o` and y_obs are device pointers.  The
// per-row arrays the aggregates read (crps for mean_crps, pinball for mean_pinball, q for coverage) are the caller's
// where given and otherwise lie in the context's sample scratch behind the chunk draw_chunks carves from it: the block
// is sized for both here, so draw_chunks never reallocates under them.
static int score_actuals_run(tsf_ctx *ctx, const tsf_spec *spec, const ForecastIn &f, const QuantileCall &c,
                             const double *y_obs, const tsf_score_out &o, hipStream_t st)
{
    const int64_t N = f.N;
    const int32_t H = f.H, n_samples = c.n_samples, n_q = c.n_q;
    const int NSP = sort_width(n_samples);
    const size_t nh = (size_t)N * H, nqh = nh * (size_t)n_q;
    ScoreArgs a;
    memset(&a, 0, sizeof(a));
    a.y = y_obs; a.pit = o.pit; a.crps = o.crps; a.q = o.q; a.pinball = o.pinball;
    a.H = H; a.NS = n_samples; a.n_q = n_q;
    for (int32_t i = 0; i < n_q; ++i) a.level[i] = c.quantiles[i];
    const size_t extra = (o.mean_crps && !o.crps ? nh : 0) + (o.mean_pinball && !o.pinball ? nqh : 0) +
                         (o.coverage && !o.q ? nqh : 0);
    if (extra) {
        const size_t draw = draw_scratch_bytes(draw_chunk_series(N, H, n_samples, 1), H, n_samples, 1);
        if (int rc = ensure_iv_ws(ctx, draw + 8 * extra)) return rc;
        double *d_next = (double *)((char *)ctx->iv_ws + draw);
        if (o.mean_crps && !o.crps) { a.crps = d_next; d_next += nh; }
        if (o.mean_pinball && !o.pinball) { a.pinball = d_next; d_next += nqh; }
        if (o.coverage && !o.q) a.q = d_next;
    }
    if (a.pit || a.crps || a.q || a.pinball) {
        auto after = [&](int64_t n0, int64_t nc, const DrawBufs &b) -> int {
            a.src = b.samp; a.n0 = n0;
            hipLaunchKernelGGL(score_kernel, dim3((unsigned)(nc * H)), dim3(256), sizeof(double) * NSP, st, a, NSP);
            HIP_TRY(ctx, hipGetLastError());
            return 0;
        };
        const DrawSpec d = {n_samples, c.seed, false, false, o.yhat, nullptr, true};
        if (int rc = draw_chunks(ctx, spec, f, d, st, after)) return rc;
    } else {
        // n_obs alone: no draw is needed, only yhat
        if (int rc = tsf_predict_dev(ctx, spec, N, H, f.theta, f.y_scale, f.grid, f.n_grids, f.ds_future, f.shared_future,
                                     f.floor_, f.cap, f.extra_future, o.yhat, nullptr, st))
            return rc;
    }
    if (o.n_obs || o.mean_crps || o.mean_pinball || o.coverage) {
        ScoreSeriesArgs s;
        memset(&s, 0, sizeof(s));
        s.y = y_obs; s.crps = a.crps; s.q = a.q; s.pinball = a.pinball;
        s.n_obs = o.n_obs; s.mean_crps = o.mean_crps; s.mean_pinball = o.mean_pinball; s.coverage = o.coverage;
        s.N = N; s.H = H; s.n_q = n_q;
        const int64_t threads = N * (1 + n_q);
        hipLaunchKernelGGL(score_series_kernel, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, st, s);
        HIP_TRY(ctx, hipGetLastError());
    }
    return 0;
}

extern "C" int tsf_score_actuals_dev(tsf_ctx *ctx, const tsf_spec *spec, int64_t N, int32_t H, const double *theta,
                                     const double *y_scale, const tsf_grid_info *grid, int32_t n_grids,
                                     const int64_t *ds_future, int32_t shared_future, const double *floor_,
                                     const double *cap, const double *extra_future, const int64_t *series_key,
                                     int32_t n_samples, uint64_t seed, const double *y_obs, int32_t n_q,
                                     const double *quantiles, tsf_score_out *out, void *stream)
{
    if (!ctx) return -1;
    NoiseArOnce ar_once(ctx);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (N < 0 || H <= 0) return fail(ctx, "N must be >= 0 and H > 0");
    if (int rc = check_score_args(ctx, n_samples, n_q, quantiles, y_obs, out)) return rc;
    if (N == 0) return 0;
    const ForecastIn f = {N, H, theta, y_scale, grid, n_grids, ds_future, shared_future, floor_, cap, extra_future, series_key};
    if (int rc = check_forecast_in(ctx, f, spec != nullptr)) return rc;
    return score_actuals_run(ctx, spec, f, {n_samples, seed, n_q, quantiles}, y_obs, *out, (hipStream_t)stream);
}

extern "C" int tsf_score_actuals(tsf_ctx *ctx, const tsf_spec *spec, int64_t N, int32_t H, const double *theta,
                                 const double *y_scale, const tsf_grid_info *grid, int32_t n_grids,
                                 const int64_t *ds_future, int32_t shared_future, const double *floor_, const double *cap,
                                 const double *extra_future, const int64_t *series_key, int32_t n_samples, uint64_t seed,
                                 const double *y_obs, int32_t n_q, const double *quantiles, tsf_score_out *out)
{
    if (!ctx) return -1;
    NoiseArOnce ar_once(ctx);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (N < 0 || H <= 0) return fail(ctx, "N must be >= 0 and H > 0");
    const ForecastIn h = {N, H, theta, y_scale, grid, n_grids, ds_future, shared_future, floor_, cap, extra_future, series_key};
    if (N > 0) {
        if (int rc = check_forecast_in(ctx, h, spec != nullptr)) return rc;
        if (int rc = check_grids(ctx, spec, grid, n_grids)) return rc;
    }
    if (int rc = check_score_args(ctx, n_samples, n_q, quantiles, y_obs, out)) return rc;
    if (N == 0) return 0;
    if (spec->n_extra > 0 && !extra_future) return fail(ctx, "extra_future is NULL");     // (ahead of the scan of y_obs)
    const size_t nhn = (size_t)N * H;
    for (size_t i = 0; i < nhn; ++i)
        if (std::isinf(y_obs[i])) {
            char msg[120];
            snprintf(msg, sizeof(msg), "y_obs[%lld][%d] is infinite: an observed value must be finite (NaN = not observed)",
                     (long long)(i / H), (int)(i % H));
            return fail(ctx, msg);
        }
    ForecastUpload up;
    if (int rc = up.upload(ctx, spec, h)) return rc;
    DevBuf d_y;
    HostOuts outs;
    const size_t nh = 8 * nhn, nqh = nh * (size_t)n_q, nq = 8 * (size_t)N * n_q;
    HIP_TRY(ctx, d_y.put(y_obs, nh));
    tsf_score_out o;
    memset(&o, 0, sizeof(o));
    o.yhat = outs.want(out->yhat, nh);
    o.pit = outs.want(out->pit, nh); o.crps = outs.want(out->crps, nh);
    o.q = outs.want(out->q, nqh); o.pinball = outs.want(out->pinball, nqh);
    o.n_obs = outs.want(out->n_obs, 4 * (size_t)N); o.mean_crps = outs.want(out->mean_crps, 8 * (size_t)N);
    o.mean_pinball = outs.want(out->mean_pinball, nq); o.coverage = outs.want(out->coverage, nq);
    if (int rc = outs.ready(ctx)) return rc;
    int rc = score_actuals_run(ctx, spec, up.dev, {n_samples, seed, n_q, quantiles}, d_y.as<double>(), o, nullptr);
    if (rc) return rc;
    HIP_TRY(ctx, hipDeviceSynchronize());
    return outs.fetch(ctx);
}

// ---- group roll-ups: predictive quantiles of sums over series ---------------------------------------------

// The directly fitted totals of one level's n slots -- the groups (tsf_rollup_set_totals) or the nodes of a level above
// them (tsf_rollup_set_node_totals): allocated by the level's first such call and not before.
struct FittedTotals {
    OwnedDev<double> T, yT;         // [n][H][S] the draws of the totals, [n][H] their yhat
    OwnedDev<int32_t> d_has;        // [n] device copy of has (with T)
    std::vector<int32_t> has;       // [n] the slot has a total (host; empty until then)
};

// One level above the groups in a roll-up's tree (include/tsf.h "tree reconciliation"), n nodes.
struct TreeLevel {
    int64_t n = 0;
    OwnedDev<double> A, C;          // [n][H][S] the bottom-up sum of the children's m; m, then c
    OwnedDev<double> yA, yC;        // [n][H]
    FittedTotals fit;               // the nodes' fitted totals
    OwnedDev<int32_t> d_first, d_child, d_parent;   // [n + 1], [n_below]: each node's children, ascending; [n_below] parents
    std::vector<int64_t> parent;    // [n_below] the parent of each node of the level below (host)
};

// The levels above a roll-up's groups and what tsf_rollup_solve_tree leaves for the two reads.
struct RollupTree {
    std::deque<TreeLevel> up;       // levels 2 .. L
    int64_t M = 0;                  // nodes of all levels, the groups included: the length of mu and kappa
    OwnedDev<double> delta, ydelta; // [G][H][S], [G][H]: m of level 1, then c - acc
    OwnedDev<double> d_mk;          // [2][M] mu, then kappa, of the last solve
    bool solved = false;            // the sweeps have run and nothing was added since
};

// The accumulators of one roll-up (include/tsf.h): owned by the handle, not carved from the context's scratch.
struct tsf_rollup {
    tsf_ctx *ctx = nullptr;
    int64_t G = 0;
    int32_t H = 0, S = 0;
    uint64_t seed = 0;
    OwnedDev<int64_t> d_ds;         // [H] the roll-up's calendar
    OwnedDev<double> acc;           // [G][H][S]
    OwnedDev<double> ysum;          // [G][H]
    std::vector<int64_t> count;     // [G] members added so far (host)
    bool poisoned = false;          // a HIP failure in the middle of an add: the accumulators may be half-added
    FittedTotals top;               // reconciliation: the groups' fitted totals
    // correlated noise (tsf_rollup_set_noise_corr): allocated by that call and not before
    bool corr = false;              // a correlation is set: adds go through rollup_add_corr_kernel
    bool added = false;             // an add of N > 0 series has reached the accumulators
    OwnedDev<double> d_corr_ab;     // [2][G] a = sqrt(1 - rho) - 1, then b = sqrt(rho)
    OwnedDev<int64_t> d_group_key;  // [G]
    std::vector<double> corr_a, corr_b;     // the host copies
    std::vector<int64_t> group_key;
    // tree reconciliation (tsf_rollup_set_tree): allocated by that call and not before
    std::unique_ptr<RollupTree> tree;
};

// A HIP failure of a roll-up's own allocations and copies: the message of the entry, -2, and the error read so that it
// is not sticky (an allocation failure is not, once read: the context stays usable).
static int rollup_hip_fail(tsf_ctx *ctx, const char *entry, hipError_t e)
{
    ctx->err = std::string(entry) + ": " + hipGetErrorString(e);
    (void)hipGetLastError();
    return -2;
}

// the accumulators of a new roll-up: the calendar sent, +0.0 everywhere else
static hipError_t rollup_alloc(tsf_rollup *r, const int64_t *ds_future)
{
    const size_t gh = (size_t)r->G * r->H;
    HIP_OK(r->d_ds.alloc((size_t)r->H));
    HIP_OK(r->acc.alloc(gh * r->S, true));
    HIP_OK(r->ysum.alloc(gh, true));
    HIP_OK(hipMemcpy(r->d_ds, ds_future, 8 * (size_t)r->H, hipMemcpyHostToDevice));
    return hipDeviceSynchronize();
}

extern "C" int tsf_rollup_create(tsf_ctx *ctx, int64_t G, int32_t H, const int64_t *ds_future, int32_t n_samples,
                                 uint64_t seed, tsf_rollup **out)
{
    if (!ctx) return -1;
    if (!out) return fail(ctx, "NULL out");
    *out = nullptr;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (G < 1 || G > 2147483647) return fail(ctx, "G must be in [1, 2^31 - 1]");
    if (H < 1) return fail(ctx, "H must be >= 1");
    if (n_samples < 2 || n_samples > 4096) return fail(ctx, "n_samples must be in [2, 4096]");
    if (!ds_future) return fail(ctx, "NULL ds_future");
    // (a return before the release frees the handle and, through its members, whatever it had allocated)
    std::unique_ptr<tsf_rollup> r(new tsf_rollup());
    r->ctx = ctx; r->G = G; r->H = H; r->S = n_samples; r->seed = seed;
    const hipError_t e = rollup_alloc(r.get(), ds_future);
    if (e != hipSuccess) return rollup_hip_fail(ctx, "tsf_rollup_create", e);
    try {
        r->count.assign((size_t)G, 0);
    } catch (const std::bad_alloc &) {
        return fail(ctx, "tsf_rollup_create: out of host memory");
    }
    *out = r.release();
    return 0;
}

extern "C" void tsf_rollup_free(tsf_rollup *r)
{
    if (!r) return;
    hipSetDevice(r->ctx->device);
    delete r;
}

static const char *const ROLLUP_POISONED =
    "the roll-up is poisoned: an earlier tsf_rollup_add or tsf_rollup_set_totals failed in the middle";
static const char *const ROLLUP_CORR_NO_RECONCILE =
    "the roll-up has a noise correlation set (tsf_rollup_set_noise_corr): reconciling correlated draws is not supported";

// How every entry on a handle opens: the handle is there (-1 without one), its device is current, no earlier call left
// it half-written; no_corr: and it has no noise correlation set (the reconciliation entries).  Then ctx = r->ctx.
static int rollup_enter(tsf_rollup *r, bool no_corr = false)
{
    if (!r) return -1;
    tsf_ctx *ctx = r->ctx;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (r->poisoned) return fail(ctx, ROLLUP_POISONED);
    if (no_corr && r->corr) return fail(ctx, ROLLUP_CORR_NO_RECONCILE);
    return 0;
}

// The series of one call on a roll-up as its entries receive them (host pointers): the models, their forecast inputs on
// the handle's calendar, and the group (or node) of each.
struct RollupCall {
    const tsf_spec *spec;
    int64_t N;
    const double *theta, *y_scale;
    const tsf_grid_info *grid;
    int32_t n_grids;
    const double *floor_, *cap, *extra_future;
    int32_t shared_extra;
    const int64_t *series_key, *group;
};

// What tsf_rollup_add, tsf_rollup_set_totals and tsf_rollup_reconcile check of their series before anything is copied
// or launched (the handle is not poisoned, N > 0).
static int rollup_check_series(tsf_rollup *r, const RollupCall &c, int64_t G = -1 /* the handle's */)
{
    tsf_ctx *ctx = r->ctx;
    const tsf_spec *spec = c.spec;
    const int64_t N = c.N, *group = c.group;
    const tsf_grid_info *grid = c.grid;
    const int32_t n_grids = c.n_grids;
    if (G < 0) G = r->G;
    if (N > 2147483647) return fail(ctx, "N must be < 2^31 per call");
    if (!spec || !c.theta || !c.y_scale || !grid) return fail(ctx, "NULL input");
    if (!c.series_key)
        return fail(ctx, "series_key is required: the index-in-call default would give two calls the same streams");
    if (!group) return fail(ctx, "NULL group");
    if (n_grids != 1 && n_grids != N) return fail(ctx, "n_grids must be 1 or N");
    for (int64_t n = 0; n < N; ++n)
        if (group[n] < 0 || group[n] >= G) {
            char msg[120];
            snprintf(msg, sizeof(msg), "group[%lld] = %lld: outside [0, G = %lld)", (long long)n, (long long)group[n],
                     (long long)G);
            return fail(ctx, msg);
        }
    if (int rc = check_grids(ctx, spec, grid, n_grids)) return rc;
    {
        DevSpec hs;
        int mode = 0;
        if (int rc = build_devspec(ctx, spec, &hs, &mode)) return rc;
    }
    if (spec->n_extra > 0 && !c.extra_future) return fail(ctx, "extra_future is NULL");
    if (spec->growth == TSF_GROWTH_LOGISTIC && !c.cap) return fail(ctx, "logistic growth needs cap");
    return 0;
}

// The series of one such call on the device, on the handle's calendar.  Shared extra columns (or none): tsf_predict on
// the shared calendar; per-series columns: tsf_predict with the calendar repeated per series (shared_future = 0), which
// is what their layout [N][n_extra][H] belongs to.
struct RollupSeries {
    DevBuf d_ds;
    ForecastUpload up;

    int upload(tsf_rollup *r, const RollupCall &c)
    {
        tsf_ctx *ctx = r->ctx;
        const int32_t H = r->H;
        const int64_t N = c.N;
        const int shared = (c.spec->n_extra == 0 || c.shared_extra) ? 1 : 0;
        // the calendar is the handle's, on the device already; the inputs beside it are uploaded
        const int64_t *ds_dev = r->d_ds;
        if (!shared) {
            std::vector<int64_t> ds_rep;
            try {
                ds_rep.resize((size_t)N * H);
            } catch (const std::bad_alloc &) {
                return fail(ctx, "tsf_rollup: out of host memory");
            }
            HIP_TRY(ctx, hipMemcpy(ds_rep.data(), r->d_ds, 8 * (size_t)H, hipMemcpyDeviceToHost));
            for (int64_t n = 1; n < N; ++n) memcpy(&ds_rep[(size_t)n * H], ds_rep.data(), 8 * (size_t)H);
            HIP_TRY(ctx, d_ds.put(ds_rep.data(), 8 * (size_t)N * H));
            ds_dev = d_ds.as<int64_t>();
        }
        const ForecastIn h = {N, H, c.theta, c.y_scale, c.grid, c.n_grids, ds_dev, shared, c.floor_, c.cap, c.extra_future,
                              c.series_key};
        return up.upload(ctx, c.spec, h, true);
    }
};

// The work of tsf_rollup_add (into acc / ysum) and of tsf_rollup_set_totals (into top / ytop) once the call is
// checked: the series' draws added to the cells of their groups by rollup_add_kernel -- on a handle with a noise
// correlation set (tsf_rollup_add only: set_totals is refused there) by rollup_add_corr_kernel, after one
// rollup_noise_scale_kernel over the call's series.
static int rollup_accumulate(tsf_rollup *r, const RollupCall &c, double *acc, double *ysum)
{
    tsf_ctx *ctx = r->ctx;
    const tsf_spec *spec = c.spec;
    const int64_t N = c.N;
    const int32_t H = r->H, S = r->S;
    const int64_t chunk = draw_chunk_series(N, H, S, 1);       // draw_chunks' chunks: one sample buffer
    RollupPlan P;
    try {
        rollup_plan(c.group, N, chunk, &P);
    } catch (const std::bad_alloc &) {
        return fail(ctx, "tsf_rollup: out of host memory");
    }
    RollupSeries in;
    if (int rc = in.upload(r, c)) return rc;
    DevBuf d_yh, d_csr, d_sn;
    HIP_TRY(ctx, d_yh.alloc(8 * (size_t)N * H));
    if (r->corr) HIP_TRY(ctx, d_sn.alloc(8 * (size_t)N));
    const size_t n_t = P.touched.size(), n_f = P.first.size();
    HIP_TRY(ctx, d_csr.alloc(4 * (n_t + n_f + (size_t)N)));
    int32_t *d_touched = d_csr.as<int32_t>(), *d_first = d_touched + n_t, *d_member = d_first + n_f;
    HIP_TRY(ctx, hipMemcpy(d_touched, P.touched.data(), 4 * n_t, hipMemcpyHostToDevice));
    HIP_TRY(ctx, hipMemcpy(d_first, P.first.data(), 4 * n_f, hipMemcpyHostToDevice));
    HIP_TRY(ctx, hipMemcpy(d_member, P.member.data(), 4 * (size_t)N, hipMemcpyHostToDevice));
    // from here on the accumulators are written: any failure leaves them half-added, so the handle is poisoned
    r->poisoned = true;
    RollupAddArgs ra;
    memset(&ra, 0, sizeof(ra));
    ra.acc = acc; ra.ysum = ysum; ra.H = H; ra.NS = S;
    if (r->corr) {
        hipLaunchKernelGGL(rollup_noise_scale_kernel, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, nullptr, in.up.dev.theta,
                           tsf_theta_stride(spec), in.up.dev.y_scale, N, d_sn.as<double>());
        HIP_TRY(ctx, hipGetLastError());
    }
    auto after = [&](int64_t n0, int64_t nc, const DrawBufs &b) -> int {
        const size_t k = (size_t)(n0 / chunk);
        const size_t n_touched = (k + 1 < P.t0.size() ? P.t0[k + 1] : n_t) - P.t0[k];
        ra.samples = b.samp; ra.yhat = d_yh.as<double>() + (size_t)n0 * H;
        ra.touched = d_touched + P.t0[k]; ra.first = d_first + P.f0[k]; ra.member = d_member + n0;
        (void)nc;
        const dim3 grid((unsigned)(n_touched * (size_t)H), (unsigned)((S + 255) / 256));
        if (r->corr) {
            const RollupCorrArgs rc = {ra, r->d_corr_ab, r->d_corr_ab + r->G, r->d_group_key, d_sn.as<double>() + n0,
                                       in.up.dev.series_key + n0, r->seed};
            hipLaunchKernelGGL(rollup_add_corr_kernel, grid, dim3(256), 0, nullptr, rc);
        } else {
            hipLaunchKernelGGL(rollup_add_kernel, grid, dim3(256), 0, nullptr, ra);
        }
        HIP_TRY(ctx, hipGetLastError());
        return 0;
    };
    const DrawSpec d = {S, r->seed, false, false, d_yh.as<double>(), nullptr, acc == r->acc && !r->corr};
    int rc = draw_chunks(ctx, spec, in.up.dev, d, nullptr, after);
    if (rc) return rc;
    HIP_TRY(ctx, hipDeviceSynchronize());
    r->poisoned = false;
    return 0;
}

extern "C" int tsf_rollup_add(tsf_rollup *r, const tsf_spec *spec, int64_t N, const double *theta, const double *y_scale,
                              const tsf_grid_info *grid, int32_t n_grids, const double *floor_, const double *cap,
                              const double *extra_future, int32_t shared_extra, const int64_t *series_key,
                              const int64_t *group)
{
    NoiseArOnce ar_once(r ? r->ctx : nullptr);
    if (int rc = rollup_enter(r)) return rc;
    tsf_ctx *ctx = r->ctx;
    // (before anything is launched: a refusal leaves the accumulators untouched and the handle usable)
    if (r->corr)
        if (int rc = refuse_noise_ar(ctx, "tsf_rollup_add on a handle with a noise correlation")) return rc;
    if (N < 0) return fail(ctx, "N must be >= 0");
    if (int rc = check_noise_ar_count(ctx, N)) return rc;
    if (N == 0) return 0;
    const RollupCall c = {spec, N, theta, y_scale, grid, n_grids, floor_, cap, extra_future, shared_extra, series_key, group};
    if (int rc = rollup_check_series(r, c)) return rc;
    if (int rc = rollup_accumulate(r, c, r->acc, r->ysum)) return rc;
    for (int64_t n = 0; n < N; ++n) r->count[(size_t)group[n]] += 1;
    r->added = true;
    if (r->tree) r->tree->solved = false;
    return 0;
}

// ---- conditional seasonalities: their design columns ----------------------------------------------------------

// What both entries check before anything is launched (cs is host memory in both); *a: the kernel's arguments but for
// its three pointers, *C: the number of columns.
static int check_cond_call(tsf_ctx *ctx, const tsf_cond_seas *cs, int64_t rows, const int64_t *ds, int32_t n_cond,
                           const uint8_t *cond, const double *cols, int64_t col_stride, CondArgs *a, int *C)
{
    if (!cs) return fail(ctx, "NULL tsf_cond_seas");
    if (rows < 0) return fail(ctx, "rows must be >= 0");
    if (col_stride < rows) return fail(ctx, "col_stride must be >= rows");
    if (cs->n < 1 || cs->n > TSF_MAX_SEAS) return fail(ctx, "tsf_cond_seas.n must be in [1, TSF_MAX_SEAS]");
    if (n_cond < 1) return fail(ctx, "n_cond must be >= 1");
    memset(a, 0, sizeof(*a));
    int col = 0;
    char msg[120];
    for (int s = 0; s < cs->n; ++s) {
        if (!(std::isfinite(cs->period[s]) && cs->period[s] > 0.0)) {
            snprintf(msg, sizeof(msg), "period[%d] = %g: a period must be finite and > 0", s, cs->period[s]);
            return fail(ctx, msg);
        }
        if (cs->order[s] < 1 || cs->order[s] > TSF_MAX_EXTRA / 2) {
            snprintf(msg, sizeof(msg), "order[%d] = %d: an order must be in [1, TSF_MAX_EXTRA / 2]", s, (int)cs->order[s]);
            return fail(ctx, msg);
        }
        if (cs->cond[s] < 0 || cs->cond[s] >= n_cond) {
            snprintf(msg, sizeof(msg), "cond[%d] = %d: outside [0, n_cond = %d)", s, (int)cs->cond[s], (int)n_cond);
            return fail(ctx, msg);
        }
        a->period[s] = cs->period[s]; a->order[s] = cs->order[s]; a->cond_row[s] = cs->cond[s]; a->col0[s] = col;
        col += 2 * cs->order[s];
        if (col > TSF_MAX_EXTRA) return fail(ctx, "the orders give more than TSF_MAX_EXTRA columns (sum of 2 * order)");
    }
    if (rows > 0 && (!ds || !cond || !cols)) return fail(ctx, "NULL input (ds, cond and cols are required)");
    a->n = cs->n; a->rows = rows; a->col_stride = col_stride;
    *C = col;
    return 0;
}

static int cond_launch(tsf_ctx *ctx, CondArgs a, const int64_t *d_ds, const uint8_t *d_cond, double *d_cols, hipStream_t st)
{
    a.ds = d_ds; a.cond = d_cond; a.cols = d_cols;
    const int64_t blocks = std::min<int64_t>((a.rows + COND_BLOCK - 1) / COND_BLOCK, 65536);    // (a grid-stride loop)
    hipLaunchKernelGGL(cond_columns_kernel, dim3((unsigned)blocks, (unsigned)a.n), dim3(COND_BLOCK), 0, st, a);
    HIP_TRY(ctx, hipGetLastError());
    return 0;
}

extern "C" int tsf_cond_columns_dev(tsf_ctx *ctx, const tsf_cond_seas *cs, int64_t rows, const int64_t *ds, int32_t n_cond,
                                    const uint8_t *cond, double *cols, int64_t col_stride, void *stream)
{
    if (!ctx) return -1;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    CondArgs a;
    int C = 0;
    if (int rc = check_cond_call(ctx, cs, rows, ds, n_cond, cond, cols, col_stride, &a, &C)) return rc;
    if (rows == 0) return 0;
    return cond_launch(ctx, a, ds, cond, cols, (hipStream_t)stream);
}

extern "C" int tsf_cond_columns(tsf_ctx *ctx, const tsf_cond_seas *cs, int64_t rows, const int64_t *ds, int32_t n_cond,
                                const uint8_t *cond, double *cols, int64_t col_stride)
{
    if (!ctx) return -1;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    CondArgs a;
    int C = 0;
    if (int rc = check_cond_call(ctx, cs, rows, ds, n_cond, cond, cols, col_stride, &a, &C)) return rc;
    if (rows == 0) return 0;
    const size_t r = (size_t)rows;
    DevBuf d_ds, d_cond, d_cols;
    HIP_TRY(ctx, d_ds.put(ds, 8 * r));
    HIP_TRY(ctx, d_cond.put(cond, (size_t)n_cond * r));
    HIP_TRY(ctx, d_cols.alloc(8 * (size_t)C * r));
    a.col_stride = rows;            // (the device copy is dense; the caller's stride is applied on the way back)
    if (int rc = cond_launch(ctx, a, d_ds.as<int64_t>(), d_cond.as<uint8_t>(), d_cols.as<double>(), nullptr)) return rc;
    // rows of `rows` doubles into rows of `col_stride`: what lies behind a column's rows at the caller's is not touched
    HIP_TRY(ctx, hipMemcpy2D(cols, 8 * (size_t)col_stride, d_cols.p, 8 * r, 8 * r, (size_t)C, hipMemcpyDeviceToHost));
    return 0;
}

// ---- correlated group roll-ups: the residual correlation of a group, and the add that draws with it -------------

extern "C" int tsf_corr_args_size(void) { return (int)sizeof(tsf_corr_args); }
extern "C" int tsf_corr_out_size(void) { return (int)sizeof(tsf_corr_out); }

// What both estimator entries check before anything is launched; group and args are host memory in both.  *a: the
// arguments in force (the defaults where args is NULL).
static int check_corr_call(tsf_ctx *ctx, int64_t N, int32_t T, const void *y, int32_t y_dtype, const double *fitted,
                           const int64_t *group, int64_t G, const tsf_corr_args *args, const tsf_corr_out *out,
                           tsf_corr_args *a)
{
    if (N < 0 || N > (int64_t)INT32_MAX) return fail(ctx, "N must be in [0, 2^31 - 1]");
    if (G < 1 || G > (int64_t)INT32_MAX) return fail(ctx, "G must be in [1, 2^31 - 1]");
    if (T < 1) return fail(ctx, "T must be >= 1 (aligned panels only)");
    if (!out || !out->rho || !out->status) return fail(ctx, "NULL output (tsf_corr_out, its rho and its status are required)");
    a->rho_max = 0.95; a->min_rows = 8;
    if (args) *a = *args;
    if (!(a->rho_max >= 0.0 && a->rho_max <= 1.0)) return fail(ctx, "rho_max must be in [0, 1]");
    if (a->min_rows < 2) return fail(ctx, "min_rows must be >= 2");
    if (y_dtype < TSF_Y_F64 || y_dtype > TSF_Y_I32) return fail(ctx, "bad y_dtype");
    if (N > 0 && (!y || !fitted || !group)) return fail(ctx, "NULL input (y, fitted and group are required)");
    for (int64_t n = 0; n < N; ++n)
        if (group[n] < -1 || group[n] >= G) {
            char msg[120];
            snprintf(msg, sizeof(msg), "group[%lld] = %lld: outside [-1, G = %lld)", (long long)n, (long long)group[n],
                     (long long)G);
            return fail(ctx, msg);
        }
    const int64_t row_blocks = ((int64_t)T + 255) / 256;
    if (G * row_blocks > (int64_t)INT32_MAX) return fail(ctx, "G * ceil(T / 256) must be < 2^31");
    return 0;
}

// The estimator on device-resident y and fitted; o: device pointers (rho and status required).  The members' CSR is
// built here, on the host, from the host's group (sorted by group, then by series index, as rollup_plan sorts).  Ends
// with a synchronisation of the stream: its scratch goes back to the pool.
static int corr_run(tsf_ctx *ctx, int64_t N, int32_t T, const void *d_y, int32_t y_dtype, const double *d_fit,
                    const int64_t *group, int64_t G, const tsf_corr_args &a, const tsf_corr_out &o, hipStream_t st)
{
    std::vector<int32_t> csr;
    try {
        csr.assign((size_t)G + 1 + (size_t)N, 0);
    } catch (const std::bad_alloc &) {
        return fail(ctx, "tsf_residual_corr: out of host memory");
    }
    int32_t *first = csr.data(), *member = first + G + 1;
    for (int64_t n = 0; n < N; ++n)
        if (group[n] >= 0) first[group[n] + 1] += 1;
    for (int64_t g = 0; g < G; ++g) first[g + 1] += first[g];
    {
        std::vector<int32_t> at(first, first + G);
        for (int64_t n = 0; n < N; ++n)
            if (group[n] >= 0) member[at[(size_t)group[n]]++] = (int32_t)n;    // ascending n within a group
    }
    const size_t nt = (size_t)N * T, gt = (size_t)G * T;
    DevBuf d_csr, d_scale, d_e, d_c, d_p;
    HIP_TRY(ctx, d_csr.alloc(4 * csr.size()));
    HIP_TRY(ctx, hipMemcpy(d_csr.p, csr.data(), 4 * csr.size(), hipMemcpyHostToDevice));
    double *scale = o.scale;
    if (!scale) { HIP_TRY(ctx, d_scale.alloc(8 * (size_t)N)); scale = d_scale.as<double>(); }
    HIP_TRY(ctx, d_e.alloc(8 * nt));
    HIP_TRY(ctx, d_c.alloc(8 * gt));
    HIP_TRY(ctx, d_p.alloc(8 * gt));
    const int32_t *d_first = d_csr.as<int32_t>(), *d_member = d_first + G + 1;
    if (N > 0) {
        const CorrScaleArgs s = {d_y, d_fit, N, T, y_dtype, a.min_rows, scale, d_e.as<double>()};
        hipLaunchKernelGGL(corr_scale_kernel, dim3((unsigned)((N + CORR_WAVES - 1) / CORR_WAVES)), dim3(CORR_WAVES * 64), 0, st, s);
        HIP_TRY(ctx, hipGetLastError());
    }
    const int32_t row_blocks = (T + 255) / 256;
    const CorrRowsArgs w = {d_e.as<double>(), d_first, d_member, T, row_blocks, d_c.as<double>(), d_p.as<int64_t>()};
    hipLaunchKernelGGL(corr_rows_kernel, dim3((unsigned)(G * row_blocks)), dim3(256), 0, st, w);
    HIP_TRY(ctx, hipGetLastError());
    const CorrGroupArgs k = {d_c.as<double>(), d_p.as<int64_t>(), scale, d_first, d_member, G, T, a.rho_max,
                             o.rho, o.rho_raw, o.n_pairs, o.n_used, o.status};
    hipLaunchKernelGGL(corr_group_kernel, dim3((unsigned)((G + CORR_WAVES - 1) / CORR_WAVES)), dim3(CORR_WAVES * 64), 0, st, k,
                       (int)TSF_CORR_OK, (int)TSF_CORR_NO_PAIRS);
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, hipStreamSynchronize(st));
    return 0;
}

extern "C" int tsf_residual_corr_dev(tsf_ctx *ctx, int64_t N, int32_t T, const void *y, int32_t y_dtype, const double *fitted,
                                     const int64_t *group, int64_t G, const tsf_corr_args *args, tsf_corr_out *out,
                                     void *stream)
{
    if (!ctx) return -1;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    tsf_corr_args a;
    if (int rc = check_corr_call(ctx, N, T, y, y_dtype, fitted, group, G, args, out, &a)) return rc;
    return corr_run(ctx, N, T, y, y_dtype, fitted, group, G, a, *out, (hipStream_t)stream);
}

extern "C" int tsf_residual_corr(tsf_ctx *ctx, int64_t N, int32_t T, const void *y, int32_t y_dtype, const double *fitted,
                                 const int64_t *group, int64_t G, const tsf_corr_args *args, tsf_corr_out *out)
{
    if (!ctx) return -1;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    tsf_corr_args a;
    if (int rc = check_corr_call(ctx, N, T, y, y_dtype, fitted, group, G, args, out, &a)) return rc;
    const size_t nt = (size_t)N * T, ysz = ysize(y_dtype), g = (size_t)G, n = (size_t)N;
    DevBuf d_y, d_fit;
    HostOuts outs;
    HIP_TRY(ctx, d_y.put(y, ysz * nt));
    HIP_TRY(ctx, d_fit.put(fitted, 8 * nt));
    tsf_corr_out o;
    memset(&o, 0, sizeof(o));
    o.rho = outs.want(out->rho, 8 * g); o.status = outs.want(out->status, 4 * g);
    o.rho_raw = outs.want(out->rho_raw, 8 * g); o.n_pairs = outs.want(out->n_pairs, 8 * g);
    o.n_used = outs.want(out->n_used, 4 * g); o.scale = outs.want(out->scale, 8 * n);
    if (int rc = outs.ready(ctx)) return rc;
    // (corr_run ends with a synchronisation of its stream)
    if (int rc = corr_run(ctx, N, T, d_y.p, y_dtype, d_fit.as<double>(), group, G, a, o, nullptr)) return rc;
    return outs.fetch(ctx);
}

// ---- serially correlated observation noise: the estimator of a series' residual autocorrelation, and the setting ----

extern "C" int tsf_ar_args_size(void) { return (int)sizeof(tsf_ar_args); }
extern "C" int tsf_ar_out_size(void) { return (int)sizeof(tsf_ar_out); }

// What both estimator entries check before anything is launched; offsets and args are host memory in both.  *a: the
// arguments in force (the defaults where args is NULL).
static int check_ar_call(tsf_ctx *ctx, int64_t N, int32_t T, const int64_t *offsets, const void *y, int32_t y_dtype,
                         const double *fitted, const tsf_ar_args *args, const tsf_ar_out *out, tsf_ar_args *a)
{
    if (N < 0 || N > (int64_t)INT32_MAX) return fail(ctx, "N must be in [0, 2^31 - 1]");
    if (!out || !out->phi || !out->status) return fail(ctx, "NULL output (tsf_ar_out, its phi and its status are required)");
    a->phi_max = 0.95; a->min_pairs = 8; a->reserved_ = 0;
    if (args) *a = *args;
    if (!(a->phi_max >= 0.0 && a->phi_max < 1.0)) return fail(ctx, "phi_max must be in [0, 1)");
    if (a->min_pairs < 1) return fail(ctx, "min_pairs must be >= 1");
    if (y_dtype < TSF_Y_F64 || y_dtype > TSF_Y_I32) return fail(ctx, "bad y_dtype");
    if (N > 0 && (!y || !fitted)) return fail(ctx, "NULL input (y and fitted are required)");
    if (!offsets) return T >= 1 ? 0 : fail(ctx, "bad panel (aligned: T >= 1)");
    if (offsets[0] != 0) return fail(ctx, "bad panel (ragged: offsets[0] = 0)");
    for (int64_t n = 0; n < N; ++n)
        if (offsets[n + 1] < offsets[n]) return fail(ctx, "bad panel (ragged: offsets ascending)");
    return 0;
}

// The estimator on device-resident y and fitted; d_off: the offsets on the device (null aligned); o: device pointers.
static int ar_run(tsf_ctx *ctx, int64_t N, int32_t T, const int64_t *d_off, const void *d_y, int32_t y_dtype,
                  const double *d_fit, const tsf_ar_args &a, const tsf_ar_out &o, hipStream_t st)
{
    if (N == 0) return 0;
    const ArArgs k = {d_y, d_fit, d_off, N, T, y_dtype, a.min_pairs, a.phi_max, o.phi, o.phi_raw, o.n_pairs, o.scale, o.status};
    hipLaunchKernelGGL(ar_series_kernel, dim3((unsigned)((N + AR_WAVES - 1) / AR_WAVES)), dim3(AR_WAVES * 64), 0, st, k,
                       (int)TSF_AR_OK, (int)TSF_AR_NO_PAIRS);
    HIP_TRY(ctx, hipGetLastError());
    return 0;
}

extern "C" int tsf_residual_autocorr_dev(tsf_ctx *ctx, int64_t N, int32_t T, const int64_t *offsets, const void *y,
                                         int32_t y_dtype, const double *fitted, const tsf_ar_args *args, tsf_ar_out *out,
                                         void *stream)
{
    if (!ctx) return -1;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    tsf_ar_args a;
    if (int rc = check_ar_call(ctx, N, T, offsets, y, y_dtype, fitted, args, out, &a)) return rc;
    hipStream_t st = (hipStream_t)stream;
    DevBuf d_off;
    if (offsets && N > 0) HIP_TRY(ctx, d_off.put(offsets, 8 * ((size_t)N + 1)));
    if (int rc = ar_run(ctx, N, T, offsets ? d_off.as<int64_t>() : nullptr, y, y_dtype, fitted, a, *out, st)) return rc;
    HIP_TRY(ctx, hipStreamSynchronize(st));         // (the offsets go back to the pool)
    return 0;
}

extern "C" int tsf_residual_autocorr(tsf_ctx *ctx, int64_t N, int32_t T, const int64_t *offsets, const void *y,
                                     int32_t y_dtype, const double *fitted, const tsf_ar_args *args, tsf_ar_out *out)
{
    if (!ctx) return -1;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    tsf_ar_args a;
    if (int rc = check_ar_call(ctx, N, T, offsets, y, y_dtype, fitted, args, out, &a)) return rc;
    if (N == 0) return 0;
    const size_t rows = offsets ? (size_t)offsets[N] : (size_t)N * T, n = (size_t)N;
    DevBuf d_off, d_y, d_fit;
    HostOuts outs;
    if (offsets) HIP_TRY(ctx, d_off.put(offsets, 8 * (n + 1)));
    HIP_TRY(ctx, d_y.put(y, ysize(y_dtype) * rows));
    HIP_TRY(ctx, d_fit.put(fitted, 8 * rows));
    tsf_ar_out o;
    memset(&o, 0, sizeof(o));
    o.phi = outs.want(out->phi, 8 * n); o.status = outs.want(out->status, 4 * n);
    o.phi_raw = outs.want(out->phi_raw, 8 * n); o.n_pairs = outs.want(out->n_pairs, 8 * n);
    o.scale = outs.want(out->scale, 8 * n);
    if (int rc = outs.ready(ctx)) return rc;
    if (int rc = ar_run(ctx, N, T, offsets ? d_off.as<int64_t>() : nullptr, d_y.p, y_dtype, d_fit.as<double>(), a, o, nullptr))
        return rc;
    HIP_TRY(ctx, hipDeviceSynchronize());
    return outs.fetch(ctx);
}

// ---- the conditioned start of the chain: the residuals' state at the end of the history, the setting, the mean ----

extern "C" int tsf_ar_last_out_size(void) { return (int)sizeof(tsf_ar_last_out); }

// What both tsf_residual_last entries check before anything is launched (tsf_residual_autocorr's refusals, and a ragged
// series whose row count does not fit last_gap); offsets and out are host memory in both.
static int check_ar_last_call(tsf_ctx *ctx, int64_t N, int32_t T, const int64_t *offsets, const void *y, int32_t y_dtype,
                              const double *fitted, const tsf_ar_last_out *out)
{
    if (N < 0 || N > (int64_t)INT32_MAX) return fail(ctx, "N must be in [0, 2^31 - 1]");
    if (!out || !out->last_resid || !out->last_gap || !out->status)
        return fail(ctx, "NULL output (tsf_ar_last_out, its last_resid, last_gap and status are required)");
    if (y_dtype < TSF_Y_F64 || y_dtype > TSF_Y_I32) return fail(ctx, "bad y_dtype");
    if (N > 0 && (!y || !fitted)) return fail(ctx, "NULL input (y and fitted are required)");
    if (!offsets) return T >= 1 ? 0 : fail(ctx, "bad panel (aligned: T >= 1)");
    if (offsets[0] != 0) return fail(ctx, "bad panel (ragged: offsets[0] = 0)");
    for (int64_t n = 0; n < N; ++n) {
        if (offsets[n + 1] < offsets[n]) return fail(ctx, "bad panel (ragged: offsets ascending)");
        if (offsets[n + 1] - offsets[n] > (int64_t)INT32_MAX) return fail(ctx, "bad panel (ragged: a series has more than 2^31 - 1 rows)");
    }
    return 0;
}

static int ar_last_run(tsf_ctx *ctx, int64_t N, int32_t T, const int64_t *d_off, const void *d_y, int32_t y_dtype,
                       const double *d_fit, const tsf_ar_last_out &o, hipStream_t st)
{
    if (N == 0) return 0;
    const ArLastArgs k = {d_y, d_fit, d_off, N, T, y_dtype, o.last_resid, o.last_gap, o.status};
    hipLaunchKernelGGL(ar_last_kernel, dim3((unsigned)((N + AR_WAVES - 1) / AR_WAVES)), dim3(AR_WAVES * 64), 0, st, k,
                       (int)TSF_AR_OK, (int)TSF_AR_NO_ROW);
    HIP_TRY(ctx, hipGetLastError());
    return 0;
}

extern "C" int tsf_residual_last_dev(tsf_ctx *ctx, int64_t N, int32_t T, const int64_t *offsets, const void *y,
                                     int32_t y_dtype, const double *fitted, tsf_ar_last_out *out, void *stream)
{
    if (!ctx) return -1;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (int rc = check_ar_last_call(ctx, N, T, offsets, y, y_dtype, fitted, out)) return rc;
    hipStream_t st = (hipStream_t)stream;
    DevBuf d_off;
    if (offsets && N > 0) HIP_TRY(ctx, d_off.put(offsets, 8 * ((size_t)N + 1)));
    if (int rc = ar_last_run(ctx, N, T, offsets ? d_off.as<int64_t>() : nullptr, y, y_dtype, fitted, *out, st)) return rc;
    HIP_TRY(ctx, hipStreamSynchronize(st));         // (the offsets go back to the pool)
    return 0;
}

extern "C" int tsf_residual_last(tsf_ctx *ctx, int64_t N, int32_t T, const int64_t *offsets, const void *y,
                                 int32_t y_dtype, const double *fitted, tsf_ar_last_out *out)
{
    if (!ctx) return -1;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (int rc = check_ar_last_call(ctx, N, T, offsets, y, y_dtype, fitted, out)) return rc;
    if (N == 0) return 0;
    const size_t rows = offsets ? (size_t)offsets[N] : (size_t)N * T, n = (size_t)N;
    DevBuf d_off, d_y, d_fit;
    HostOuts outs;
    if (offsets) HIP_TRY(ctx, d_off.put(offsets, 8 * (n + 1)));
    HIP_TRY(ctx, d_y.put(y, ysize(y_dtype) * rows));
    HIP_TRY(ctx, d_fit.put(fitted, 8 * rows));
    tsf_ar_last_out o;
    memset(&o, 0, sizeof(o));
    o.last_resid = outs.want(out->last_resid, 8 * n); o.last_gap = outs.want(out->last_gap, 4 * n);
    o.status = outs.want(out->status, 4 * n);
    if (int rc = outs.ready(ctx)) return rc;
    if (int rc = ar_last_run(ctx, N, T, offsets ? d_off.as<int64_t>() : nullptr, d_y.p, y_dtype, d_fit.as<double>(), o, nullptr))
        return rc;
    HIP_TRY(ctx, hipDeviceSynchronize());
    return outs.fetch(ctx);
}

// Both kernels on one copy of the panel: what tsf_residual_autocorr and tsf_residual_last return, each bit for bit, for
// the caller who wants both (the copy-in of y and fitted is most of either call).
extern "C" int tsf_residual_autocorr_last(tsf_ctx *ctx, int64_t N, int32_t T, const int64_t *offsets, const void *y,
                                          int32_t y_dtype, const double *fitted, const tsf_ar_args *args, tsf_ar_out *out,
                                          tsf_ar_last_out *last)
{
    if (!ctx) return -1;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    tsf_ar_args a;
    if (int rc = check_ar_call(ctx, N, T, offsets, y, y_dtype, fitted, args, out, &a)) return rc;
    if (int rc = check_ar_last_call(ctx, N, T, offsets, y, y_dtype, fitted, last)) return rc;
    if (N == 0) return 0;
    const size_t rows = offsets ? (size_t)offsets[N] : (size_t)N * T, n = (size_t)N;
    DevBuf d_off, d_y, d_fit;
    HostOuts outs;
    if (offsets) HIP_TRY(ctx, d_off.put(offsets, 8 * (n + 1)));
    HIP_TRY(ctx, d_y.put(y, ysize(y_dtype) * rows));
    HIP_TRY(ctx, d_fit.put(fitted, 8 * rows));
    tsf_ar_out o;
    memset(&o, 0, sizeof(o));
    o.phi = outs.want(out->phi, 8 * n); o.status = outs.want(out->status, 4 * n);
    o.phi_raw = outs.want(out->phi_raw, 8 * n); o.n_pairs = outs.want(out->n_pairs, 8 * n);
    o.scale = outs.want(out->scale, 8 * n);
    tsf_ar_last_out l;
    memset(&l, 0, sizeof(l));
    l.last_resid = outs.want(last->last_resid, 8 * n); l.last_gap = outs.want(last->last_gap, 4 * n);
    l.status = outs.want(last->status, 4 * n);
    if (int rc = outs.ready(ctx)) return rc;
    const int64_t *off = offsets ? d_off.as<int64_t>() : nullptr;
    if (int rc = ar_run(ctx, N, T, off, d_y.p, y_dtype, d_fit.as<double>(), a, o, nullptr)) return rc;
    if (int rc = ar_last_run(ctx, N, T, off, d_y.p, y_dtype, d_fit.as<double>(), l, nullptr)) return rc;
    HIP_TRY(ctx, hipDeviceSynchronize());
    return outs.fetch(ctx);
}

// ---- the noise state of a fitted panel in one pass, and the corrected point forecast (tsf_noise_state_kernels.h) ----

extern "C" int tsf_noise_state_out_size(void) { return (int)sizeof(tsf_noise_state_out); }

// A panel and its fit as tsf_noise_state takes them: host pointers in the host entry, device pointers behind it and in
// the `_dev` entry (offsets: host in both).
struct NoiseStateIn {
    int64_t N;
    int32_t T;
    const int64_t *offsets, *ds;
    const void *y;
    int32_t y_dtype;
    const double *floor_, *cap, *extra, *theta, *y_scale;
    const tsf_grid_info *grid;
    int32_t n_grids;
    const int32_t *status;
    const uint8_t *excluded;
};

// What both tsf_noise_state entries check before anything is launched and before anything is dereferenced but offsets:
// the panel checks of the two estimator entries, then (N > 0) tsf_predict's on the fit.  *a: the arguments in force.
static int check_noise_state_call(tsf_ctx *ctx, const tsf_spec *spec, const NoiseStateIn &in, const tsf_ar_args *args,
                                  const tsf_noise_state_out *out, tsf_ar_args *a)
{
    if (!out) return fail(ctx, "NULL output (tsf_noise_state_out)");
    // (the estimators' checks know y and fitted: y stands for both here, the fitted values are never materialised)
    const void *panel = in.N > 0 ? in.y : nullptr;
    const tsf_ar_out ar = {out->phi, out->phi_raw, out->n_pairs, out->scale, out->status};
    if (int rc = check_ar_call(ctx, in.N, in.T, in.offsets, panel, in.y_dtype, (const double *)panel, args, &ar, a)) return rc;
    const tsf_ar_last_out last = {out->last_resid, out->last_gap, out->last_status};
    if (int rc = check_ar_last_call(ctx, in.N, in.T, in.offsets, panel, in.y_dtype, (const double *)panel, &last)) return rc;
    if (in.N == 0) return 0;
    if (!spec || !in.ds || !in.theta || !in.y_scale || !in.grid || !in.status)
        return fail(ctx, "NULL input (spec, ds, theta, y_scale, grid and status are required)");
    if (in.n_grids != 1 && in.n_grids != in.N) return fail(ctx, "n_grids must be 1 or N");
    return 0;
}

// The launch on device-resident inputs; o: device pointers.  The spec goes to the context's copy in stream order first.
static int noise_state_run(tsf_ctx *ctx, const tsf_spec *spec, const NoiseStateIn &d, const int64_t *d_off, int64_t rows,
                           const tsf_ar_args &a, const tsf_noise_state_out &o, hipStream_t st)
{
    const ForecastIn f = {d.N, 1, d.theta, d.y_scale, d.grid, d.n_grids, d.ds, 0, d.floor_, d.cap, d.extra, nullptr};
    DevSpec hs;
    if (int rc = forecast_prologue(ctx, spec, f, st, &hs)) return rc;
    NoiseStateArgs k;
    memset(&k, 0, sizeof(k));
    k.sp = ctx->d_spec; k.N = d.N; k.T = d.T; k.y_dtype = d.y_dtype; k.theta_stride = tsf_theta_stride(spec);
    k.n_grids = d.n_grids; k.min_pairs = a.min_pairs; k.phi_max = a.phi_max;
    k.offsets = d_off; k.ds = d.ds; k.y = d.y; k.excluded = d.excluded; k.floor_ = d.floor_; k.cap = d.cap;
    k.extra = hs.n_extra > 0 ? d.extra : nullptr; k.extra_stride = d_off ? rows : (int64_t)d.T;
    k.theta = d.theta; k.y_scale = d.y_scale; k.grid = d.grid; k.fit_status = d.status;
    k.phi = o.phi; k.phi_raw = o.phi_raw; k.n_pairs = o.n_pairs; k.scale = o.scale; k.status = o.status;
    k.last_resid = o.last_resid; k.last_gap = o.last_gap; k.last_status = o.last_status; k.last_ds_ns = o.last_ds_ns;
    hipLaunchKernelGGL(noise_state_kernel, dim3((unsigned)((d.N + NS_WAVES - 1) / NS_WAVES)), dim3(NS_WAVES * 64), 0, st, k,
                       (int)TSF_AR_OK, (int)TSF_AR_NO_PAIRS, (int)TSF_AR_NO_ROW);
    HIP_TRY(ctx, hipGetLastError());
    return 0;
}

extern "C" int tsf_noise_state_dev(tsf_ctx *ctx, const tsf_spec *spec, int64_t N, int32_t T, const int64_t *offsets,
                                   const int64_t *ds, const void *y, int32_t y_dtype, const double *floor_,
                                   const double *cap, const double *extra, const double *theta, const double *y_scale,
                                   const tsf_grid_info *grid, int32_t n_grids, const int32_t *status,
                                   const uint8_t *excluded, const tsf_ar_args *args, tsf_noise_state_out *out, void *stream)
{
    if (!ctx) return -1;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const NoiseStateIn in = {N, T, offsets, ds, y, y_dtype, floor_, cap, extra, theta, y_scale, grid, n_grids, status, excluded};
    tsf_ar_args a;
    if (int rc = check_noise_state_call(ctx, spec, in, args, out, &a)) return rc;
    if (N == 0) return 0;
    hipStream_t st = (hipStream_t)stream;
    DevBuf d_off;
    if (offsets) HIP_TRY(ctx, d_off.put(offsets, 8 * ((size_t)N + 1)));
    if (int rc = noise_state_run(ctx, spec, in, offsets ? d_off.as<int64_t>() : nullptr, offsets ? offsets[N] : 0, a, *out, st))
        return rc;
    HIP_TRY(ctx, hipStreamSynchronize(st));         // (the offsets go back to the pool)
    return 0;
}

extern "C" int tsf_noise_state(tsf_ctx *ctx, const tsf_spec *spec, int64_t N, int32_t T, const int64_t *offsets,
                               const int64_t *ds, const void *y, int32_t y_dtype, const double *floor_, const double *cap,
                               const double *extra, const double *theta, const double *y_scale, const tsf_grid_info *grid,
                               int32_t n_grids, const int32_t *status, const uint8_t *excluded, const tsf_ar_args *args,
                               tsf_noise_state_out *out)
{
    if (!ctx) return -1;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const NoiseStateIn h = {N, T, offsets, ds, y, y_dtype, floor_, cap, extra, theta, y_scale, grid, n_grids, status, excluded};
    tsf_ar_args a;
    if (int rc = check_noise_state_call(ctx, spec, h, args, out, &a)) return rc;
    if (N == 0) return 0;
    const size_t n = (size_t)N, rows = offsets ? (size_t)offsets[N] : n * T, nds = offsets ? rows : (size_t)T;
    {   // what only a host entry can see: the spec against the inputs, the grids the kernel will read, the marks
        const ForecastIn f = {N, 1, theta, y_scale, grid, n_grids, ds, 0, floor_, cap, extra, nullptr};
        DevSpec hs;
        if (int rc = forecast_spec(ctx, spec, f, &hs)) return rc;
        if (int rc = check_grids(ctx, spec, grid, n_grids, status, N)) return rc;
        if (excluded)
            for (size_t i = 0; i < rows; ++i)
                if (excluded[i] > 1) return fail(ctx, "excluded holds a value other than 0 / 1");
    }
    NoiseStateIn d = h;
    DevBuf d_off, d_ds, d_y, d_ex, d_fl, d_cap, d_x, d_th, d_ys, d_grid, d_st;
    if (offsets) HIP_TRY(ctx, d_off.put(offsets, 8 * (n + 1)));
    if (int rc = ForecastUpload::put(ctx, &d_ds, ds, 8 * nds, &d.ds)) return rc;
    HIP_TRY(ctx, d_y.put(y, ysize(y_dtype) * rows));
    d.y = d_y.p;
    if (int rc = ForecastUpload::put(ctx, &d_ex, excluded, rows, &d.excluded)) return rc;
    if (int rc = ForecastUpload::put(ctx, &d_fl, floor_, 8 * n, &d.floor_)) return rc;
    if (int rc = ForecastUpload::put(ctx, &d_cap, cap, 8 * n, &d.cap)) return rc;
    if (spec->n_extra == 0) d.extra = nullptr;
    else if (int rc = ForecastUpload::put(ctx, &d_x, extra, 8 * (size_t)spec->n_extra * nds, &d.extra)) return rc;
    if (int rc = ForecastUpload::put(ctx, &d_th, theta, 8 * n * tsf_theta_stride(spec), &d.theta)) return rc;
    if (int rc = ForecastUpload::put(ctx, &d_ys, y_scale, 8 * n, &d.y_scale)) return rc;
    if (int rc = ForecastUpload::put(ctx, &d_grid, grid, sizeof(tsf_grid_info) * (size_t)n_grids, &d.grid)) return rc;
    if (int rc = ForecastUpload::put(ctx, &d_st, status, 4 * n, &d.status)) return rc;
    HostOuts outs;
    tsf_noise_state_out o;
    memset(&o, 0, sizeof(o));
    o.phi = outs.want(out->phi, 8 * n); o.status = outs.want(out->status, 4 * n);
    o.phi_raw = outs.want(out->phi_raw, 8 * n); o.n_pairs = outs.want(out->n_pairs, 8 * n);
    o.scale = outs.want(out->scale, 8 * n); o.last_resid = outs.want(out->last_resid, 8 * n);
    o.last_gap = outs.want(out->last_gap, 4 * n); o.last_status = outs.want(out->last_status, 4 * n);
    o.last_ds_ns = outs.want(out->last_ds_ns, 8 * n);
    if (int rc = outs.ready(ctx)) return rc;
    if (int rc = noise_state_run(ctx, spec, d, offsets ? d_off.as<int64_t>() : nullptr, (int64_t)rows, a, o, nullptr)) return rc;
    HIP_TRY(ctx, hipDeviceSynchronize());
    return outs.fetch(ctx);
}

// phi, resid, steps of tsf_predict_conditioned (host memory in both variants), checked as tsf_set_noise_ar and
// tsf_set_noise_ar_start check them; *pm: (phi, m0 = resid * phi^steps) per series, tsf_noise_ar_mean's first row.
static int conditioned_pairs(tsf_ctx *ctx, int64_t N, const double *phi, const double *resid, const int32_t *steps,
                             std::vector<double> *pm)
{
    if (!phi || !resid || !steps) return fail(ctx, "NULL input (phi, resid and steps are required)");
    char msg[160];
    for (int64_t i = 0; i < N; ++i) {
        if (!(std::fabs(phi[i]) < 1.0)) {
            snprintf(msg, sizeof(msg), "phi[%lld] = %g: each phi must be finite with |phi| < 1", (long long)i, phi[i]);
            return fail(ctx, msg);
        }
        if (!std::isfinite(resid[i])) {
            snprintf(msg, sizeof(msg), "resid[%lld] = %g: a residual must be finite", (long long)i, resid[i]);
            return fail(ctx, msg);
        }
        if (steps[i] < 1) {
            snprintf(msg, sizeof(msg), "steps[%lld] = %d: the first future row lies at least one row behind the last residual",
                     (long long)i, (int)steps[i]);
            return fail(ctx, msg);
        }
    }
    try {
        pm->resize(2 * (size_t)N);
    } catch (const std::bad_alloc &) {
        return fail(ctx, "tsf_predict_conditioned: out of host memory");
    }
    for (int64_t i = 0; i < N; ++i) {
        (*pm)[2 * (size_t)i] = phi[i];
        (*pm)[2 * (size_t)i + 1] = resid[i] * ar_start_p0(phi[i], steps[i]);
    }
    return 0;
}

extern "C" int tsf_predict_conditioned_dev(tsf_ctx *ctx, const tsf_spec *spec, int64_t N, int32_t H, const double *theta,
                                           const double *y_scale, const tsf_grid_info *grid, int32_t n_grids,
                                           const int64_t *ds_future, int32_t shared_future, const double *floor_,
                                           const double *cap, const double *extra_future, const double *phi,
                                           const double *resid, const int32_t *steps, double *yhat, int32_t *yhat_int,
                                           void *stream)
{
    if (!ctx) return -1;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const ForecastIn f = {N, H, theta, y_scale, grid, n_grids, ds_future, shared_future, floor_, cap, extra_future, nullptr};
    if (int rc = check_forecast_in(ctx, f, spec && yhat)) return rc;
    std::vector<double> pm;
    if (int rc = conditioned_pairs(ctx, N, phi, resid, steps, &pm)) return rc;
    hipStream_t st = (hipStream_t)stream;
    DevSpec hs;
    if (int rc = forecast_prologue(ctx, spec, f, st, &hs)) return rc;
    DevBuf d_pm;
    HIP_TRY(ctx, d_pm.put(pm.data(), 8 * pm.size()));
    PredictArgs a = predict_args(ctx, spec, f, yhat);
    bool tab_ready = false;
    if (int rc = launch_predict(ctx, hs, a, 0, N, &tab_ready, st)) return rc;
    const ConditionedArgs c = {d_pm.as<double>(), floor_, yhat, yhat_int, N, H};
    const int64_t cells = N * (int64_t)H;
    hipLaunchKernelGGL(conditioned_shift_kernel, dim3((unsigned)((cells + 255) / 256)), dim3(256), 0, st, c);
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, hipStreamSynchronize(st));         // (the pairs go back to the pool)
    return 0;
}

extern "C" int tsf_predict_conditioned(tsf_ctx *ctx, const tsf_spec *spec, int64_t N, int32_t H, const double *theta,
                                       const double *y_scale, const tsf_grid_info *grid, int32_t n_grids,
                                       const int64_t *ds_future, int32_t shared_future, const double *floor_,
                                       const double *cap, const double *extra_future, const double *phi,
                                       const double *resid, const int32_t *steps, double *yhat, int32_t *yhat_int)
{
    if (!ctx) return -1;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const ForecastIn h = {N, H, theta, y_scale, grid, n_grids, ds_future, shared_future, floor_, cap, extra_future, nullptr};
    if (int rc = check_forecast_in(ctx, h, spec && yhat)) return rc;
    if (int rc = check_grids(ctx, spec, grid, n_grids)) return rc;
    {
        std::vector<double> pm;     // (checked here too: a refusal comes before anything is copied)
        if (int rc = conditioned_pairs(ctx, N, phi, resid, steps, &pm)) return rc;
    }
    ForecastUpload up;
    if (int rc = up.upload(ctx, spec, h)) return rc;
    const ForecastIn &d = up.dev;
    DevBuf d_yh, d_yi;
    HIP_TRY(ctx, d_yh.alloc(8 * (size_t)N * H));
    if (yhat_int) HIP_TRY(ctx, d_yi.alloc(4 * (size_t)N * H));
    if (int rc = tsf_predict_conditioned_dev(ctx, spec, N, H, d.theta, d.y_scale, d.grid, n_grids, d.ds_future, shared_future,
                                             d.floor_, d.cap, d.extra_future, phi, resid, steps, d_yh.as<double>(),
                                             yhat_int ? d_yi.as<int32_t>() : nullptr, nullptr))
        return rc;
    HIP_TRY(ctx, hipDeviceSynchronize());
    HIP_TRY(ctx, hipMemcpy(yhat, d_yh.p, 8 * (size_t)N * H, hipMemcpyDeviceToHost));
    if (yhat_int) HIP_TRY(ctx, hipMemcpy(yhat_int, d_yi.p, 4 * (size_t)N * H, hipMemcpyDeviceToHost));
    return 0;
}

extern "C" int tsf_set_noise_ar_start(tsf_ctx *ctx, const double *resid, const int32_t *steps, int64_t n)
{
    if (!ctx) return -1;
    ctx->ar_start_pending.clear();
    if (!resid || !steps || n <= 0) return 0;
    char msg[200];
    if (ctx->ar_pending.size() != 2 * (size_t)n) {
        const long long pending = (long long)(ctx->ar_pending.size() / 2);
        ctx->ar_pending.clear();
        if (pending == 0)
            return fail(ctx, "tsf_set_noise_ar_start: no tsf_set_noise_ar setting is pending (phi first, then the start)");
        snprintf(msg, sizeof(msg), "tsf_set_noise_ar_start was given %lld series and the pending tsf_set_noise_ar setting has "
                 "%lld (the setting is cleared)", (long long)n, pending);
        return fail(ctx, msg);
    }
    for (int64_t i = 0; i < n; ++i) {
        if (!std::isfinite(resid[i])) {
            snprintf(msg, sizeof(msg), "resid[%lld] = %g: a residual must be finite (the setting is cleared)", (long long)i, resid[i]);
            ctx->ar_pending.clear();
            return fail(ctx, msg);
        }
        if (steps[i] < 1) {
            snprintf(msg, sizeof(msg), "steps[%lld] = %d: the first future row lies at least one row behind the last residual "
                     "(the setting is cleared)", (long long)i, (int)steps[i]);
            ctx->ar_pending.clear();
            return fail(ctx, msg);
        }
    }
    try {
        ctx->ar_start_pending.resize(3 * (size_t)n);
    } catch (const std::bad_alloc &) {
        ctx->ar_start_pending.clear();
        ctx->ar_pending.clear();
        return fail(ctx, "tsf_set_noise_ar_start: out of host memory");
    }
    for (int64_t i = 0; i < n; ++i) {
        const double p0 = ar_start_p0(ctx->ar_pending[2 * (size_t)i], steps[i]);
        ctx->ar_start_pending[3 * (size_t)i] = p0;
        ctx->ar_start_pending[3 * (size_t)i + 1] = std::sqrt(1.0 - p0 * p0);
        ctx->ar_start_pending[3 * (size_t)i + 2] = resid[i] * p0;
    }
    return 0;
}

extern "C" int tsf_set_noise_ar(tsf_ctx *ctx, const double *phi, int64_t n)
{
    if (!ctx) return -1;
    ctx->ar_start_pending.clear();
    ctx->ar_pending.clear();
    if (!phi || n <= 0) return 0;
    for (int64_t i = 0; i < n; ++i)
        if (!(std::fabs(phi[i]) < 1.0)) {            // (NaN fails the comparison)
            char msg[120];
            snprintf(msg, sizeof(msg), "phi[%lld] = %g: an autocorrelation must be finite with |phi| < 1", (long long)i, phi[i]);
            return fail(ctx, msg);
        }
    try {
        ctx->ar_pending.resize(2 * (size_t)n);
    } catch (const std::bad_alloc &) {
        ctx->ar_pending.clear();
        return fail(ctx, "tsf_set_noise_ar: out of host memory");
    }
    for (int64_t i = 0; i < n; ++i) {
        ctx->ar_pending[2 * (size_t)i] = phi[i];
        ctx->ar_pending[2 * (size_t)i + 1] = std::sqrt(1.0 - phi[i] * phi[i]);
    }
    return 0;
}

extern "C" int tsf_rollup_set_noise_corr(tsf_rollup *r, const double *rho, const int64_t *group_key)
{
    if (int rc = rollup_enter(r)) return rc;
    tsf_ctx *ctx = r->ctx;
    if (r->added || r->top.T)
        return fail(ctx, "tsf_rollup_set_noise_corr after a tsf_rollup_add or tsf_rollup_set_totals: a correlation is set on an "
                         "empty roll-up");
    if (!rho) return fail(ctx, "NULL rho");
    const size_t G = (size_t)r->G;
    for (size_t g = 0; g < G; ++g)
        if (!(rho[g] >= 0.0 && rho[g] <= 1.0)) {
            char msg[120];
            snprintf(msg, sizeof(msg), "rho[%lld] = %g: a correlation must be finite and in [0, 1]", (long long)g, rho[g]);
            return fail(ctx, msg);
        }
    std::vector<double> ab;
    std::vector<int64_t> key;
    try {
        ab.resize(2 * G);
        key.resize(G);
    } catch (const std::bad_alloc &) {
        return fail(ctx, "tsf_rollup_set_noise_corr: out of host memory");
    }
    for (size_t g = 0; g < G; ++g) {
        ab[g] = std::sqrt(1.0 - rho[g]) - 1.0;
        ab[G + g] = std::sqrt(rho[g]);
        key[g] = group_key ? group_key[g] : (int64_t)g;
    }
    // (the tables are the handle's from their allocation on, whatever fails behind it)
    const hipError_t e = [&]() -> hipError_t {
        if (!r->d_corr_ab) HIP_OK(r->d_corr_ab.alloc(2 * G));
        if (!r->d_group_key) HIP_OK(r->d_group_key.alloc(G));
        HIP_OK(hipMemcpy(r->d_corr_ab, ab.data(), 16 * G, hipMemcpyHostToDevice));
        return hipMemcpy(r->d_group_key, key.data(), 8 * G, hipMemcpyHostToDevice);
    }();
    if (e != hipSuccess) {
        if (r->corr) r->poisoned = true;        // (an earlier table may be half overwritten)
        return rollup_hip_fail(ctx, "tsf_rollup_set_noise_corr", e);
    }
    r->corr_a.assign(ab.begin(), ab.begin() + (std::ptrdiff_t)G);
    r->corr_b.assign(ab.begin() + (std::ptrdiff_t)G, ab.end());
    r->group_key.swap(key);
    r->corr = true;
    return 0;
}

// What a read of a roll-up checks of its outputs and levels (those of a tsf_rollup_out or a tsf_reconcile_out):
// tsf_predict_quantiles' checks, with the handle's sample count.
static int check_rollup_read(tsf_rollup *r, int32_t n_q, const double *quantiles, double *yhat, double *q, double *cum_q,
                             double *samples)
{
    tsf_quantile_out chk;
    memset(&chk, 0, sizeof(chk));
    chk.yhat = yhat; chk.q = q; chk.cum_q = cum_q; chk.samples = samples;
    return check_quantile_args(r->ctx, r->S, n_q, quantiles, &chk);
}

// The read of every group's cells behind tsf_rollup_quantiles and tsf_rollup_reconciled_totals (which has put yhat into
// `outs`), a range of groups at a time.  Without `total` the cells are the accumulators: q is sorted from them in place,
// a range being what quantile_kernel's grid (groups * H) takes, and the samples are the accumulators themselves.  With
// it, reconcile_total_kernel first writes a range's cells into the context's scratch (its out and g0 are set here): q is
// sorted from there, and the samples leave the scratch range by range in stream order.  In both, the running sums of a
// range for cum_q lie in the scratch as well, and a range is what keeps the scratch within its 512 MB.
//
// cells_read is that read over any G cells [G][H][S] the handle holds (`acc`: the accumulators, or a level of a solved
// tree); `make` (null: the cells are `acc` itself) launches what writes the cells g0 .. g0 + gc into the scratch at dst.
using CellMaker = std::function<int(double *dst, int64_t g0, int64_t gc)>;

static int cells_read(tsf_rollup *r, const double *acc, int64_t G, int32_t n_q, const double *quantiles,
                      const tsf_rollup_out &out, const CellMaker *make, HostOuts &outs)
{
    tsf_ctx *ctx = r->ctx;
    const int32_t H = r->H, S = r->S;
    const size_t hs = (size_t)H * S, gh = (size_t)G * H, nqh = 8 * gh * (size_t)n_q;
    const QuantilePass qp(H, S, n_q, quantiles);
    double *d_q = outs.want(out.q, nqh), *d_cq = outs.want(out.cum_q, nqh);
    if (!make) outs.adopt(out.samples, const_cast<double *>(acc), 8 * gh * S);
    if (int rc = outs.ready(ctx)) return rc;
    if (d_q && !make) {
        const int64_t range = std::max<int64_t>(1, ((int64_t)1 << 30) / H);
        for (int64_t g0 = 0; g0 < G; g0 += range)
            if (int rc = qp.launch(ctx, acc + (size_t)g0 * hs, d_q, g0, std::min(range, G - g0), nullptr)) return rc;
    }
    const size_t n_buf = (make ? 1 : 0) + (d_cq ? 1 : 0);       // per range in the scratch: the cells, their running sums
    if (n_buf) {
        const int64_t range = std::max<int64_t>(1, std::min<int64_t>(G, (int64_t)(((size_t)512 << 20) / (8 * hs * n_buf))));
        if (int rc = ensure_iv_ws(ctx, 8 * (size_t)range * hs * n_buf)) return rc;
        double *d_x = (double *)ctx->iv_ws, *d_c = make ? d_x + (size_t)range * hs : d_x;
        for (int64_t g0 = 0; g0 < G; g0 += range) {
            const int64_t gc = std::min(range, G - g0);
            const double *cells = make ? d_x : acc + (size_t)g0 * hs;
            if (make) {
                if (int rc = (*make)(d_x, g0, gc)) return rc;
                if (d_q)
                    if (int rc = qp.launch(ctx, d_x, d_q, g0, gc, nullptr)) return rc;
            }
            if (d_cq) {
                hipLaunchKernelGGL(rollup_cumsum_kernel, dim3((unsigned)((gc * S + 255) / 256)), dim3(256), 0, nullptr,
                                   cells, d_c, gc, H, S);
                HIP_TRY(ctx, hipGetLastError());
                if (int rc = qp.launch(ctx, d_c, d_cq, g0, gc, nullptr)) return rc;
            }
            if (make && out.samples)
                HIP_TRY(ctx, hipMemcpyAsync(out.samples + (size_t)g0 * hs, d_x, 8 * (size_t)gc * hs, hipMemcpyDeviceToHost,
                                            nullptr));
        }
    }
    HIP_TRY(ctx, hipDeviceSynchronize());
    return outs.fetch(ctx);
}

static int rollup_read(tsf_rollup *r, int32_t n_q, const double *quantiles, const tsf_rollup_out &out,
                       ReconcileTotalArgs *total, HostOuts &outs)
{
    tsf_ctx *ctx = r->ctx;
    const int32_t H = r->H, S = r->S;
    const CellMaker make = [&](double *dst, int64_t g0, int64_t gc) -> int {
        total->out = dst; total->g0 = g0;
        hipLaunchKernelGGL(reconcile_total_kernel, dim3((unsigned)(gc * H), (unsigned)((S + 255) / 256)), dim3(256), 0,
                           nullptr, *total);
        HIP_TRY(ctx, hipGetLastError());
        return 0;
    };
    if (int rc = cells_read(r, r->acc, r->G, n_q, quantiles, out, total ? &make : nullptr, outs)) return rc;
    if (out.count) memcpy(out.count, r->count.data(), 8 * (size_t)r->G);
    return 0;
}

extern "C" int tsf_rollup_quantiles(tsf_rollup *r, int32_t n_q, const double *quantiles, tsf_rollup_out *out)
{
    if (int rc = rollup_enter(r)) return rc;
    tsf_ctx *ctx = r->ctx;
    if (!out) return fail(ctx, "NULL output (tsf_rollup_out and its yhat are required)");
    if (int rc = check_rollup_read(r, n_q, quantiles, out->yhat, out->q, out->cum_q, out->samples)) return rc;
    HostOuts outs;
    outs.adopt(out->yhat, r->ysum.p, 8 * (size_t)r->G * r->H);
    return rollup_read(r, n_q, quantiles, *out, nullptr, outs);
}

// ---- totals over row windows: quantiles and scores of calendar-period totals ---------------------------------

extern "C" int tsf_window_out_size(void) { return (int)sizeof(tsf_window_out); }

// the outputs that are read from the sorted window sums: they need the draws (of a roll-up: the accumulators)
static bool window_wants_draws(const tsf_window_out &o)
{
    return o.q || o.pit || o.crps || o.pinball || o.mean_crps || o.mean_pinball || o.coverage;
}

// the window checks of tsf_shares.cpp (WindowCall: tsf_shares.h), their message left in the context
static int check_windows(tsf_ctx *ctx, int32_t H, const WindowCall &w)
{
    char msg[WINDOW_MSG];
    return check_windows(H, w, msg) ? fail(ctx, msg) : 0;
}
static int check_disjoint_windows(tsf_ctx *ctx, int32_t H, const WindowCall &w)
{
    char msg[WINDOW_MSG];
    return check_disjoint_windows(H, w, msg) ? fail(ctx, msg) : 0;
}

// What the three window entries check before anything is copied or launched: tsf_predict_quantiles' checks of the sample
// count and the levels, the windows against H, and what the outputs need.
static int check_window_args(tsf_ctx *ctx, int32_t H, int32_t n_samples, int32_t n_q, const double *quantiles,
                             const WindowCall &w, const tsf_window_out *out)
{
    if (!out) return fail(ctx, "NULL output (tsf_window_out is required)");
    if (int rc = check_samples_and_levels(ctx, n_samples, n_q, quantiles)) return rc;
    if (int rc = check_windows(ctx, H, w)) return rc;
    const bool want_q = out->q || out->pinball || out->mean_pinball || out->coverage;
    const bool want_score = out->pit || out->crps || out->pinball || out->n_obs || out->mean_crps || out->mean_pinball ||
                            out->coverage;
    if (!out->yhat && !out->total && !want_q && !want_score)
        return fail(ctx, "nothing requested: every output of tsf_window_out is NULL");
    if (n_q == 0 && want_q) return fail(ctx, "n_q = 0 with q, pinball, mean_pinball or coverage requested");
    if (want_score && !w.y_win) return fail(ctx, "NULL y_win with a score output requested");
    return 0;
}

// the host-pointer entries: an observed total is finite or NaN
static int check_y_win(tsf_ctx *ctx, const double *y_win, int64_t N, int32_t K)
{
    const size_t nk = (size_t)N * K;
    for (size_t i = 0; y_win && i < nk; ++i)
        if (std::isinf(y_win[i])) {
            char msg[120];
            snprintf(msg, sizeof(msg), "y_win[%lld][%d] is infinite: an observed total must be finite (NaN = not observed)",
                     (long long)(i / K), (int)(i % K));
            return fail(ctx, msg);
        }
    return 0;
}

// window_score_kernel's arguments for the whole call, with what lies in the context's sample scratch behind its first
// `base` bytes (the chunk draw_chunks carves from it: the block is sized for both here, so draw_chunks never
// reallocates under them): the per-window arrays the aggregates read where the caller did not ask for them, yhat where
// it is needed and not asked for, and the windows themselves (copied from the caller's host arrays before this
// returns, as forecast_prologue's copy of the spec is).  Every pointer of `o` and w.y_win are device pointers.
static int window_prepare(tsf_ctx *ctx, size_t base, int64_t N, int32_t H, int32_t n_samples, const QuantileCall &c,
                          const WindowCall &w, const tsf_window_out &o, bool need_yhat, hipStream_t st, WindowArgs *a,
                          double **yhat)
{
    const size_t nk = (size_t)N * w.K, nqk = nk * (size_t)c.n_q;
    const size_t extra = (o.mean_crps && !o.crps ? nk : 0) + (o.mean_pinball && !o.pinball ? nqk : 0) +
                         (o.coverage && !o.q ? nqk : 0) + (need_yhat && !o.yhat ? (size_t)N * H : 0);
    if (int rc = ensure_iv_ws(ctx, base + 8 * extra + 8 * (size_t)w.K)) return rc;
    double *d_next = (double *)((char *)ctx->iv_ws + base);
    memset(a, 0, sizeof(*a));
    a->y = w.y_win; a->pit = o.pit; a->crps = o.crps; a->q = o.q; a->pinball = o.pinball;
    a->H = H; a->K = w.K; a->NS = n_samples; a->n_q = c.n_q;
    for (int32_t i = 0; i < c.n_q; ++i) a->level[i] = c.quantiles[i];
    if (o.mean_crps && !o.crps) { a->crps = d_next; d_next += nk; }
    if (o.mean_pinball && !o.pinball) { a->pinball = d_next; d_next += nqk; }
    if (o.coverage && !o.q) { a->q = d_next; d_next += nqk; }
    *yhat = o.yhat;
    if (need_yhat && !o.yhat) { *yhat = d_next; d_next += (size_t)N * H; }
    int32_t *d_w = (int32_t *)d_next;
    HIP_TRY(ctx, hipMemcpyAsync(d_w, w.win_start, 4 * (size_t)w.K, hipMemcpyHostToDevice, st));
    HIP_TRY(ctx, hipMemcpyAsync(d_w + w.K, w.win_end, 4 * (size_t)w.K, hipMemcpyHostToDevice, st));
    a->w0 = d_w; a->w1 = d_w + w.K;
    return 0;
}

// window_score_kernel over the n series (groups) whose samples start at src, the first of them series n0 of the call;
// a range of series per launch (the grid is series * K)
static int launch_window_scores(tsf_ctx *ctx, WindowArgs a, const double *src, int64_t n0, int64_t n, hipStream_t st)
{
    const int NSP = sort_width(a.NS);
    const int64_t range = std::max<int64_t>(1, ((int64_t)1 << 30) / a.K);
    for (int64_t i0 = 0; i0 < n; i0 += range) {
        const int64_t nc = std::min(range, n - i0);
        a.src = src + (size_t)i0 * a.H * a.NS; a.n0 = n0 + i0;
        hipLaunchKernelGGL(window_score_kernel, dim3((unsigned)(nc * a.K)), dim3(256), sizeof(double) * NSP, st, a, NSP);
        HIP_TRY(ctx, hipGetLastError());
    }
    return 0;
}

// what follows the window scores: the point totals from yhat, the per-series means by score_series_kernel with the
// windows in the place of the rows
static int window_finish(tsf_ctx *ctx, const WindowArgs &a, const double *yhat, int64_t N, const tsf_window_out &o,
                         hipStream_t st)
{
    if (o.total) {
        const int64_t threads = N * a.K;
        hipLaunchKernelGGL(window_total_kernel, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, st, yhat, a.w0, a.w1,
                           o.total, N, a.H, a.K);
        HIP_TRY(ctx, hipGetLastError());
    }
    if (o.n_obs || o.mean_crps || o.mean_pinball || o.coverage) {
        ScoreSeriesArgs s;
        memset(&s, 0, sizeof(s));
        s.y = a.y; s.crps = a.crps; s.q = a.q; s.pinball = a.pinball;
        s.n_obs = o.n_obs; s.mean_crps = o.mean_crps; s.mean_pinball = o.mean_pinball; s.coverage = o.coverage;
        s.N = N; s.H = a.K; s.n_q = a.n_q;
        const int64_t threads = N * (1 + a.n_q);
        hipLaunchKernelGGL(score_series_kernel, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, st, s);
        HIP_TRY(ctx, hipGetLastError());
    }
    return 0;
}

// The work of both tsf_predict_windows entries on device-resident inputs.
static int predict_windows_run(tsf_ctx *ctx, const tsf_spec *spec, const ForecastIn &f, const QuantileCall &c,
                               const WindowCall &w, const tsf_window_out &o, hipStream_t st)
{
    const int64_t N = f.N;
    const int32_t H = f.H, n_samples = c.n_samples;
    const bool draws = window_wants_draws(o), need_yhat = draws || o.yhat || o.total;
    const size_t base = draws ? draw_scratch_bytes(draw_chunk_series(N, H, n_samples, 1), H, n_samples, 1) : 0;
    WindowArgs a;
    double *yhat = nullptr;
    if (int rc = window_prepare(ctx, base, N, H, n_samples, c, w, o, need_yhat, st, &a, &yhat)) return rc;
    if (draws) {
        auto after = [&](int64_t n0, int64_t nc, const DrawBufs &b) -> int {
            return launch_window_scores(ctx, a, b.samp, n0, nc, st);
        };
        const DrawSpec d = {n_samples, c.seed, false, false, yhat, nullptr, true};
        if (int rc = draw_chunks(ctx, spec, f, d, st, after)) return rc;
    } else if (need_yhat) {
        if (int rc = tsf_predict_dev(ctx, spec, N, H, f.theta, f.y_scale, f.grid, f.n_grids, f.ds_future, f.shared_future,
                                     f.floor_, f.cap, f.extra_future, yhat, nullptr, st))
            return rc;
    }
    return window_finish(ctx, a, yhat, N, o, st);
}

extern "C" int tsf_predict_windows_dev(tsf_ctx *ctx, const tsf_spec *spec, int64_t N, int32_t H, const double *theta,
                                       const double *y_scale, const tsf_grid_info *grid, int32_t n_grids,
                                       const int64_t *ds_future, int32_t shared_future, const double *floor_,
                                       const double *cap, const double *extra_future, const int64_t *series_key,
                                       int32_t n_samples, uint64_t seed, int32_t K, const int32_t *win_start,
                                       const int32_t *win_end, const double *y_win, int32_t n_q, const double *quantiles,
                                       tsf_window_out *out, void *stream)
{
    if (!ctx) return -1;
    NoiseArOnce ar_once(ctx);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const ForecastIn f = {N, H, theta, y_scale, grid, n_grids, ds_future, shared_future, floor_, cap, extra_future, series_key};
    if (int rc = check_forecast_in(ctx, f, spec != nullptr)) return rc;
    const WindowCall w = {K, win_start, win_end, y_win};
    if (int rc = check_window_args(ctx, H, n_samples, n_q, quantiles, w, out)) return rc;
    return predict_windows_run(ctx, spec, f, {n_samples, seed, n_q, quantiles}, w, *out, (hipStream_t)stream);
}

// The outputs of a host-pointer window entry over N series (groups) on the device: each field `h` asks for, at its size.
// yhat_dev: the entry has yhat on the device already (the roll-up's ysum) and no buffer is taken for it.
static tsf_window_out window_dev_outs(HostOuts &outs, const tsf_window_out &h, int64_t N, int32_t H, int32_t K, int32_t n_q,
                                      double *yhat_dev)
{
    const size_t nh = 8 * (size_t)N * H, nk = 8 * (size_t)N * K, nqk = nk * (size_t)n_q, nq = 8 * (size_t)N * n_q;
    tsf_window_out o;
    memset(&o, 0, sizeof(o));
    o.yhat = yhat_dev ? outs.adopt(h.yhat, yhat_dev, nh) : outs.want(h.yhat, nh);
    o.total = outs.want(h.total, nk); o.q = outs.want(h.q, nqk);
    o.pit = outs.want(h.pit, nk); o.crps = outs.want(h.crps, nk); o.pinball = outs.want(h.pinball, nqk);
    o.n_obs = outs.want(h.n_obs, 4 * (size_t)N); o.mean_crps = outs.want(h.mean_crps, 8 * (size_t)N);
    o.mean_pinball = outs.want(h.mean_pinball, nq); o.coverage = outs.want(h.coverage, nq);
    return o;
}

extern "C" int tsf_predict_windows(tsf_ctx *ctx, const tsf_spec *spec, int64_t N, int32_t H, const double *theta,
                                   const double *y_scale, const tsf_grid_info *grid, int32_t n_grids,
                                   const int64_t *ds_future, int32_t shared_future, const double *floor_, const double *cap,
                                   const double *extra_future, const int64_t *series_key, int32_t n_samples, uint64_t seed,
                                   int32_t K, const int32_t *win_start, const int32_t *win_end, const double *y_win,
                                   int32_t n_q, const double *quantiles, tsf_window_out *out)
{
    if (!ctx) return -1;
    NoiseArOnce ar_once(ctx);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const ForecastIn h = {N, H, theta, y_scale, grid, n_grids, ds_future, shared_future, floor_, cap, extra_future, series_key};
    if (int rc = check_forecast_in(ctx, h, spec != nullptr)) return rc;
    if (int rc = check_grids(ctx, spec, grid, n_grids)) return rc;
    const WindowCall hw = {K, win_start, win_end, y_win};
    if (int rc = check_window_args(ctx, H, n_samples, n_q, quantiles, hw, out)) return rc;
    if (spec->n_extra > 0 && !extra_future) return fail(ctx, "extra_future is NULL");     // (ahead of the scan of y_win)
    if (int rc = check_y_win(ctx, y_win, N, K)) return rc;
    ForecastUpload up;
    if (int rc = up.upload(ctx, spec, h)) return rc;
    DevBuf d_y;
    HostOuts outs;
    WindowCall w = hw;
    if (y_win) { HIP_TRY(ctx, d_y.put(y_win, 8 * (size_t)N * K)); w.y_win = d_y.as<double>(); }
    const tsf_window_out o = window_dev_outs(outs, *out, N, H, K, n_q, nullptr);
    if (int rc = outs.ready(ctx)) return rc;
    if (int rc = predict_windows_run(ctx, spec, up.dev, {n_samples, seed, n_q, quantiles}, w, o, nullptr)) return rc;
    HIP_TRY(ctx, hipDeviceSynchronize());
    return outs.fetch(ctx);
}

extern "C" int tsf_rollup_windows(tsf_rollup *r, int32_t K, const int32_t *win_start, const int32_t *win_end,
                                  const double *y_win, int32_t n_q, const double *quantiles, tsf_window_out *out)
{
    if (int rc = rollup_enter(r)) return rc;
    tsf_ctx *ctx = r->ctx;
    const int32_t H = r->H, S = r->S;
    const int64_t G = r->G;
    const WindowCall hw = {K, win_start, win_end, y_win};
    if (int rc = check_window_args(ctx, H, S, n_q, quantiles, hw, out)) return rc;
    if (int rc = check_y_win(ctx, y_win, G, K)) return rc;
    // the accumulators are read in place, a group in the place of a series; yhat is the handle's ysum
    DevBuf d_y;
    HostOuts outs;
    WindowCall w = hw;
    if (y_win) { HIP_TRY(ctx, d_y.put(y_win, 8 * (size_t)G * K)); w.y_win = d_y.as<double>(); }
    const tsf_window_out o = window_dev_outs(outs, *out, G, H, K, n_q, r->ysum);
    if (int rc = outs.ready(ctx)) return rc;
    WindowArgs a;
    double *yhat = nullptr;
    if (int rc = window_prepare(ctx, 0, G, H, S, {S, r->seed, n_q, quantiles}, w, o, false, nullptr, &a, &yhat)) return rc;
    if (window_wants_draws(o))
        if (int rc = launch_window_scores(ctx, a, r->acc, 0, G, nullptr)) return rc;
    if (int rc = window_finish(ctx, a, r->ysum, G, o, nullptr)) return rc;
    HIP_TRY(ctx, hipDeviceSynchronize());
    return outs.fetch(ctx);
}

// ---- reconciliation: member forecasts and fitted totals made coherent ---------------------------------------

extern "C" int tsf_reconcile_out_size(void) { return (int)sizeof(tsf_reconcile_out); }

// (tsf_reconcile_shares, the host-only solver of the shares: tsf_shares.cpp)

// The two steps of tsf_rollup_set_totals and tsf_rollup_set_node_totals once the call's series are checked, for the
// totals c of a level of n slots (`noun`s: c.group names each total's slot) kept in *f.
// Claim: a slot takes one total, ever -- *has = the level's flags with this call's set; the level's buffers are
// allocated by its first call.  Nothing of the handle's has changed yet but that.
static int fitted_totals_claim(tsf_rollup *r, const char *entry, const char *noun, FittedTotals *f, int64_t n,
                               const RollupCall &c, std::vector<int32_t> *has_out)
{
    tsf_ctx *ctx = r->ctx;
    std::vector<int32_t> &has = *has_out;
    try {
        has = f->has;
        has.resize((size_t)n, 0);
    } catch (const std::bad_alloc &) {
        return fail(ctx, (std::string(entry) + ": out of host memory").c_str());
    }
    for (int64_t i = 0; i < c.N; ++i) {
        if (has[(size_t)c.group[i]]) {
            char msg[160];
            snprintf(msg, sizeof(msg), "%s[%lld] = %lld: the %s has a total already (one total per %s)", noun,
                     (long long)i, (long long)c.group[i], noun, noun);
            return fail(ctx, msg);
        }
        has[(size_t)c.group[i]] = 1;
    }
    if (!f->T) {
        // a second accumulator: +0.0 everywhere, so that the add below leaves the draws themselves in it
        // (the three become the handle's together or not at all: a failure frees what the locals hold)
        OwnedDev<double> T, yT;
        OwnedDev<int32_t> d_has;
        const hipError_t e = [&]() -> hipError_t {
            HIP_OK(T.alloc((size_t)n * r->H * r->S, true));
            HIP_OK(yT.alloc((size_t)n * r->H, true));
            HIP_OK(d_has.alloc((size_t)n, true));
            return hipDeviceSynchronize();
        }();
        if (e != hipSuccess) return rollup_hip_fail(ctx, entry, e);
        f->T.swap(T); f->yT.swap(yT); f->d_has.swap(d_has);
    }
    return 0;
}

// Draw: the totals' draws into the claimed slots, then the flags of the claim made the level's.
static int fitted_totals_draw(tsf_rollup *r, FittedTotals *f, const RollupCall &c, std::vector<int32_t> &has)
{
    tsf_ctx *ctx = r->ctx;
    if (int rc = rollup_accumulate(r, c, f->T, f->yT)) return rc;
    // (a failure of this copy leaves the device's flags behind the draws in T: poisoned like a failed add)
    r->poisoned = true;
    HIP_TRY(ctx, hipMemcpy(f->d_has, has.data(), 4 * has.size(), hipMemcpyHostToDevice));
    r->poisoned = false;
    f->has.swap(has);
    return 0;
}

extern "C" int tsf_rollup_set_totals(tsf_rollup *r, const tsf_spec *spec, int64_t Gt, const double *theta,
                                     const double *y_scale, const tsf_grid_info *grid, int32_t n_grids,
                                     const double *floor_, const double *cap, const double *extra_future,
                                     int32_t shared_extra, const int64_t *series_key, const int64_t *group)
{
    NoiseArOnce ar_once(r ? r->ctx : nullptr);
    if (int rc = rollup_enter(r, true)) return rc;
    tsf_ctx *ctx = r->ctx;
    if (int rc = refuse_noise_ar(ctx, "tsf_rollup_set_totals")) return rc;
    if (Gt < 0) return fail(ctx, "N must be >= 0");
    if (Gt == 0) return 0;
    const RollupCall c = {spec, Gt, theta, y_scale, grid, n_grids, floor_, cap, extra_future, shared_extra, series_key, group};
    if (int rc = rollup_check_series(r, c)) return rc;
    std::vector<int32_t> has;
    if (int rc = fitted_totals_claim(r, "tsf_rollup_set_totals", "group", &r->top, r->G, c, &has)) return rc;
    if (int rc = fitted_totals_draw(r, &r->top, c, has)) return rc;
    if (r->tree) r->tree->solved = false;
    return 0;
}

// share [n]: finite and in [0, 1]
static int check_shares(tsf_ctx *ctx, const char *name, const double *share, int64_t n)
{
    for (int64_t i = 0; i < n; ++i)
        if (!(share[i] >= 0.0 && share[i] <= 1.0)) {            // (NaN fails both comparisons)
            char msg[120];
            snprintf(msg, sizeof(msg), "%s[%lld] = %g: a share must be finite and in [0, 1]", name, (long long)i, share[i]);
            return fail(ctx, msg);
        }
    return 0;
}

// The second pass over the members behind tsf_rollup_reconcile and tsf_rollup_reconcile_tree, once the entry has
// checked its handle: the call's checks, the members drawn again chunk by chunk, `pass` launched on each chunk's sample
// buffer and point forecast in place (its arguments: samp, yhat, group and share of the chunk, the chunk's series count),
// then the running sums, the sorts and the copies out.
using MemberPass = std::function<void(double *samp, double *yhat, const int32_t *group, const double *share, int64_t nc)>;

static int reconcile_members(tsf_rollup *r, const char *entry, const RollupCall &c, const double *share, int32_t n_q,
                             const double *quantiles, tsf_reconcile_out *out, const MemberPass &pass)
{
    tsf_ctx *ctx = r->ctx;
    const tsf_spec *spec = c.spec;
    const int64_t N = c.N, *group = c.group;
    if (int rc = rollup_check_series(r, c)) return rc;
    if (!share) return fail(ctx, "NULL share");
    if (int rc = check_shares(ctx, "share", share, N)) return rc;
    if (!out) return fail(ctx, "NULL output (tsf_reconcile_out and its yhat are required)");
    if (int rc = check_rollup_read(r, n_q, quantiles, out->yhat, out->q, out->cum_q, out->samples)) return rc;
    const int32_t H = r->H, S = r->S;
    std::vector<int32_t> g32;
    try {
        g32.resize((size_t)N);
    } catch (const std::bad_alloc &) {
        return fail(ctx, (std::string(entry) + ": out of host memory").c_str());
    }
    for (int64_t n = 0; n < N; ++n) g32[(size_t)n] = (int32_t)group[n];
    RollupSeries in;
    if (int rc = in.upload(r, c)) return rc;
    // the shares and the groups of the whole call, sent once ahead of the first launch
    const size_t nh = 8 * (size_t)N * H, nqh = nh * (size_t)n_q;
    HostOuts outs;
    DevBuf d_share, d_group;
    double *d_yh = outs.want(out->yhat, nh), *d_q = outs.want(out->q, nqh), *d_cq = outs.want(out->cum_q, nqh);
    if (int rc = outs.ready(ctx)) return rc;
    HIP_TRY(ctx, d_share.put(share, 8 * (size_t)N));
    HIP_TRY(ctx, d_group.put(g32.data(), 4 * (size_t)N));
    const QuantilePass qp(H, S, n_q, quantiles);
    auto after = [&](int64_t n0, int64_t nc, const DrawBufs &b) -> int {
        pass(b.samp, d_yh + (size_t)n0 * H, d_group.as<int32_t>() + n0, d_share.as<double>() + n0, nc);
        HIP_TRY(ctx, hipGetLastError());
        if (out->cum_q) {
            // the running sums of the reconciled draws over the ones interval_sample_kernel left in the second buffer
            hipLaunchKernelGGL(rollup_cumsum_kernel, dim3((unsigned)((nc * S + 255) / 256)), dim3(256), 0, nullptr,
                               b.samp, b.cum, nc, H, S);
            HIP_TRY(ctx, hipGetLastError());
        }
        const struct { const double *src; double *dst; } sorts[2] = {{b.samp, d_q}, {b.cum, d_cq}};
        for (const auto &so : sorts)
            if (so.dst)
                if (int rc = qp.launch(ctx, so.src, so.dst, n0, nc, nullptr)) return rc;
        // the reconciled draws leave the scratch before the next chunk overwrites it (stream order)
        if (out->samples)
            HIP_TRY(ctx, hipMemcpyAsync(out->samples + (size_t)n0 * H * S, b.samp, 8 * (size_t)nc * H * S,
                                        hipMemcpyDeviceToHost, nullptr));
        return 0;
    };
    const DrawSpec d = {S, r->seed, out->cum_q != nullptr, false, d_yh, nullptr, false};
    if (int rc = draw_chunks(ctx, spec, in.up.dev, d, nullptr, after)) return rc;
    HIP_TRY(ctx, hipDeviceSynchronize());
    return outs.fetch(ctx);
}

extern "C" int tsf_rollup_reconcile(tsf_rollup *r, const tsf_spec *spec, int64_t N, const double *theta,
                                    const double *y_scale, const tsf_grid_info *grid, int32_t n_grids,
                                    const double *floor_, const double *cap, const double *extra_future,
                                    int32_t shared_extra, const int64_t *series_key, const int64_t *group,
                                    const double *share, int32_t n_q, const double *quantiles, tsf_reconcile_out *out)
{
    NoiseArOnce ar_once(r ? r->ctx : nullptr);
    if (int rc = rollup_enter(r, true)) return rc;
    tsf_ctx *ctx = r->ctx;
    if (int rc = refuse_noise_ar(ctx, "tsf_rollup_reconcile")) return rc;
    if (N < 0) return fail(ctx, "N must be >= 0");
    if (N == 0) return 0;
    if (!r->top.T) return fail(ctx, "tsf_rollup_reconcile before any tsf_rollup_set_totals: the roll-up has no total");
    const int32_t H = r->H, S = r->S;
    ReconcileMemberArgs m;
    memset(&m, 0, sizeof(m));
    m.acc = r->acc; m.top = r->top.T; m.ysum = r->ysum; m.ytop = r->top.yT; m.has_top = r->top.d_has; m.H = H; m.NS = S;
    const MemberPass pass = [&](double *samp, double *yhat, const int32_t *g, const double *sh, int64_t nc) {
        m.samp = samp; m.yhat = yhat; m.group = g; m.share = sh;
        hipLaunchKernelGGL(reconcile_member_kernel, dim3((unsigned)(nc * H), (unsigned)((S + 255) / 256)), dim3(256), 0,
                           nullptr, m);
    };
    const RollupCall c = {spec, N, theta, y_scale, grid, n_grids, floor_, cap, extra_future, shared_extra, series_key, group};
    return reconcile_members(r, "tsf_rollup_reconcile", c, share, n_q, quantiles, out, pass);
}

extern "C" int tsf_rollup_reconciled_totals(tsf_rollup *r, const double *share_total, int32_t n_q,
                                            const double *quantiles, tsf_rollup_out *out)
{
    if (int rc = rollup_enter(r, true)) return rc;
    tsf_ctx *ctx = r->ctx;
    if (!r->top.T)
        return fail(ctx, "tsf_rollup_reconciled_totals before any tsf_rollup_set_totals: the roll-up has no total");
    if (!share_total) return fail(ctx, "NULL share_total");
    if (int rc = check_shares(ctx, "share_total", share_total, r->G)) return rc;
    if (!out) return fail(ctx, "NULL output (tsf_rollup_out and its yhat are required)");
    if (int rc = check_rollup_read(r, n_q, quantiles, out->yhat, out->q, out->cum_q, out->samples)) return rc;
    DevBuf d_share;
    HostOuts outs;
    HIP_TRY(ctx, d_share.put(share_total, 8 * (size_t)r->G));
    // rollup_read's ranges of groups, each reconciled into the scratch first
    ReconcileTotalArgs t;
    memset(&t, 0, sizeof(t));
    t.acc = r->acc; t.top = r->top.T; t.ysum = r->ysum; t.ytop = r->top.yT; t.has_top = r->top.d_has;
    t.share = d_share.as<double>(); t.yout = outs.want(out->yhat, 8 * (size_t)r->G * r->H); t.H = r->H; t.NS = r->S;
    return rollup_read(r, n_q, quantiles, *out, &t, outs);
}

// ---- tree reconciliation: levels above the groups ------------------------------------------------------------

static const char *const TREE_NOT_SET = "before tsf_rollup_set_tree: the roll-up has no tree";

extern "C" int tsf_rollup_set_tree(tsf_rollup *r, int32_t n_upper, const int64_t *n_nodes, const int64_t *parent)
{
    if (int rc = rollup_enter(r, true)) return rc;
    tsf_ctx *ctx = r->ctx;
    if (r->tree) return fail(ctx, "tsf_rollup_set_tree: the roll-up has a tree already (one tree per roll-up)");
    if (n_upper < 1 || n_upper > TSF_TREE_MAX_LEVELS) return fail(ctx, "n_upper must be in [1, TSF_TREE_MAX_LEVELS]");
    if (!n_nodes || !parent) return fail(ctx, "NULL n_nodes or parent");
    const int32_t H = r->H, S = r->S;
    const int64_t cell_max = 2147483647 / H;                    // a launch has nodes * H blocks
    if (r->G > cell_max) return fail(ctx, "tsf_rollup_set_tree: G * H must be < 2^31");
    {
        int64_t below = r->G, n_par = 0;
        for (int32_t k = 0; k < n_upper; ++k) {
            if (n_nodes[k] < 1 || n_nodes[k] > cell_max) {
                char msg[120];
                snprintf(msg, sizeof(msg), "n_nodes[%d] = %lld: must be >= 1 and n_nodes * H < 2^31", k, (long long)n_nodes[k]);
                return fail(ctx, msg);
            }
            for (int64_t c = 0; c < below; ++c)
                if (parent[n_par + c] < 0 || parent[n_par + c] >= n_nodes[k]) {
                    char msg[160];
                    snprintf(msg, sizeof(msg), "parent[%lld] = %lld (node %lld of level %d): outside [0, %lld)",
                             (long long)(n_par + c), (long long)parent[n_par + c], (long long)c, k + 1, (long long)n_nodes[k]);
                    return fail(ctx, msg);
                }
            n_par += below; below = n_nodes[k];
        }
    }
    std::unique_ptr<RollupTree> t;
    std::vector<std::vector<int32_t>> first, child, par32;
    try {
        t.reset(new RollupTree());
        int64_t below = r->G, n_par = 0;
        t->M = r->G;
        for (int32_t k = 0; k < n_upper; ++k) {
            t->up.emplace_back();
            TreeLevel &lv = t->up.back();
            lv.n = n_nodes[k];
            lv.parent.assign(parent + n_par, parent + n_par + below);
            // the children of each node in ascending child index: a counting sort
            first.emplace_back((size_t)lv.n + 1, 0);
            child.emplace_back((size_t)below);
            par32.emplace_back((size_t)below);
            std::vector<int32_t> &f = first.back();
            for (int64_t c = 0; c < below; ++c) f[(size_t)lv.parent[(size_t)c] + 1] += 1;
            for (int64_t p = 0; p < lv.n; ++p) f[(size_t)p + 1] += f[(size_t)p];
            std::vector<int32_t> at(f.begin(), f.end() - 1);
            for (int64_t c = 0; c < below; ++c) {
                child.back()[(size_t)at[(size_t)lv.parent[(size_t)c]]++] = (int32_t)c;
                par32.back()[(size_t)c] = (int32_t)lv.parent[(size_t)c];
            }
            n_par += below; below = lv.n; t->M += lv.n;
        }
    } catch (const std::bad_alloc &) {
        return fail(ctx, "tsf_rollup_set_tree: out of host memory");
    }
    const hipError_t err = [&]() -> hipError_t {
        const size_t hs = (size_t)H * S;
        HIP_OK(t->delta.alloc((size_t)r->G * hs));
        HIP_OK(t->ydelta.alloc((size_t)r->G * H));
        HIP_OK(t->d_mk.alloc(2 * (size_t)t->M));
        for (size_t k = 0; k < t->up.size(); ++k) {
            TreeLevel &lv = t->up[k];
            const size_t n = (size_t)lv.n, nb = child[k].size();
            HIP_OK(lv.A.alloc(n * hs)); HIP_OK(lv.C.alloc(n * hs));
            HIP_OK(lv.yA.alloc(n * H)); HIP_OK(lv.yC.alloc(n * H));
            HIP_OK(lv.d_first.alloc(n + 1)); HIP_OK(lv.d_child.alloc(nb)); HIP_OK(lv.d_parent.alloc(nb));
            HIP_OK(hipMemcpy(lv.d_first, first[k].data(), 4 * (n + 1), hipMemcpyHostToDevice));
            HIP_OK(hipMemcpy(lv.d_child, child[k].data(), 4 * nb, hipMemcpyHostToDevice));
            HIP_OK(hipMemcpy(lv.d_parent, par32[k].data(), 4 * nb, hipMemcpyHostToDevice));
        }
        return hipDeviceSynchronize();
    }();
    if (err != hipSuccess) return rollup_hip_fail(ctx, "tsf_rollup_set_tree", err);
    r->tree.swap(t);
    return 0;
}

// level (1 = the groups) -> the level above the groups it names, or a refusal
static int tree_level(tsf_rollup *r, const char *entry, int32_t level, int32_t lowest, TreeLevel **lv)
{
    tsf_ctx *ctx = r->ctx;
    if (!r->tree) return fail(ctx, (std::string(entry) + " " + TREE_NOT_SET).c_str());
    const int32_t L = 1 + (int32_t)r->tree->up.size();
    if (level < lowest || level > L) {
        char msg[200];
        snprintf(msg, sizeof(msg), "%s: level = %d: outside [%d, %d]%s", entry, level, lowest, L,
                 level == 1 ? " (tsf_rollup_set_totals is the entry for level 1)" : "");
        return fail(ctx, msg);
    }
    *lv = level >= 2 ? &r->tree->up[(size_t)level - 2] : nullptr;
    return 0;
}

extern "C" int tsf_rollup_set_node_totals(tsf_rollup *r, int32_t level, const tsf_spec *spec, int64_t Gt,
                                          const double *theta, const double *y_scale, const tsf_grid_info *grid,
                                          int32_t n_grids, const double *floor_, const double *cap,
                                          const double *extra_future, int32_t shared_extra, const int64_t *series_key,
                                          const int64_t *node)
{
    NoiseArOnce ar_once(r ? r->ctx : nullptr);
    if (int rc = rollup_enter(r, true)) return rc;
    tsf_ctx *ctx = r->ctx;
    if (int rc = refuse_noise_ar(ctx, "tsf_rollup_set_node_totals")) return rc;
    TreeLevel *lv = nullptr;
    if (int rc = tree_level(r, "tsf_rollup_set_node_totals", level, 2, &lv)) return rc;
    if (Gt < 0) return fail(ctx, "N must be >= 0");
    if (Gt == 0) return 0;
    const RollupCall c = {spec, Gt, theta, y_scale, grid, n_grids, floor_, cap, extra_future, shared_extra, series_key, node};
    if (int rc = rollup_check_series(r, c, lv->n)) return rc;
    std::vector<int32_t> has;
    if (int rc = fitted_totals_claim(r, "tsf_rollup_set_node_totals", "node", &lv->fit, lv->n, c, &has)) return rc;
    r->tree->solved = false;
    return fitted_totals_draw(r, &lv->fit, c, has);
}

extern "C" int tsf_rollup_solve_tree(tsf_rollup *r, const double *mu, const double *kappa)
{
    if (int rc = rollup_enter(r, true)) return rc;
    tsf_ctx *ctx = r->ctx;
    if (!r->tree) return fail(ctx, (std::string("tsf_rollup_solve_tree ") + TREE_NOT_SET).c_str());
    RollupTree &t = *r->tree;
    if (!mu || !kappa) return fail(ctx, "NULL mu or kappa");
    if (int rc = check_shares(ctx, "mu", mu, t.M)) return rc;
    if (int rc = check_shares(ctx, "kappa", kappa, t.M)) return rc;
    t.solved = false;
    HIP_TRY(ctx, hipMemcpy(t.d_mk, mu, 8 * (size_t)t.M, hipMemcpyHostToDevice));
    HIP_TRY(ctx, hipMemcpy(t.d_mk + t.M, kappa, 8 * (size_t)t.M, hipMemcpyHostToDevice));
    const int32_t H = r->H, S = r->S;
    const unsigned by = (unsigned)((S + 255) / 256);
    const double *d_mu = t.d_mk, *d_kappa = t.d_mk + t.M;
    // up: the groups' blend, then per level the gather of the level below and the blend with the level's own totals
    TreeBlendArgs b;
    memset(&b, 0, sizeof(b));
    b.H = H; b.NS = S;
    b.A = r->acc; b.t = r->top.T; b.m = t.delta; b.yA = r->ysum; b.yt = r->top.yT; b.ym = t.ydelta;
    b.has = r->top.T ? r->top.d_has.p : nullptr; b.mu = d_mu;
    hipLaunchKernelGGL(tree_blend_kernel, dim3((unsigned)(r->G * H), by), dim3(256), 0, nullptr, b);
    HIP_TRY(ctx, hipGetLastError());
    const double *m = t.delta, *ym = t.ydelta;
    int64_t off = r->G;
    for (TreeLevel &lv : t.up) {
        const TreeGatherArgs g = {m, lv.A, ym, lv.yA, lv.d_first, lv.d_child, H, S};
        hipLaunchKernelGGL(tree_gather_kernel, dim3((unsigned)(lv.n * H), by), dim3(256), 0, nullptr, g);
        HIP_TRY(ctx, hipGetLastError());
        b.A = lv.A; b.t = lv.fit.T; b.m = lv.C; b.yA = lv.yA; b.yt = lv.fit.yT; b.ym = lv.yC;
        b.has = lv.fit.T ? lv.fit.d_has.p : nullptr; b.mu = d_mu + off;
        hipLaunchKernelGGL(tree_blend_kernel, dim3((unsigned)(lv.n * H), by), dim3(256), 0, nullptr, b);
        HIP_TRY(ctx, hipGetLastError());
        m = lv.C; ym = lv.yC; off += lv.n;
    }
    // down: the top level's c is its m; every level below takes its share of what its parent moved by
    for (size_t k = t.up.size(); k-- > 0;) {
        TreeLevel &lv = t.up[k];
        off -= lv.n;                                            // (now the first node of level k + 2)
        const bool groups = k == 0;
        const int64_t n = groups ? r->G : t.up[k - 1].n;
        TreePushArgs p;
        memset(&p, 0, sizeof(p));
        p.H = H; p.NS = S;
        p.m = groups ? t.delta.p : t.up[k - 1].C.p; p.ym = groups ? t.ydelta.p : t.up[k - 1].yC.p;
        p.cp = lv.C; p.Ap = lv.A; p.ycp = lv.yC; p.yAp = lv.yA;
        p.acc = groups ? r->acc.p : nullptr; p.yacc = groups ? r->ysum.p : nullptr;
        p.parent = lv.d_parent; p.kappa = d_kappa + (off - n);
        hipLaunchKernelGGL(tree_push_kernel, dim3((unsigned)(n * H), by), dim3(256), 0, nullptr, p);
        HIP_TRY(ctx, hipGetLastError());
    }
    HIP_TRY(ctx, hipDeviceSynchronize());
    t.solved = true;
    return 0;
}

static const char *const TREE_NOT_SOLVED =
    "the tree is not solved: tsf_rollup_solve_tree has not run since the last add, set_totals or set_node_totals";

extern "C" int tsf_rollup_reconcile_tree(tsf_rollup *r, const tsf_spec *spec, int64_t N, const double *theta,
                                         const double *y_scale, const tsf_grid_info *grid, int32_t n_grids,
                                         const double *floor_, const double *cap, const double *extra_future,
                                         int32_t shared_extra, const int64_t *series_key, const int64_t *group,
                                         const double *share, int32_t n_q, const double *quantiles, tsf_reconcile_out *out)
{
    NoiseArOnce ar_once(r ? r->ctx : nullptr);
    if (int rc = rollup_enter(r, true)) return rc;
    tsf_ctx *ctx = r->ctx;
    if (int rc = refuse_noise_ar(ctx, "tsf_rollup_reconcile_tree")) return rc;
    if (N < 0) return fail(ctx, "N must be >= 0");
    if (N == 0) return 0;
    if (!r->tree) return fail(ctx, (std::string("tsf_rollup_reconcile_tree ") + TREE_NOT_SET).c_str());
    if (!r->tree->solved) return fail(ctx, (std::string("tsf_rollup_reconcile_tree: ") + TREE_NOT_SOLVED).c_str());
    const int32_t H = r->H, S = r->S;
    TreeMemberArgs m;
    memset(&m, 0, sizeof(m));
    m.delta = r->tree->delta; m.ydelta = r->tree->ydelta; m.H = H; m.NS = S;
    const MemberPass pass = [&](double *samp, double *yhat, const int32_t *g, const double *sh, int64_t nc) {
        m.samp = samp; m.yhat = yhat; m.group = g; m.share = sh;
        hipLaunchKernelGGL(tree_member_kernel, dim3((unsigned)(nc * H), (unsigned)((S + 255) / 256)), dim3(256), 0, nullptr, m);
    };
    const RollupCall c = {spec, N, theta, y_scale, grid, n_grids, floor_, cap, extra_future, shared_extra, series_key, group};
    return reconcile_members(r, "tsf_rollup_reconcile_tree", c, share, n_q, quantiles, out, pass);
}

extern "C" int tsf_rollup_tree_totals(tsf_rollup *r, int32_t level, int64_t node0, int64_t n_nodes, int32_t n_q,
                                      const double *quantiles, tsf_rollup_out *out)
{
    if (int rc = rollup_enter(r, true)) return rc;
    tsf_ctx *ctx = r->ctx;
    TreeLevel *lv = nullptr;
    if (int rc = tree_level(r, "tsf_rollup_tree_totals", level, 1, &lv)) return rc;
    RollupTree &t = *r->tree;
    if (!t.solved) return fail(ctx, (std::string("tsf_rollup_tree_totals: ") + TREE_NOT_SOLVED).c_str());
    const int64_t n_level = lv ? lv->n : r->G;
    if (node0 < 0 || n_nodes < 0 || node0 > n_level || n_nodes > n_level - node0) {
        char msg[160];
        snprintf(msg, sizeof(msg), "nodes [%lld, %lld + %lld): outside the level's [0, %lld)", (long long)node0,
                 (long long)node0, (long long)n_nodes, (long long)n_level);
        return fail(ctx, msg);
    }
    if (!out) return fail(ctx, "NULL output (tsf_rollup_out and its yhat are required)");
    if (int rc = check_rollup_read(r, n_q, quantiles, out->yhat, out->q, out->cum_q, out->samples)) return rc;
    if (n_nodes == 0) return 0;
    const int32_t H = r->H, S = r->S;
    const size_t hs = (size_t)H * S;
    if (out->count) {
        // the members added below each node: the groups' counts summed up the levels
        try {
            std::vector<int64_t> cnt(r->count), up;
            for (int32_t k = 2; k <= level; ++k) {
                const TreeLevel &l = t.up[(size_t)k - 2];
                up.assign((size_t)l.n, 0);
                for (size_t c = 0; c < cnt.size(); ++c) up[(size_t)l.parent[c]] += cnt[c];
                cnt.swap(up);
            }
            memcpy(out->count, cnt.data() + node0, 8 * (size_t)n_nodes);
        } catch (const std::bad_alloc &) {
            return fail(ctx, "tsf_rollup_tree_totals: out of host memory");
        }
    }
    HostOuts outs;
    if (lv) {
        // a level above the groups: c itself is kept
        outs.adopt(out->yhat, lv->yC + (size_t)node0 * H, 8 * (size_t)n_nodes * H);
        return cells_read(r, lv->C + (size_t)node0 * hs, n_nodes, n_q, quantiles, *out, nullptr, outs);
    }
    // the groups: acc + (c - acc), range by range into the scratch
    TreeTotalArgs a;
    memset(&a, 0, sizeof(a));
    a.acc = r->acc; a.delta = t.delta; a.ysum = r->ysum; a.ydelta = t.ydelta; a.H = H; a.NS = S;
    double *d_yh = outs.want(out->yhat, 8 * (size_t)n_nodes * H);
    const CellMaker make = [&](double *dst, int64_t g0, int64_t gc) -> int {
        a.out = dst; a.yout = d_yh + (size_t)g0 * H; a.g0 = node0 + g0;
        hipLaunchKernelGGL(tree_total_kernel, dim3((unsigned)(gc * H), (unsigned)((S + 255) / 256)), dim3(256), 0, nullptr, a);
        HIP_TRY(ctx, hipGetLastError());
        return 0;
    };
    return cells_read(r, nullptr, n_nodes, n_q, quantiles, *out, &make, outs);
}

// ---- temporal reconciliation: daily forecasts and fitted period totals made coherent ------------------------

extern "C" int tsf_temporal_out_size(void) { return (int)sizeof(tsf_temporal_out); }

// phi [N] in [0, 1) -> the (phi, sqrt(1 - phi^2)) pairs interval_sample_kernel<true> reads (tsf_set_noise_ar's)
static int noise_ar_pairs(tsf_ctx *ctx, const char *name, const double *phi, int64_t N, std::vector<double> *pairs)
{
    pairs->clear();
    if (!phi) return 0;
    for (int64_t i = 0; i < N; ++i)
        if (!(phi[i] >= 0.0 && phi[i] < 1.0)) {                     // (NaN fails both comparisons)
            char msg[120];
            snprintf(msg, sizeof(msg), "%s[%lld] = %g: an autocorrelation must be in [0, 1)", name, (long long)i, phi[i]);
            return fail(ctx, msg);
        }
    pairs->resize(2 * (size_t)N);
    for (int64_t i = 0; i < N; ++i) {
        (*pairs)[2 * (size_t)i] = phi[i];
        (*pairs)[2 * (size_t)i + 1] = std::sqrt(1.0 - phi[i] * phi[i]);
    }
    return 0;
}

// series per chunk of tsf_predict_temporal: the daily model's n_buf sample buffers [H][n_samples], the period model's
// one [K][n_samples] and the three per-row pieces of both within 512 MB
static int64_t temporal_chunk_series(int64_t N, int32_t H, int32_t K, int32_t n_samples, size_t n_buf)
{
    const size_t per_series = 8 * ((size_t)H * (3 + n_buf * (size_t)n_samples) + (size_t)K * (3 + (size_t)n_samples));
    int64_t chunk = (int64_t)(((size_t)512 << 20) / per_series);
    if (chunk < 1) chunk = 1;
    if (chunk > N) chunk = N;
    return chunk;
}

// What tsf_predict_temporal refuses of its own arguments (the forecasts' inputs are checked by the entry), before
// anything is copied or launched.
static int check_temporal_args(tsf_ctx *ctx, int64_t N, int32_t H, int32_t K, int32_t n_samples, const int32_t *win_start,
                               const int32_t *win_end, const double *share, const double *share_total, int32_t n_q,
                               const double *quantiles, const tsf_temporal_out *out)
{
    if (!out || !out->yhat) return fail(ctx, "NULL output (tsf_temporal_out and its yhat are required)");
    if (int rc = check_samples_and_levels(ctx, n_samples, n_q, quantiles)) return rc;
    const WindowCall wc = {K, win_start, win_end, nullptr};
    if (int rc = check_windows(ctx, H, wc)) return rc;
    if (int rc = check_disjoint_windows(ctx, H, wc)) return rc;
    if (!share || !share_total) return fail(ctx, "NULL share or share_total");
    if (int rc = check_shares(ctx, "share", share, N * H)) return rc;
    const size_t nk = (size_t)N * K;
    for (size_t i = 0; i < nk; ++i)
        if (!std::isnan(share_total[i]) && !(share_total[i] >= 0.0 && share_total[i] <= 1.0)) {
            char msg[160];
            snprintf(msg, sizeof(msg), "share_total[%lld][%d] = %g: a share must be in [0, 1] (NaN: the window is not reconciled)",
                     (long long)(i / K), (int)(i % K), share_total[i]);
            return fail(ctx, msg);
        }
    const bool want_q = out->q || out->cum_q || out->win_q;
    if (!want_q && !out->samples && !out->win_samples)
        return fail(ctx, "nothing requested but yhat and total: q, cum_q, win_q, samples and win_samples are all NULL");
    if (n_q == 0 && want_q) return fail(ctx, "n_q = 0 with a quantile output requested");
    return 0;
}

extern "C" int tsf_predict_temporal(tsf_ctx *ctx,
                                    const tsf_spec *spec, int64_t N, int32_t H, const double *theta, const double *y_scale,
                                    const tsf_grid_info *grid, int32_t n_grids, const int64_t *ds_future,
                                    int32_t shared_future, const double *floor_, const double *cap,
                                    const double *extra_future, const int64_t *series_key, const double *noise_ar,
                                    const tsf_spec *spec_p, int32_t K, const double *theta_p, const double *y_scale_p,
                                    const tsf_grid_info *grid_p, int32_t n_grids_p, const int64_t *ds_period,
                                    int32_t shared_period, const double *floor_p, const double *cap_p,
                                    const double *extra_period, const int64_t *period_key, const double *noise_ar_p,
                                    int32_t n_samples, uint64_t seed, const int32_t *win_start, const int32_t *win_end,
                                    const double *share, const double *share_total, int32_t n_q, const double *quantiles,
                                    tsf_temporal_out *out)
{
    if (!ctx) return -1;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (N < 0) return fail(ctx, "N must be >= 0");
    if (N == 0) return 0;
    if (K < 1 || K > TSF_MAX_WINDOWS) return fail(ctx, "K must be in [1, TSF_MAX_WINDOWS]");
    const ForecastIn h = {N, H, theta, y_scale, grid, n_grids, ds_future, shared_future, floor_, cap, extra_future, series_key};
    const ForecastIn hp = {N, K, theta_p, y_scale_p, grid_p, n_grids_p, ds_period, shared_period, floor_p, cap_p, extra_period,
                           period_key};
    if (int rc = check_forecast_in(ctx, h, spec != nullptr)) return rc;
    if (int rc = check_forecast_in(ctx, hp, spec_p != nullptr)) return rc;
    if (!series_key || !period_key)
        return fail(ctx, "series_key and period_key are required: the index-in-call default would give both models the same streams");
    if (int rc = check_grids(ctx, spec, grid, n_grids)) return rc;
    if (int rc = check_grids(ctx, spec_p, grid_p, n_grids_p)) return rc;
    ModelDraw day, per;
    std::vector<double> ar, ar_p;
    try {
        if (int rc = check_temporal_args(ctx, N, H, K, n_samples, win_start, win_end, share, share_total, n_q, quantiles, out))
            return rc;
        if (int rc = noise_ar_pairs(ctx, "noise_ar", noise_ar, N, &ar)) return rc;
        if (int rc = noise_ar_pairs(ctx, "noise_ar_p", noise_ar_p, N, &ar_p)) return rc;
    } catch (const std::bad_alloc &) {
        return fail(ctx, "tsf_predict_temporal: out of host memory");
    }
    if (int rc = forecast_spec(ctx, spec, h, &day.hs)) return rc;
    if (int rc = forecast_spec(ctx, spec_p, hp, &per.hs)) return rc;

    // both models' inputs, the shares, the windows and the AR pairs onto the device; the [N][.]-sized outputs there
    ForecastUpload up, up_p;
    if (int rc = up.upload(ctx, spec, h)) return rc;
    if (int rc = up_p.upload(ctx, spec_p, hp)) return rc;
    const size_t nh = (size_t)N * H, nk = (size_t)N * K;
    DevBuf d_share, d_mu, d_win, d_ar, d_ar_p, d_yp;
    HIP_TRY(ctx, d_share.put(share, 8 * nh));
    HIP_TRY(ctx, d_mu.put(share_total, 8 * nk));
    HIP_TRY(ctx, d_win.alloc(8 * (size_t)K));
    int32_t *d_w0 = d_win.as<int32_t>(), *d_w1 = d_w0 + K;
    HIP_TRY(ctx, hipMemcpy(d_w0, win_start, 4 * (size_t)K, hipMemcpyHostToDevice));
    HIP_TRY(ctx, hipMemcpy(d_w1, win_end, 4 * (size_t)K, hipMemcpyHostToDevice));
    if (!ar.empty()) HIP_TRY(ctx, d_ar.put(ar.data(), 8 * ar.size()));
    if (!ar_p.empty()) HIP_TRY(ctx, d_ar_p.put(ar_p.data(), 8 * ar_p.size()));
    HIP_TRY(ctx, d_yp.alloc(8 * nk));
    HostOuts outs;
    double *d_yh = outs.want(out->yhat, 8 * nh);
    double *d_q = outs.want(out->q, 8 * nh * (size_t)n_q), *d_cq = outs.want(out->cum_q, 8 * nh * (size_t)n_q);
    double *d_tot = outs.want(out->total, 8 * nk), *d_wq = outs.want(out->win_q, 8 * nk * (size_t)n_q);
    if (int rc = outs.ready(ctx)) return rc;

    // the chunk's scratch: the per-row pieces of both models, the daily buffer, the running sums with cum_q, the period buffer
    const size_t NS = (size_t)n_samples, n_buf = out->cum_q ? 2 : 1;
    const int64_t chunk = temporal_chunk_series(N, H, K, n_samples, n_buf);
    const size_t ch = (size_t)chunk * H, ck = (size_t)chunk * K;
    if (int rc = ensure_iv_ws(ctx, 8 * (ch * (3 + n_buf * NS) + ck * (3 + NS)))) return rc;
    double *d_pieces = (double *)ctx->iv_ws, *d_pieces_p = d_pieces + 3 * ch;
    double *d_samp = d_pieces_p + 3 * ck, *d_cum = out->cum_q ? d_samp + ch * NS : nullptr;
    double *d_psamp = d_samp + n_buf * ch * NS;
    hipStream_t st = nullptr;
    const DrawSpec dd = {n_samples, seed, false, false, d_yh, nullptr, false};
    const DrawSpec dp = {n_samples, seed, false, false, d_yp.as<double>(), nullptr, false};
    day.bind(ctx, spec, up.dev, dd, ar.empty() ? nullptr : d_ar.as<double>(), d_pieces, ch, {d_samp, nullptr, nullptr});
    per.bind(ctx, spec_p, up_p.dev, dp, ar_p.empty() ? nullptr : d_ar_p.as<double>(), d_pieces_p, ck, {d_psamp, nullptr, nullptr});
    const QuantilePass qp(H, n_samples, n_q, quantiles), qpw(K, n_samples, n_q, quantiles);
    TemporalArgs t;
    memset(&t, 0, sizeof(t));
    t.samp = d_samp; t.win = d_psamp; t.w0 = d_w0; t.w1 = d_w1; t.H = H; t.K = K; t.NS = n_samples;
    for (int64_t n0 = 0; n0 < N; n0 += chunk) {
        const int64_t nc = std::min(chunk, N - n0);
        // (the context has one device spec and one future design table: each model's are sent ahead of its draw)
        if (int rc = day.send_spec(ctx, st)) return rc;
        if (int rc = day.chunk(ctx, n0, nc, st)) return rc;
        if (int rc = per.send_spec(ctx, st)) return rc;
        if (int rc = per.chunk(ctx, n0, nc, st)) return rc;
        t.share = d_share.as<double>() + (size_t)n0 * H; t.share_total = d_mu.as<double>() + (size_t)n0 * K;
        hipLaunchKernelGGL(temporal_reconcile_kernel, dim3((unsigned)(nc * K), (unsigned)((n_samples + 255) / 256)), dim3(256),
                           0, st, t);
        HIP_TRY(ctx, hipGetLastError());
        if (d_cum) {
            hipLaunchKernelGGL(rollup_cumsum_kernel, dim3((unsigned)((nc * n_samples + 255) / 256)), dim3(256), 0, st, d_samp,
                               d_cum, nc, H, n_samples);
            HIP_TRY(ctx, hipGetLastError());
        }
        if (d_q) if (int rc = qp.launch(ctx, d_samp, d_q, n0, nc, st)) return rc;
        if (d_cq) if (int rc = qp.launch(ctx, d_cum, d_cq, n0, nc, st)) return rc;
        if (d_wq) if (int rc = qpw.launch(ctx, d_psamp, d_wq, n0, nc, st)) return rc;
        // the reconciled draws leave the scratch before the next chunk overwrites it (stream order)
        if (out->samples)
            HIP_TRY(ctx, hipMemcpyAsync(out->samples + (size_t)n0 * H * NS, d_samp, 8 * (size_t)nc * H * NS,
                                        hipMemcpyDeviceToHost, st));
        if (out->win_samples)
            HIP_TRY(ctx, hipMemcpyAsync(out->win_samples + (size_t)n0 * K * NS, d_psamp, 8 * (size_t)nc * K * NS,
                                        hipMemcpyDeviceToHost, st));
    }
    // the point forecasts of the whole call: yhat rewritten in place, total where wanted
    hipLaunchKernelGGL(temporal_point_kernel, dim3((unsigned)((N * K + 255) / 256)), dim3(256), 0, st, d_yh,
                       d_yp.as<double>(), d_w0, d_w1, d_share.as<double>(), d_mu.as<double>(), d_tot, N, H, K);
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, hipDeviceSynchronize());
    return outs.fetch(ctx);
}

// ---- diagnostics --------------------------------------------------------------------------------

extern "C" int tsf_design(tsf_ctx *ctx, const tsf_spec *spec, int32_t T, const int64_t *ds,
                          const double *extra, double *X_out, double *t_out,
                          tsf_grid_info *grid_out)
{
    if (!ctx) return -1;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (!spec || !ds || T < 2) return fail(ctx, "bad input");
    DevSpec hs;
    int mode = 0;
    int rc = build_devspec(ctx, spec, &hs, &mode);
    if (rc) return rc;
    if (hs.n_extra > 0 && !extra) return fail(ctx, "extra is NULL");
    const int NT = (T + W - 1) / W;
    FitPlan one = {};               // one grid's tables, nothing else
    one.n_grids = 1; one.NTmax = NT;
    const WsLayout l = ws_layout(1, one, hs.KP);
    rc = ensure_ws(ctx, l.total);
    if (rc) return rc;
    char *ws = (char *)ctx->ws;
    DevBuf d_ds, d_ex;
    HIP_TRY(ctx, d_ds.alloc(8 * (size_t)T));
    HIP_TRY(ctx, hipMemcpy(d_ds.p, ds, 8 * (size_t)T, hipMemcpyHostToDevice));
    if (hs.n_extra > 0) {
        HIP_TRY(ctx, d_ex.alloc(8 * (size_t)hs.n_extra * T));
        HIP_TRY(ctx, hipMemcpy(d_ex.p, extra, 8 * (size_t)hs.n_extra * T, hipMemcpyHostToDevice));
    }
    HIP_TRY(ctx, hipMemcpy(ctx->d_spec, &hs, sizeof(hs), hipMemcpyHostToDevice));
    HIP_TRY(ctx, hipMemset(ws + l.Xw, 0, sizeof(double) * (size_t)NT * hs.KP * W));
    HIP_TRY(ctx, hipMemset(ws + l.gtab, 0, sizeof(GridTab)));
    hipLaunchKernelGGL(setup_grid_kernel, dim3(1), dim3(256), 0, nullptr, ctx->d_spec, 1, nullptr, T,
                       d_ds.as<int64_t>(), d_ex.as<double>(), (int64_t)T, NT, (GridTab *)(ws + l.gtab),
                       (double *)(ws + l.tw), (uint16_t *)(ws + l.cw), (double *)(ws + l.Xw), nullptr,
                       (int64_t)0, (int64_t)0);
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, hipDeviceSynchronize());
    std::vector<double> Xw((size_t)NT * hs.KP * W), tw((size_t)NT * W);
    GridTab gt;
    HIP_TRY(ctx, hipMemcpy(Xw.data(), ws + l.Xw, Xw.size() * 8, hipMemcpyDeviceToHost));
    HIP_TRY(ctx, hipMemcpy(tw.data(), ws + l.tw, tw.size() * 8, hipMemcpyDeviceToHost));
    HIP_TRY(ctx, hipMemcpy(&gt, ws + l.gtab, sizeof(gt), hipMemcpyDeviceToHost));
    for (int i = 0; i < T; ++i) {
        const int L = i / NT, q = i - L * NT;
        if (t_out) t_out[i] = tw[(size_t)q * W + L];
        if (X_out)
            for (int j = 0; j < hs.K; ++j)
                X_out[(size_t)i * hs.K + hs.perm[j]] = Xw[((size_t)q * hs.KP + j) * W + L];
    }
    if (grid_out) *grid_out = gt.info;
    return 0;
}

extern "C" int tsf_selftest_math(tsf_ctx *ctx, int32_t op, int64_t n, const double *a,
                                 const double *b, double *out)
{
    if (!ctx) return -1;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (n <= 0 || !a || !out) return fail(ctx, "bad input");
    DevBuf da, db, dout;
    HIP_TRY(ctx, da.alloc(8 * n)); HIP_TRY(ctx, dout.alloc(8 * n));
    HIP_TRY(ctx, hipMemcpy(da.p, a, 8 * n, hipMemcpyHostToDevice));
    if (b) { HIP_TRY(ctx, db.alloc(8 * n)); HIP_TRY(ctx, hipMemcpy(db.p, b, 8 * n, hipMemcpyHostToDevice)); }
    hipLaunchKernelGGL(selftest_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, nullptr, op, n,
                       da.as<double>(), b ? db.as<double>() : nullptr, dout.as<double>());
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, hipDeviceSynchronize());
    HIP_TRY(ctx, hipMemcpy(out, dout.p, 8 * n, hipMemcpyDeviceToHost));
    return 0;
}

// ---- measurement hooks --------------------------------------------------------------------------

extern "C" int tsf_set_cost_hints(tsf_ctx *ctx, const int32_t *cost, int64_t n)
{
    if (!ctx) return -1;
    ctx->order_n = 0;
    if (!cost || n <= 0) return 0;
    if (n > (int64_t)INT32_MAX) return fail(ctx, "tsf_set_cost_hints: too many series");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    std::vector<int32_t> order((size_t)n);
    for (int64_t i = 0; i < n; ++i) order[(size_t)i] = (int32_t)i;
    std::stable_sort(order.begin(), order.end(), [cost](int32_t x, int32_t y) { return cost[x] > cost[y]; });
    const int b = ctx->order_next;
    if (ctx->order_busy[b]) {   // a fit two calls back may still be reading this buffer on its stream
        HIP_TRY(ctx, hipEventSynchronize(ctx->order_ev[b]));
        ctx->order_busy[b] = 0;
    }
    const size_t need = sizeof(int32_t) * (size_t)n;
    if (ctx->order_cap[b] < need) {
        if (ctx->order_dev[b]) { HIP_TRY(ctx, hipFree(ctx->order_dev[b])); ctx->order_dev[b] = nullptr; ctx->order_cap[b] = 0; }
        HIP_TRY(ctx, hipMalloc((void **)&ctx->order_dev[b], need));
        ctx->order_cap[b] = need;
    }
    HIP_TRY(ctx, hipMemcpy(ctx->order_dev[b], order.data(), need, hipMemcpyHostToDevice));
    ctx->order_next = b ^ 1;
    ctx->order_n = n;
    if (cost != ctx->cost_host.data()) ctx->cost_host.assign(cost, cost + n);
    return 0;
}

extern "C" int tsf_set_profiling(tsf_ctx *ctx, int32_t enable)
{
    if (!ctx) return -1;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (enable && !ctx->ev_created) {
        for (int i = 0; i < TSF_PROFILE_RING; ++i) {
            HIP_TRY(ctx, hipEventCreate(&ctx->ev0[i]));
            HIP_TRY(ctx, hipEventCreate(&ctx->ev1[i]));
        }
        ctx->ev_created = 1;
    }
    ctx->profiling = enable ? 1 : 0;
    ctx->ev_count = 0;
    return 0;
}

extern "C" int tsf_profile_read(tsf_ctx *ctx, float *ms_out, int32_t max_n, int32_t *n_out)
{
    if (!ctx) return -1;
    if (!ms_out || !n_out) return fail(ctx, "NULL output");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    long n = ctx->ev_count < TSF_PROFILE_RING ? ctx->ev_count : TSF_PROFILE_RING;
    if (n > max_n) n = max_n;
    const long first = ctx->ev_count - n;
    for (long i = 0; i < n; ++i) {
        const int slot = (int)((first + i) % TSF_PROFILE_RING);
        HIP_TRY(ctx, hipEventSynchronize(ctx->ev1[slot]));
        HIP_TRY(ctx, hipEventElapsedTime(&ms_out[i], ctx->ev0[slot], ctx->ev1[slot]));
    }
    *n_out = (int32_t)n;
    return 0;
}

extern "C" int tsf_last_fit_route(tsf_ctx *ctx, int32_t *sparse_columns)
{
    if (!ctx || !sparse_columns) return -1;
    *sparse_columns = 0;
    if (!ctx->last_sp_flag) return 0;
    int bad = 1;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, hipDeviceSynchronize());
    HIP_TRY(ctx, hipMemcpy(&bad, ctx->last_sp_flag, sizeof(int), hipMemcpyDeviceToHost));
    *sparse_columns = bad ? 0 : 1;
    return 0;
}

extern "C" int tsf_last_fit_kernel_ms(tsf_ctx *ctx, float *ms_out)
{
    if (!ctx) return -1;
    if (!ms_out || ctx->ev_count == 0) return fail(ctx, "no profiled fit call recorded");
    int32_t n = 0;
    float tmp[TSF_PROFILE_RING];
    int rc = tsf_profile_read(ctx, tmp, TSF_PROFILE_RING, &n);
    if (rc) return rc;
    *ms_out = tmp[n - 1];
    return 0;
}

// ---- cross-validation (include/tsf.h) ---------------------------------------------------------------
// The caller's panel crosses to the device once; every fit launch gets its fold panel from cv_expand_kernel (history
// rows of its folds, cut on the device) and runs through run_fit like a ragged fit, its calendar classes handed in
// (aligned input: fold c of every series is one calendar, known from the construction; ragged input: the prefixes of
// the caller's series through calendar_classes, reading the caller's rows in place).  The fold results are scattered to
// plan order, the holdout rows predicted by the predict (and interval) kernels in one call over every fold, and
// cv_metrics_kernel reduces them per series.  tsf_tune runs the same pieces: the plan, the panel, the holdout rows and
// the fold panel of each optimiser group once, the fits, predict and metrics once per candidate.

extern "C" int tsf_last_cv_grids(const tsf_ctx *ctx, int64_t *n_grids, int32_t *n_launches)
{
    if (!ctx || !n_grids || !n_launches) return -1;
    *n_grids = ctx->cv_grids;
    *n_launches = ctx->cv_launches;
    return 0;
}

namespace {
// The caller's panel as the host entries of the panel jobs receive it (host pointers).
struct PanelIn {
    int64_t N; int32_t T; const int64_t *offsets, *ds; const void *y; int32_t y_dtype; const double *floor_, *cap, *extra;
};

struct CvHoldout {              // the holdout rows of every fold as one padded future panel [F][Hmax]
    DevBuf d_fds, d_fex, d_fkey, d_ffl, d_fcap;
};

struct CvMetrics {              // cv_metrics_kernel's tables, scratch and outputs
    DevBuf d_foff, d_roff, d_moff, d_fcut, d_frow0, d_hs, d_ts, d_pre, d_yo, d_loo, d_hio, d_mh, d_mm, d_sst;
    CvMetricArgs ma;
};

// What a cross-validation call derives once from its arguments: the plan, the fold tables, the caller's panel on the
// device (cv_upload), the fold fit outputs in plan order, the holdout rows, their forecasts [F][Hmax] and the metrics.
struct CvCall : PanelIn {
    bool aligned = false;
    size_t ysz = 8;
    int n_extra = 0, stride = 0;
    bool has_floor = false, has_cap = false;
    std::vector<std::vector<tsf_cv::Fold>> plan;
    std::vector<int32_t> pst;
    std::vector<int64_t> pnh, pnm, fold_off, rows_off, m_off;
    int64_t F = 0, R = 0, M = 0;
    std::vector<int32_t> f_series, f_c;
    std::vector<int64_t> f_cut, f_hist, f_hold, f_row0;
    std::vector<double> f_floor, f_cap;
    std::vector<int32_t> f_keep;        // specified changepoints: the leading dates <= the fold's cutoff (else empty)
    int32_t Hmax = 1, C = 0;
    DevBuf d_ds, d_y, d_off, d_ex, d_fl, d_cap, d_key, d_fser, d_fc, d_fhist, d_fhold;
    CvPanel pn;
    DevFitOut fit;
    CvHoldout hold;
    DevBuf d_yh, d_lo, d_hi;
    CvMetrics met;
};

// Views of the caller's series that cv_expand_kernel cuts: view v = rows [0, hist[v]) of series series[v].  The folds
// of a call (on an aligned panel every cutoff is one calendar: cls = the cutoff index), or whole series (tsf_tune's
// ragged refit).
struct CvViews {
    const int32_t *d_series;    // device [V]
    const int32_t *series;      // host [V]
    const int64_t *hist;        // host [V]
    const int32_t *cls;         // host [V]: calendar class known from the construction, or null (classes by hashing)
    int32_t n_cls;
    const int32_t *keep;        // host [V]: specified changepoints the view's fit keeps (CvCall::f_keep), or null (all)
};

// The panel of one fit launch: views gf[0 .. G), cut on the device, and their calendar classes.
struct CvGroup {
    std::vector<int32_t> gf;
    std::vector<int64_t> goff;          // [G + 1] row offsets of the members in the launch's panel
    int64_t G = 0, rows = 0, n_distinct = 0;
    int32_t maxT = 0;
    DevBuf d_gf, d_goff, d_gds, d_gy, d_gex, d_gfl, d_gcap, d_gof, d_grows, d_gord;
    DevBuf d_gkeep;             // [grids of the launch] CvViews::keep per grid (setup_grid_kernel grid_keep), where given
};

}  // namespace

// the caller's panel and its shape (what cv_upload and every launch over the panel read of a CvCall)
static void cv_call_shape(const PanelIn &p, const tsf_spec *spec, CvCall *S)
{
    static_cast<PanelIn &>(*S) = p;
    S->aligned = p.offsets == nullptr;
    S->ysz = ysize(p.y_dtype);
    S->n_extra = spec->n_extra; S->stride = tsf_theta_stride(spec);
    S->has_floor = p.floor_ != nullptr; S->has_cap = p.cap != nullptr;
}

// specified changepoints: per fold (cutoffs f_cut) the leading dates <= its cutoff -- what prophet_copy(m, cutoff) keeps,
// changepoints[changepoints <= cutoff], a prefix of the sorted list; empty for a spec without specified dates
static std::vector<int32_t> cv_fold_keep(const tsf_spec &spec, const std::vector<int64_t> &f_cut)
{
    std::vector<int32_t> keep;
    if (!(spec.changepoints_specified == 1 && spec.n_changepoints >= 0 && spec.n_changepoints <= TSF_MAX_S)) return keep;
    keep.resize(f_cut.size());
    for (size_t f = 0; f < f_cut.size(); ++f) {
        int32_t k = 0;
        while (k < spec.n_changepoints && spec.changepoint_ns[k] <= f_cut[f]) ++k;
        keep[f] = k;
    }
    return keep;
}

// the plan and the fold tables (host only)
static void cv_plan_call(const PanelIn &p, const tsf_cv_args &a, const tsf_spec *spec, CvCall *S)
{
    const int64_t N = p.N, *offsets = p.offsets, *ds = p.ds;
    const int32_t T = p.T;
    const double *floor_ = p.floor_, *cap = p.cap;
    cv_call_shape(p, spec, S);
    tsf_cv::panel_plan(N, T, offsets, ds, a, &S->plan, &S->pst, &S->pnh, &S->pnm);
    S->fold_off.assign((size_t)N + 1, 0); S->rows_off.assign((size_t)N + 1, 0); S->m_off.assign((size_t)N + 1, 0);
    for (int64_t n = 0; n < N; ++n) {
        S->fold_off[(size_t)n + 1] = S->fold_off[(size_t)n] + (int64_t)S->plan[(size_t)n].size();
        S->rows_off[(size_t)n + 1] = S->rows_off[(size_t)n] + S->pnh[(size_t)n];
        S->m_off[(size_t)n + 1] = S->m_off[(size_t)n] + S->pnm[(size_t)n];
    }
    const int64_t F = S->F = S->fold_off[(size_t)N];
    S->R = S->rows_off[(size_t)N]; S->M = S->m_off[(size_t)N];
    S->f_series.resize((size_t)F); S->f_c.resize((size_t)F);
    S->f_cut.resize((size_t)F); S->f_hist.resize((size_t)F); S->f_hold.resize((size_t)F); S->f_row0.resize((size_t)F);
    S->f_floor.resize(floor_ ? (size_t)F : 0); S->f_cap.resize(cap ? (size_t)F : 0);
    for (int64_t n = 0; n < N; ++n) {
        int64_t r = S->rows_off[(size_t)n];
        for (size_t c = 0; c < S->plan[(size_t)n].size(); ++c) {
            const int64_t f = S->fold_off[(size_t)n] + (int64_t)c;
            const tsf_cv::Fold &x = S->plan[(size_t)n][c];
            S->f_series[(size_t)f] = (int32_t)n; S->f_c[(size_t)f] = (int32_t)c;
            S->f_cut[(size_t)f] = x.cutoff; S->f_hist[(size_t)f] = x.hist; S->f_hold[(size_t)f] = x.hold; S->f_row0[(size_t)f] = r;
            if (floor_) S->f_floor[(size_t)f] = floor_[n];
            if (cap) S->f_cap[(size_t)f] = cap[n];
            r += x.hold;
            if (x.hold > S->Hmax) S->Hmax = (int32_t)x.hold;
        }
        if ((int32_t)S->plan[(size_t)n].size() > S->C) S->C = (int32_t)S->plan[(size_t)n].size();
    }
    S->f_keep = cv_fold_keep(*spec, S->f_cut);
}

// the caller's panel, once; the fold tables; the fold outputs in plan order
static int cv_upload(tsf_ctx *ctx, const int64_t *series_key, CvCall *S)
{
    const int64_t N = S->N, F = S->F, T = S->T;
    const int64_t n_ds = S->aligned ? T : S->offsets[N];
    const int64_t n_y = S->aligned ? N * T : S->offsets[N];
    HIP_TRY(ctx, S->d_ds.put(S->ds, 8 * (size_t)n_ds));
    HIP_TRY(ctx, S->d_y.put(S->y, S->ysz * (size_t)n_y));
    if (!S->aligned) HIP_TRY(ctx, S->d_off.put(S->offsets, 8 * ((size_t)N + 1)));
    if (S->n_extra > 0) HIP_TRY(ctx, S->d_ex.put(S->extra, 8 * (size_t)S->n_extra * n_ds));
    if (S->floor_) HIP_TRY(ctx, S->d_fl.put(S->floor_, 8 * (size_t)N));
    if (S->cap) HIP_TRY(ctx, S->d_cap.put(S->cap, 8 * (size_t)N));
    if (series_key) HIP_TRY(ctx, S->d_key.put(series_key, 8 * (size_t)N));
    if (F > 0) {                        // (tsf_tune uploads a panel without folds for its refit)
        HIP_TRY(ctx, S->d_fser.put(S->f_series.data(), 4 * (size_t)F));
        HIP_TRY(ctx, S->d_fc.put(S->f_c.data(), 4 * (size_t)F));
        HIP_TRY(ctx, S->d_fhist.put(S->f_hist.data(), 8 * (size_t)F));
        HIP_TRY(ctx, S->d_fhold.put(S->f_hold.data(), 8 * (size_t)F));
    }
    CvPanel &pn = S->pn;
    pn.ds = S->d_ds.as<int64_t>(); pn.y = S->d_y.p; pn.extra = S->n_extra > 0 ? S->d_ex.as<double>() : nullptr;
    pn.src_off = S->aligned ? nullptr : S->d_off.as<int64_t>(); pn.T = S->aligned ? T : 0;
    pn.src_total = S->aligned ? 0 : S->offsets[N];
    pn.ysz = (int)S->ysz; pn.n_extra = S->n_extra;
    return S->fit.alloc(ctx, F, S->stride, F, FIT_OUT_RAW);
}

static CvViews cv_fold_views(CvCall &S)
{
    return CvViews{S.d_fser.as<int32_t>(), S.f_series.data(), S.f_hist.data(), S.aligned ? S.f_c.data() : nullptr, S.C,
                   S.f_keep.empty() ? nullptr : S.f_keep.data()};
}

// the layout of a launch's panel over the members gf, member g with n_rows[gf[g]] rows: the list and the row offsets on
// the device, the panel's buffers allocated (for cv_expand_kernel or screen_compact_kernel to fill)
static int cv_group_layout(tsf_ctx *ctx, const CvCall &S, const std::vector<int32_t> &gf, const int64_t *n_rows, CvGroup *E)
{
    const size_t G = gf.size();
    E->G = (int64_t)G;
    E->gf = gf;
    E->goff.assign(G + 1, 0);
    for (size_t g = 0; g < G; ++g) {
        const int64_t h = n_rows[(size_t)gf[g]];
        E->goff[g + 1] = E->goff[g] + h;
        if (h > E->maxT) E->maxT = (int32_t)h;
    }
    const size_t rows = (size_t)(E->rows = E->goff[G]);
    if (G == 0) return 0;
    HIP_TRY(ctx, E->d_gf.put(gf.data(), 4 * G));
    HIP_TRY(ctx, E->d_goff.put(E->goff.data(), 8 * (G + 1)));
    HIP_TRY(ctx, E->d_gds.alloc(8 * rows)); HIP_TRY(ctx, E->d_gy.alloc(S.ysz * rows));
    if (S.n_extra > 0) HIP_TRY(ctx, E->d_gex.alloc(8 * (size_t)S.n_extra * rows));
    if (S.has_floor) HIP_TRY(ctx, E->d_gfl.alloc(8 * G));
    if (S.has_cap) HIP_TRY(ctx, E->d_gcap.alloc(8 * G));
    return 0;
}

// the panel of one fit launch over the views gf (cv_expand_kernel) and its calendar classes (fit_host_one's rule:
// ragged, no explicit columns, two views or more; the tables through upload_calendar_tables as there)
static int cv_expand(tsf_ctx *ctx, CvCall &S, const CvViews &V, const std::vector<int32_t> &gf, CvGroup *E)
{
    if (int rc = cv_group_layout(ctx, S, gf, V.hist, E)) return rc;
    const int64_t G = E->G, rows = E->rows;
    const std::vector<int64_t> &goff = E->goff;
    if (G == 0) return 0;
    hipLaunchKernelGGL(cv_expand_kernel, dim3((unsigned)(G < 65535 ? G : 65535)), dim3(256), 0, nullptr, S.pn, G,
                       E->d_gf.as<int32_t>(), V.d_series, E->d_goff.as<int64_t>(), rows,
                       S.has_floor ? S.d_fl.as<double>() : nullptr, S.has_cap ? S.d_cap.as<double>() : nullptr,
                       E->d_gds.as<int64_t>(), E->d_gy.p, S.n_extra > 0 ? E->d_gex.as<double>() : nullptr,
                       S.has_floor ? E->d_gfl.as<double>() : nullptr, S.has_cap ? E->d_gcap.as<double>() : nullptr);
    HIP_TRY(ctx, hipGetLastError());
    int64_t n_distinct = 0;
    if (S.n_extra == 0 && G >= 2 && ctx->opt[TSF_OPT_GRID_SHARE] != 0) {
        std::vector<int32_t> gof((size_t)G);
        std::vector<int64_t> reps;
        if (V.cls) {
            std::vector<int32_t> id_of((size_t)V.n_cls, -1);
            for (int64_t g = 0; g < G; ++g) {
                const int32_t c = V.cls[(size_t)gf[(size_t)g]];
                if (id_of[(size_t)c] < 0) { id_of[(size_t)c] = (int32_t)reps.size(); reps.push_back(g); }
                gof[(size_t)g] = id_of[(size_t)c];
            }
        } else {
            std::vector<int64_t> vstart((size_t)G), vlen((size_t)G);
            for (int64_t g = 0; g < G; ++g) {
                vstart[(size_t)g] = S.offsets[V.series[(size_t)gf[(size_t)g]]];
                vlen[(size_t)g] = V.hist[(size_t)gf[(size_t)g]];
            }
            calendar_classes(S.ds, vstart.data(), vlen.data(), G, &gof, &reps);
        }
        if (V.keep) {
            // views that share a timestamp vector share a grid only where they keep the same number of dates (two series
            // of one calendar whose cutoffs differ): split the classes that do not
            std::map<std::pair<int32_t, int32_t>, int32_t> ids;
            std::vector<int64_t> reps2;
            for (int64_t g = 0; g < G; ++g) {
                const auto key = std::make_pair(gof[(size_t)g], V.keep[(size_t)gf[(size_t)g]]);
                auto it = ids.find(key);
                if (it == ids.end()) { it = ids.emplace(key, (int32_t)reps2.size()).first; reps2.push_back(g); }
                gof[(size_t)g] = it->second;
            }
            reps.swap(reps2);
        }
        if (int rc = upload_calendar_tables(ctx, gof, reps, goff.data(), &E->d_gof, &E->d_grows, &E->d_gord, &n_distinct))
            return rc;
        if (V.keep && n_distinct > 0) {
            std::vector<int32_t> kp;
            for (int64_t r : reps) kp.push_back(V.keep[(size_t)gf[(size_t)r]]);
            HIP_TRY(ctx, E->d_gkeep.put(kp.data(), 4 * kp.size()));
        }
    }
    if (V.keep && n_distinct == 0) {        // a grid per view
        std::vector<int32_t> kp((size_t)G);
        for (int64_t g = 0; g < G; ++g) kp[(size_t)g] = V.keep[(size_t)gf[(size_t)g]];
        HIP_TRY(ctx, E->d_gkeep.put(kp.data(), 4 * (size_t)G));
    }
    E->n_distinct = n_distinct;
    return 0;
}

// one fit launch over an expanded group with spec gs, its outputs scattered to dst at the views' indices
static int cv_fit(tsf_ctx *ctx, CvCall &S, CvGroup &E, const tsf_spec &gs, const tsf_fit_out &dst, int64_t *n_grids,
                  int32_t *n_launches)
{
    const int64_t G = E.G;
    if (G == 0) return 0;
    const int stride = S.stride;
    DevFitOut launch;
    if (int rc = launch.alloc(ctx, G, stride, G, FIT_OUT_LAUNCH)) return rc;
    tsf_fit_out go = launch.view();
    const int64_t nd = E.n_distinct;
    FitCall c = {};
    c.N = G; c.offsets = E.d_goff.as<int64_t>(); c.total_rows = E.rows; c.max_T = E.maxT;
    c.ds = E.d_gds.as<int64_t>(); c.y = E.d_gy.p; c.y_dtype = S.y_dtype;
    if (S.has_floor) c.floor = E.d_gfl.as<double>();
    if (S.has_cap) c.cap = E.d_gcap.as<double>();
    if (S.n_extra > 0) c.extra = E.d_gex.as<double>();
    if (nd > 0) { c.grid_of = E.d_gof.as<int32_t>(); c.grid_rows = E.d_grows.as<int64_t>(); c.grid_order = E.d_gord.as<int32_t>(); }
    c.n_distinct = nd;
    if (E.d_gkeep.p) c.grid_keep = E.d_gkeep.as<int32_t>();
    int rc = run_fit(ctx, &gs, c, &go);
    if (rc) return rc;
    *n_grids += ctx->last_plan.n_grids;
    *n_launches += 1;
    hipLaunchKernelGGL(cv_scatter_kernel, dim3((unsigned)G), dim3(64), 0, nullptr, G, E.d_gf.as<int32_t>(), stride, go, dst);
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, hipDeviceSynchronize());       // (this launch's buffers go back to the pool)
    return 0;
}

// ---- fbprophet's optimiser rule (include/tsf.h, TSF_ALGO_AUTO) ---------------------------------------------------
// Newton for a history of fewer than TSF_NEWTON_BELOW_T rows, L-BFGS otherwise, Newton once more where L-BFGS ended
// the way pystan raises RuntimeError on -- for models Newton takes (at most TSF_MAX_P parameters).  TSF_ALGO_LBFGS /
// TSF_ALGO_NEWTON: every member on that optimiser, nothing retried.  The one implementation, for the folds of a
// cross-validation, calibration or tuning and the series of tsf_tune's refit and of tsf_fit_screened's rounds.
struct OptimiserGroups { std::vector<int32_t> lbfgs, newton; };
enum RuleLaunch { RULE_LBFGS, RULE_RETRY, RULE_NEWTON };        // the launches of the rule, in their order

static bool newton_takes(const tsf_spec &s) { return 3 + s.n_changepoints + tsf_spec_K(&s) <= TSF_MAX_P; }
// the n members members[i] (null: 0 .. n - 1) split by their row counts rows[member]
static OptimiserGroups optimiser_groups(const tsf_spec &spec, const int32_t *members, size_t n, const int64_t *rows)
{
    OptimiserGroups g;
    const bool auto_algo = spec.algorithm == TSF_ALGO_AUTO, newton_ok = newton_takes(spec);
    for (size_t i = 0; i < n; ++i) {
        const int32_t m = members ? members[i] : (int32_t)i;
        const bool nw = auto_algo ? (newton_ok && rows[m] < TSF_NEWTON_BELOW_T) : spec.algorithm == TSF_ALGO_NEWTON;
        (nw ? g.newton : g.lbfgs).push_back(m);
    }
    return g;
}

// the members of `sel` whose L-BFGS fit (status in `st`, indexed by member) ended the way pystan raises RuntimeError on
static std::vector<int32_t> newton_retry(const std::vector<int32_t> &sel, const std::vector<int32_t> &st)
{
    std::vector<int32_t> retry;
    for (int32_t f : sel) {
        const int32_t s = st[(size_t)f];
        if (s == TSF_ST_LSFAIL || s == TSF_ST_INIT_NONFINITE || s == TSF_ST_EVAL_LIMIT) retry.push_back(f);
    }
    return retry;
}

// The rule's launches through fit_group(the launch's spec, its members, which launch): the L-BFGS group, those of it
// to retry (by the statuses the first launch left in dst, indexed by member), the Newton group; an empty list launches
// nothing.  `which` lets tsf_tune, which cuts the two groups' panels once for all candidates, tell them from a retry.
template <class FitGroup>
static int fit_by_rule(tsf_ctx *ctx, const tsf_spec &spec, const OptimiserGroups &g, const DevFitOut &dst, FitGroup fit_group)
{
    tsf_spec sp_l = spec, sp_n = spec;
    sp_l.algorithm = TSF_ALGO_LBFGS;
    sp_n.algorithm = TSF_ALGO_NEWTON;
    if (!g.lbfgs.empty()) {
        if (int rc = fit_group(sp_l, g.lbfgs, RULE_LBFGS)) return rc;
        if (spec.algorithm == TSF_ALGO_AUTO && newton_takes(spec)) {
            std::vector<int32_t> st(dst.n);
            HIP_TRY(ctx, hipMemcpy(st.data(), dst.status.p, 4 * dst.n, hipMemcpyDeviceToHost));
            const std::vector<int32_t> retry = newton_retry(g.lbfgs, st);
            if (!retry.empty())
                if (int rc = fit_group(sp_n, retry, RULE_RETRY)) return rc;
        }
    }
    return g.newton.empty() ? 0 : fit_group(sp_n, g.newton, RULE_NEWTON);
}

static int cv_holdout(tsf_ctx *ctx, CvCall &S, const int64_t *series_key, CvHoldout *H)
{
    const int64_t F = S.F;
    const int32_t Hmax = S.Hmax;
    HIP_TRY(ctx, H->d_fds.alloc(8 * (size_t)F * Hmax));
    if (S.n_extra > 0) HIP_TRY(ctx, H->d_fex.alloc(8 * (size_t)F * S.n_extra * Hmax));
    HIP_TRY(ctx, H->d_fkey.alloc(8 * (size_t)F));
    if (S.has_floor) HIP_TRY(ctx, H->d_ffl.put(S.f_floor.data(), 8 * (size_t)F));
    if (S.has_cap) HIP_TRY(ctx, H->d_fcap.put(S.f_cap.data(), 8 * (size_t)F));
    hipLaunchKernelGGL(cv_holdout_kernel, dim3((unsigned)(F < 65535 ? F : 65535)), dim3(128), 0, nullptr, S.pn, F, Hmax,
                       S.d_fser.as<int32_t>(), S.d_fc.as<int32_t>(), S.d_fhist.as<int64_t>(), S.d_fhold.as<int64_t>(),
                       series_key ? S.d_key.as<int64_t>() : nullptr, H->d_fds.as<int64_t>(),
                       S.n_extra > 0 ? H->d_fex.as<double>() : nullptr, H->d_fkey.as<int64_t>());
    HIP_TRY(ctx, hipGetLastError());
    return 0;
}

// cv_metrics_kernel's arguments over the holdout forecasts yhat (and lo / hi: intervals) [F][Hmax]
static int cv_metrics_setup(tsf_ctx *ctx, CvCall &S, const double *yhat, const double *lo, const double *hi,
                            double rolling_window, CvMetrics *X)
{
    const int64_t N = S.N, F = S.F, R = S.R, M = S.M;
    const bool iv = lo != nullptr;
    HIP_TRY(ctx, X->d_foff.put(S.fold_off.data(), 8 * ((size_t)N + 1)));
    HIP_TRY(ctx, X->d_roff.put(S.rows_off.data(), 8 * ((size_t)N + 1)));
    HIP_TRY(ctx, X->d_moff.put(S.m_off.data(), 8 * ((size_t)N + 1)));
    HIP_TRY(ctx, X->d_fcut.put(S.f_cut.data(), 8 * (size_t)F));
    HIP_TRY(ctx, X->d_frow0.put(S.f_row0.data(), 8 * (size_t)F));
    HIP_TRY(ctx, X->d_hs.alloc(8 * (size_t)R)); HIP_TRY(ctx, X->d_ts.alloc(8 * 4 * (size_t)R)); HIP_TRY(ctx, X->d_pre.alloc(8 * 4 * (size_t)(R + 64 * N)));
    HIP_TRY(ctx, X->d_yo.alloc(8 * (size_t)R));
    if (iv) { HIP_TRY(ctx, X->d_loo.alloc(8 * (size_t)R)); HIP_TRY(ctx, X->d_hio.alloc(8 * (size_t)R)); }
    HIP_TRY(ctx, X->d_mh.alloc(8 * (size_t)M)); HIP_TRY(ctx, X->d_mm.alloc(8 * 5 * (size_t)M));
    HIP_TRY(ctx, X->d_sst.put(S.pst.data(), 4 * (size_t)N));
    CvMetricArgs &ma = X->ma;
    memset(&ma, 0, sizeof(ma));
    ma.p = S.pn; ma.y_dtype = S.y_dtype; ma.N = N; ma.Hmax = S.Hmax;
    ma.fold_off = X->d_foff.as<int64_t>(); ma.rows_off = X->d_roff.as<int64_t>(); ma.m_off = X->d_moff.as<int64_t>();
    ma.cutoff = X->d_fcut.as<int64_t>(); ma.fold_hist = S.d_fhist.as<int64_t>(); ma.fold_hold = S.d_fhold.as<int64_t>();
    ma.fold_row0 = X->d_frow0.as<int64_t>(); ma.fit_status = S.fit.status.as<int32_t>();
    ma.yhat = yhat; ma.lo = lo; ma.hi = hi;
    ma.rolling_window = rolling_window;
    ma.h_s = X->d_hs.as<int64_t>(); ma.t_s = X->d_ts.as<double>(); ma.pre = X->d_pre.as<double>(); ma.R = R;
    ma.yhat_out = X->d_yo.as<double>(); ma.lo_out = iv ? X->d_loo.as<double>() : nullptr; ma.hi_out = iv ? X->d_hio.as<double>() : nullptr;
    double *mm = X->d_mm.as<double>();
    ma.horizon = X->d_mh.as<int64_t>(); ma.mse = mm; ma.rmse = mm + M; ma.mae = mm + 2 * M; ma.mape = mm + 3 * M;
    ma.coverage = mm + 4 * M; ma.series_status = X->d_sst.as<int32_t>();
    return 0;
}

static int calib_run(tsf_ctx *ctx, int64_t N, const int64_t *d_off, const int64_t *h_off, const int64_t *d_h, const double *d_y,
                     const double *d_yhat, const double *d_lower, const double *d_upper, const tsf_calib_args &a,
                     const tsf_calib_table &o, hipStream_t st);
static int calib_no_table(const tsf_calib_args &a, int64_t N, const tsf_calib_table &t);

// what every panel job asks of its panel (max_N: tsf_fit_screened's lists index the series in 32 bits)
static int check_panel_in(tsf_ctx *ctx, const tsf_spec *spec, const PanelIn &p, int64_t max_N = INT64_MAX)
{
    if (p.N > max_N || tsf_cv::check_panel(p.N, p.T, p.offsets, p.ds))
        return fail(ctx, "bad panel (aligned: offsets NULL, 1 <= T <= TSF_MAX_T; ragged: T = 0, offsets[0] = 0, ascending)");
    if (spec->n_extra > 0 && !p.extra) return fail(ctx, "extra columns declared but extra is NULL");
    if (spec->growth == TSF_GROWTH_LOGISTIC && !p.cap) return fail(ctx, "logistic growth needs cap");
    return 0;
}

// ---- the steps of cross_validate_run -----------------------------------------------------------------------------

// the arguments, before the plan: *a = the cross-validation arguments with their defaults filled in
static int cv_check_args(tsf_ctx *ctx, const tsf_spec *spec, const PanelIn &p, const tsf_cv_args *args, int32_t n_samples,
                         double interval_width, const tsf_cv_out *out, const tsf_calib_args *cal, tsf_cv_args *a)
{
    if (!spec || !p.ds || !p.y || (!cal && !out) || (out && !out->series_status)) return fail(ctx, "NULL input");
    if (p.y_dtype < TSF_Y_F64 || p.y_dtype > TSF_Y_I32) return fail(ctx, "bad y_dtype");
    if (tsf_cv::resolve_args(args, a)) return fail(ctx, "bad cross-validation arguments (horizon_ns > 0, rolling_window in [0, 1])");
    if (int rc = check_panel_in(ctx, spec, p)) return rc;
    const bool iv = n_samples > 0;
    if (iv && (n_samples < 2 || n_samples > 4096)) return fail(ctx, "n_samples must be 0 or in [2, 4096]");
    if (iv && !(interval_width > 0.0 && interval_width < 1.0)) return fail(ctx, "interval_width must be in (0, 1)");
    if (cal) {
        if (cal->horizon_ns != a->horizon_ns) return fail(ctx, "tsf_calib_args.horizon_ns must equal the cross-validation's horizon");
        if (cal->mode == TSF_CALIB_CQR && !(cal->n_levels == 1 && iv && cal->levels[0] == interval_width))
            return fail(ctx, "TSF_CALIB_CQR needs n_levels == 1, n_samples > 0 and levels[0] == interval_width");
    }
    return check_algorithm(ctx, spec);
}

// every fold fitted by the optimiser rule, one launch per group over its fold panel, the outputs in S.fit
static int cv_fit_folds(tsf_ctx *ctx, CvCall &S, const tsf_spec &spec)
{
    const CvViews folds = cv_fold_views(S);
    const tsf_fit_out dst = S.fit.view();
    return fit_by_rule(ctx, spec, optimiser_groups(spec, nullptr, (size_t)S.F, S.f_hist.data()), S.fit,
                       [&](const tsf_spec &gs, const std::vector<int32_t> &gf, RuleLaunch) -> int {
                           CvGroup E;
                           if (int rc = cv_expand(ctx, S, folds, gf, &E)) return rc;
                           return cv_fit(ctx, S, E, gs, dst, &ctx->cv_grids, &ctx->cv_launches);
                       });
}

// the holdout rows of every fold predicted in one call (n_samples > 0: with intervals), then the metrics per series
static int cv_forecast_and_score(tsf_ctx *ctx, CvCall &S, const tsf_spec *spec, const int64_t *series_key, int32_t n_samples,
                                 double interval_width, uint64_t seed, double rolling_window)
{
    const int64_t F = S.F;
    const int32_t Hmax = S.Hmax;
    const bool iv = n_samples > 0;
    const tsf_fit_out fit = S.fit.view();
    HIP_TRY(ctx, S.d_yh.alloc(8 * (size_t)F * Hmax));
    if (iv) { HIP_TRY(ctx, S.d_lo.alloc(8 * (size_t)F * Hmax)); HIP_TRY(ctx, S.d_hi.alloc(8 * (size_t)F * Hmax)); }
    if (int rc = cv_holdout(ctx, S, series_key, &S.hold)) return rc;
    const CvHoldout &H = S.hold;
    const double *pfl = S.has_floor ? H.d_ffl.as<double>() : nullptr, *pcap = S.has_cap ? H.d_fcap.as<double>() : nullptr;
    const double *pex = spec->n_extra > 0 ? H.d_fex.as<double>() : nullptr;
    const int rc = iv ? tsf_predict_intervals_dev(ctx, spec, F, Hmax, fit.theta, fit.y_scale, fit.grid, (int32_t)F,
                                                  H.d_fds.as<int64_t>(), 0, pfl, pcap, pex, H.d_fkey.as<int64_t>(), n_samples,
                                                  interval_width, seed, S.d_yh.as<double>(), S.d_lo.as<double>(),
                                                  S.d_hi.as<double>(), nullptr)
                      : tsf_predict_dev(ctx, spec, F, Hmax, fit.theta, fit.y_scale, fit.grid, (int32_t)F, H.d_fds.as<int64_t>(),
                                        0, pfl, pcap, pex, S.d_yh.as<double>(), nullptr, nullptr);
    if (rc) return rc;
    if (int rc2 = cv_metrics_setup(ctx, S, S.d_yh.as<double>(), iv ? S.d_lo.as<double>() : nullptr,
                                   iv ? S.d_hi.as<double>() : nullptr, rolling_window, &S.met))
        return rc2;
    hipLaunchKernelGGL(cv_metrics_kernel, dim3((unsigned)S.N), dim3(64), 0, nullptr, S.met.ma);
    HIP_TRY(ctx, hipGetLastError());
    return 0;
}

// tsf_calibrate's tail: the rule on the device's own holdout rows -- horizon and y per row, then the table; only it
// crosses back
static int cv_calibration_tail(tsf_ctx *ctx, const CvCall &S, bool iv, const tsf_calib_args &cal, const tsf_calib_table &tab)
{
    const CvMetrics &X = S.met;
    const int64_t N = S.N, R = S.R;
    const int cells = (cal.n_buckets + 1) * cal.n_levels;
    DevBuf d_rh, d_ry, d_q, d_n, d_cst;
    HIP_TRY(ctx, d_rh.alloc(8 * (size_t)R)); HIP_TRY(ctx, d_ry.alloc(8 * (size_t)R));
    HIP_TRY(ctx, d_q.alloc(8 * (size_t)N * cells)); HIP_TRY(ctx, d_n.alloc(4 * (size_t)N * cells)); HIP_TRY(ctx, d_cst.alloc(4 * (size_t)N));
    hipLaunchKernelGGL(calib_cv_rows_kernel, dim3((unsigned)(N < 65535 ? N : 65535)), dim3(256), 0, nullptr, X.ma,
                       d_rh.as<int64_t>(), d_ry.as<double>());
    HIP_TRY(ctx, hipGetLastError());
    const tsf_calib_table dt{d_q.as<double>(), d_n.as<int32_t>(), d_cst.as<int32_t>()};
    if (int rc = calib_run(ctx, N, X.d_roff.as<int64_t>(), S.rows_off.data(), d_rh.as<int64_t>(), d_ry.as<double>(),
                           X.d_yo.as<double>(), iv ? X.d_loo.as<double>() : nullptr, iv ? X.d_hio.as<double>() : nullptr,
                           cal, dt, nullptr))
        return rc;
    hipLaunchKernelGGL(calib_mask_kernel, dim3((unsigned)(N < 65535 ? N : 65535)), dim3(256), 0, nullptr, N, cells,
                       X.d_sst.as<int32_t>(), dt.q, dt.n, dt.status);
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, hipDeviceSynchronize());
    HIP_TRY(ctx, hipMemcpy(tab.q, d_q.p, 8 * (size_t)N * cells, hipMemcpyDeviceToHost));
    HIP_TRY(ctx, hipMemcpy(tab.n, d_n.p, 4 * (size_t)N * cells, hipMemcpyDeviceToHost));
    HIP_TRY(ctx, hipMemcpy(tab.status, d_cst.p, 4 * (size_t)N, hipMemcpyDeviceToHost));
    return 0;
}

// the fold fits, the holdout forecasts, the metric rows and the series statuses to the caller's arrays
static int cv_download(tsf_ctx *ctx, const CvCall &S, bool iv, const tsf_cv_out &out)
{
    const CvMetrics &X = S.met;
    const size_t N = (size_t)S.N, R = (size_t)S.R, M = (size_t)S.M;
    if (int rc = S.fit.download(ctx, out.fit, S.F)) return rc;
    HIP_TRY(ctx, hipMemcpy(out.yhat, X.d_yo.p, 8 * R, hipMemcpyDeviceToHost));
    if (iv) {
        HIP_TRY(ctx, hipMemcpy(out.yhat_lower, X.d_loo.p, 8 * R, hipMemcpyDeviceToHost));
        HIP_TRY(ctx, hipMemcpy(out.yhat_upper, X.d_hio.p, 8 * R, hipMemcpyDeviceToHost));
    }
    if (M > 0) {
        const double *mm = X.d_mm.as<double>();
        HIP_TRY(ctx, hipMemcpy(out.horizon_ns, X.d_mh.p, 8 * M, hipMemcpyDeviceToHost));
        HIP_TRY(ctx, hipMemcpy(out.mse, mm, 8 * M, hipMemcpyDeviceToHost));
        HIP_TRY(ctx, hipMemcpy(out.rmse, mm + M, 8 * M, hipMemcpyDeviceToHost));
        HIP_TRY(ctx, hipMemcpy(out.mae, mm + 2 * M, 8 * M, hipMemcpyDeviceToHost));
        HIP_TRY(ctx, hipMemcpy(out.mape, mm + 3 * M, 8 * M, hipMemcpyDeviceToHost));
        if (iv) HIP_TRY(ctx, hipMemcpy(out.coverage, mm + 4 * M, 8 * M, hipMemcpyDeviceToHost));
    }
    HIP_TRY(ctx, hipMemcpy(out.series_status, X.d_sst.p, 4 * N, hipMemcpyDeviceToHost));
    return 0;
}

// tsf_cross_validate (cal == nullptr: out required) and tsf_calibrate (cal and tab given, checked by the caller: the rule
// runs on the device's holdout rows behind the metrics, and out may be null: then only the table crosses back)
static int cross_validate_run(tsf_ctx *ctx, const tsf_spec *spec, const PanelIn &p, const tsf_cv_args *args,
                              const int64_t *series_key, int32_t n_samples, double interval_width, uint64_t seed,
                              tsf_cv_out *out, const tsf_calib_args *cal, const tsf_calib_table *tab)
{
    // with intervals the folds' holdout rows are drawn (through tsf_predict_intervals_dev, which would take the setting)
    NoiseArOnce ar_once(n_samples > 0 ? ctx : nullptr);
    if (n_samples > 0)
        if (int rc = refuse_noise_ar(ctx, "cross-validation / calibration with intervals")) return rc;
    tsf_cv_args a;
    if (int rc = cv_check_args(ctx, spec, p, args, n_samples, interval_width, out, cal, &a)) return rc;
    const bool iv = n_samples > 0;
    ctx->order_n = 0;                   // (pending cost hints were meant for a fit call)
    ctx->cv_grids = 0;
    ctx->cv_launches = 0;
    CvCall S;
    cv_plan_call(p, a, spec, &S);
    if (out) memcpy(out->series_status, S.pst.data(), sizeof(int32_t) * (size_t)p.N);
    if (S.F == 0) return cal ? calib_no_table(*cal, p.N, *tab) : 0;
    if (out) {
        if (!fit_out_complete(out->fit)) return fail(ctx, "tsf_cv_out.fit has NULL members");
        if (!out->yhat || !out->horizon_ns || !out->mse || !out->rmse || !out->mae || !out->mape ||
            (iv && (!out->yhat_lower || !out->yhat_upper || !out->coverage)))
            return fail(ctx, "tsf_cv_out has NULL members");
    }
    if (int rc = cv_upload(ctx, series_key, &S)) return rc;
    if (int rc = cv_fit_folds(ctx, S, *spec)) return rc;
    if (int rc = cv_forecast_and_score(ctx, S, spec, series_key, n_samples, interval_width, seed, a.rolling_window)) return rc;
    if (cal) {
        if (int rc = cv_calibration_tail(ctx, S, iv, *cal, *tab)) return rc;
        if (!out) return 0;
    }
    HIP_TRY(ctx, hipDeviceSynchronize());
    return cv_download(ctx, S, iv, *out);
}

extern "C" int tsf_cross_validate(tsf_ctx *ctx, const tsf_spec *spec, int64_t N, int32_t T, const int64_t *offsets,
                                  const int64_t *ds, const void *y, int32_t y_dtype, const double *floor_,
                                  const double *cap, const double *extra, const tsf_cv_args *args,
                                  const int64_t *series_key, int32_t n_samples, double interval_width, uint64_t seed,
                                  tsf_cv_out *out)
{
    if (!ctx) return -1;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    return cross_validate_run(ctx, spec, PanelIn{N, T, offsets, ds, y, y_dtype, floor_, cap, extra}, args, series_key,
                              n_samples, interval_width, seed, out, nullptr, nullptr);
}

// The identity views of an uploaded panel -- view n = every row of series n -- for the launches that fit whole
// histories (tsf_tune's refit, tsf_fit_screened's first fit).
struct WholeViews {
    std::vector<int32_t> ident;
    std::vector<int64_t> len;           // rows per series
    int64_t max_len = 0;
    DevBuf d_ident;                     // (ragged panels: cv_expand_kernel reads it; an aligned panel is gathered by rows)

    int build(tsf_ctx *ctx, const CvCall &S)
    {
        const size_t N = (size_t)S.N;
        ident.resize(N);
        len.resize(N);
        for (size_t n = 0; n < N; ++n) {
            ident[n] = (int32_t)n;
            len[n] = S.aligned ? S.T : S.offsets[n + 1] - S.offsets[n];
            if (len[n] > max_len) max_len = len[n];
        }
        if (!S.aligned) HIP_TRY(ctx, d_ident.put(ident.data(), 4 * N));
        return 0;
    }
    CvViews views() const { return CvViews{d_ident.as<int32_t>(), ident.data(), len.data(), nullptr, 0, nullptr}; }
};

// One fit launch over the whole histories of the series sel of an uploaded panel with spec gs, its outputs put at the
// series' positions of dst (tsf_tune's refit, tsf_fit_screened's first fit): aligned, the series' rows gathered into a
// [G][T] panel (tune_gather_kernel; dst.grid[0] receives the one grid); ragged, their full histories as views
// (cv_expand_kernel; dst.grid[n] per series).  whole: the identity views of the panel.
static int fit_whole_group(tsf_ctx *ctx, CvCall &S, const CvViews &whole, const tsf_spec &gs, const std::vector<int32_t> &sel,
                           const tsf_fit_out &dst, int64_t *n_grids, int32_t *n_launches)
{
    const int64_t G = (int64_t)sel.size();
    if (G == 0) return 0;
    if (!S.aligned) {
        CvGroup E;
        if (int rc = cv_expand(ctx, S, whole, sel, &E)) return rc;
        return cv_fit(ctx, S, E, gs, dst, n_grids, n_launches);
    }
    const int32_t T = S.T;
    const int stride = S.stride;
    DevBuf d_sel, d_gy, d_gfl, d_gcap;
    HIP_TRY(ctx, d_sel.put(sel.data(), 4 * (size_t)G));
    HIP_TRY(ctx, d_gy.alloc(S.ysz * (size_t)G * T));
    if (S.has_floor) HIP_TRY(ctx, d_gfl.alloc(8 * (size_t)G));
    if (S.has_cap) HIP_TRY(ctx, d_gcap.alloc(8 * (size_t)G));
    hipLaunchKernelGGL(tune_gather_kernel, dim3((unsigned)(G < 65535 ? G : 65535)), dim3(256), 0, nullptr, S.pn, G,
                       d_sel.as<int32_t>(), S.has_floor ? S.d_fl.as<double>() : nullptr, S.has_cap ? S.d_cap.as<double>() : nullptr,
                       d_gy.p, S.has_floor ? d_gfl.as<double>() : nullptr, S.has_cap ? d_gcap.as<double>() : nullptr);
    HIP_TRY(ctx, hipGetLastError());
    DevFitOut launch;
    if (int rc = launch.alloc(ctx, G, stride, 1, FIT_OUT_LAUNCH)) return rc;
    tsf_fit_out go = launch.view();
    FitCall c = {};
    c.N = G; c.aligned = 1; c.T = T; c.max_T = T;
    c.ds = S.d_ds.as<int64_t>(); c.y = d_gy.p; c.y_dtype = S.y_dtype;
    if (S.has_floor) c.floor = d_gfl.as<double>();
    if (S.has_cap) c.cap = d_gcap.as<double>();
    if (S.n_extra > 0) c.extra = S.d_ex.as<double>();
    int rc = run_fit(ctx, &gs, c, &go);
    if (rc) return rc;
    *n_launches += 1;
    hipLaunchKernelGGL(tune_scatter_kernel, dim3((unsigned)G), dim3(64), 0, nullptr, G, d_sel.as<int32_t>(), stride, go, dst);
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, hipDeviceSynchronize());
    return 0;
}

// ---- prior-scale tuning (include/tsf.h) ---------------------------------------------------------------

extern "C" int tsf_last_tune_counts(const tsf_ctx *ctx, int32_t *expand_launches, int32_t *fit_launches)
{
    if (!ctx || !expand_launches || !fit_launches) return -1;
    *expand_launches = ctx->tune_expand;
    *fit_launches = ctx->tune_fits;
    return 0;
}

// every optimiser field of a and b equal (what tsf_select asks of its candidates beside n_extra)
static bool same_optimiser(const tsf_spec &a, const tsf_spec &b)
{
    return a.max_iter == b.max_iter && a.history == b.history && a.init_alpha == b.init_alpha && a.tol_obj == b.tol_obj &&
           a.tol_rel_obj == b.tol_rel_obj && a.tol_grad == b.tol_grad && a.tol_rel_grad == b.tol_rel_grad &&
           a.tol_param == b.tol_param && a.eval_form == b.eval_form && a.recenter_every == b.recenter_every &&
           a.recenter_ratio == b.recenter_ratio && a.algorithm == b.algorithm && a.residual_kernel == b.residual_kernel &&
           a.coop_after == b.coop_after && a.converge == b.converge && a.map_max_iter == b.map_max_iter &&
           a.map_tol == b.map_tol;
}

// every field of a and b equal except the prior scales (the columns' entries only)
static bool same_but_prior_scales(const tsf_spec &a, const tsf_spec &b)
{
    if (a.growth != b.growth || a.n_changepoints != b.n_changepoints || a.changepoint_range != b.changepoint_range ||
        a.n_seas != b.n_seas || a.n_extra != b.n_extra || a.changepoints_specified != b.changepoints_specified)
        return false;
    if (a.changepoints_specified && a.n_changepoints >= 0 && a.n_changepoints <= TSF_MAX_S)
        for (int j = 0; j < a.n_changepoints; ++j)
            if (a.changepoint_ns[j] != b.changepoint_ns[j]) return false;
    if (a.n_seas < 0 || a.n_seas > TSF_MAX_SEAS || a.n_extra < 0 || a.n_extra > TSF_MAX_EXTRA) return false;
    for (int i = 0; i < a.n_seas; ++i)
        if (a.seas_period[i] != b.seas_period[i] || a.seas_order[i] != b.seas_order[i] || a.seas_mode[i] != b.seas_mode[i])
            return false;
    for (int i = 0; i < a.n_extra; ++i)
        if (a.extra_mode[i] != b.extra_mode[i]) return false;
    return same_optimiser(a, b);
}

static bool prior_scales_ok(const tsf_spec &s)
{
    auto ok = [](double v) { return std::isfinite(v) && v > 0.0; };
    if (!ok(s.changepoint_prior_scale)) return false;
    for (int i = 0; i < s.n_seas; ++i) if (!ok(s.seas_prior_scale[i])) return false;
    for (int i = 0; i < s.n_extra; ++i) if (!ok(s.extra_prior_scale[i])) return false;
    return true;
}

// ---- the steps of tsf_tune ------------------------------------------------------------------------------------------

// *a = the cross-validation arguments with their defaults filled in and one metric row per series
static int tune_check_args(tsf_ctx *ctx, const tsf_spec *base, const tsf_spec *cand, int32_t C, const PanelIn &p,
                           const tsf_cv_args *cv, int32_t metric, int32_t refit, const tsf_tune_out *out, tsf_cv_args *a)
{
    if (!base || !cand || !p.ds || !p.y || !out || !out->score || !out->cand_status || !out->best || !out->series_status)
        return fail(ctx, "NULL input");
    if (C < 1 || C > TSF_TUNE_MAX_CAND) return fail(ctx, "C must be in [1, TSF_TUNE_MAX_CAND]");
    if (metric < TSF_TUNE_MSE || metric > TSF_TUNE_MAPE) return fail(ctx, "bad metric (TSF_TUNE_MSE .. TSF_TUNE_MAPE)");
    if (refit != 0 && refit != 1) return fail(ctx, "refit must be 0 or 1");
    if (p.y_dtype < TSF_Y_F64 || p.y_dtype > TSF_Y_I32) return fail(ctx, "bad y_dtype");
    if (!cv) return fail(ctx, "cv is NULL");
    tsf_cv_args cv1 = *cv;
    cv1.rolling_window = 1.0;           // one metric row per series, over all its holdout rows
    if (tsf_cv::resolve_args(&cv1, a)) return fail(ctx, "bad cross-validation arguments (horizon_ns > 0)");
    if (int rc = check_panel_in(ctx, base, p)) return rc;
    if (!prior_scales_ok(*base)) return fail(ctx, "base: prior scales must be finite and > 0");
    for (int32_t c = 0; c < C; ++c) {
        if (!same_but_prior_scales(*base, cand[c]))
            return fail(ctx, "a candidate differs from base in more than its prior scales");
        if (!prior_scales_ok(cand[c])) return fail(ctx, "a candidate's prior scales must be finite and > 0");
    }
    if (refit && !fit_out_complete(out->fit)) return fail(ctx, "tsf_tune_out.fit has NULL members");
    return check_algorithm(ctx, base);      // (the candidates' is base's)
}

struct TuneScores {             // [N][C] scores and statuses, the plan's statuses, the choice and the series statuses
    DevBuf d_score, d_cst, d_pst, d_best, d_sstat;
};

// The fold panels of the rule's L-BFGS and Newton group, cut once for every candidate that groups the folds alike.
struct FoldPanels {
    bool cut = false;
    OptimiserGroups g;
    CvGroup E_l, E_n;
};

// every candidate cross-validated: shared by all of them the holdout rows and the metric tables; shared by those that
// group the folds alike (tsf_tune: all; tsf_select: by newton_takes under TSF_ALGO_AUTO and by their specified
// changepoints) the fold panel of the rule's L-BFGS and Newton group; per candidate the fits, one
// predict, the metrics and its column of the scores.  S.fit holds rows of the widest candidate's stride; each
// candidate's launches write and its predict reads them at its own (S.stride follows the candidate).
static int tune_score_candidates(tsf_ctx *ctx, CvCall &S, const tsf_spec *cand, int32_t C, int32_t metric,
                                 double rolling_window, TuneScores *B)
{
    const int64_t N = S.N, F = S.F;
    if (F == 0) {                       // no series has a fold: every score NaN, every status the plan's
        const size_t NC = (size_t)N * C;
        std::vector<double> sc(NC, std::nan(""));
        std::vector<int32_t> cs(NC);
        for (size_t i = 0; i < NC; ++i) cs[i] = S.pst[i / C];
        HIP_TRY(ctx, hipMemcpy(B->d_score.p, sc.data(), 8 * NC, hipMemcpyHostToDevice));
        HIP_TRY(ctx, hipMemcpy(B->d_cst.p, cs.data(), 4 * NC, hipMemcpyHostToDevice));
        return 0;
    }
    int64_t grids = 0;                  // (not reported)
    CvHoldout &H = S.hold;
    CvMetrics &X = S.met;
    HIP_TRY(ctx, S.d_yh.alloc(8 * (size_t)F * S.Hmax));
    if (int rc = cv_holdout(ctx, S, nullptr, &H)) return rc;
    if (int rc = cv_metrics_setup(ctx, S, S.d_yh.as<double>(), nullptr, nullptr, rolling_window, &X)) return rc;
    const double *mval = X.d_mm.as<double>() + (size_t)metric * S.M;
    const tsf_fit_out fit = S.fit.view();
    // what the fold panels of a candidate depend on: bit 0, the rule hands its short folds to Newton; bit 1 and the
    // list, its specified changepoints (the table kept per fold, cv_fold_keep, follows from them)
    using PanelKey = std::pair<int, std::vector<int64_t>>;
    auto key_of = [](const tsf_spec &s) {
        PanelKey k(s.algorithm == TSF_ALGO_AUTO && newton_takes(s) ? 1 : 0, {});
        if (s.changepoints_specified == 1 && s.n_changepoints >= 0 && s.n_changepoints <= TSF_MAX_S) {
            k.first |= 2;
            k.second.assign(s.changepoint_ns, s.changepoint_ns + s.n_changepoints);
        }
        return k;
    };
    std::map<PanelKey, FoldPanels> panels;
    std::map<PanelKey, int32_t> users;          // candidates still to come per key: a panel is freed after its last
    for (int32_t c = 0; c < C; ++c) ++users[key_of(cand[c])];
    const double *pfl = S.has_floor ? H.d_ffl.as<double>() : nullptr, *pcap = S.has_cap ? H.d_fcap.as<double>() : nullptr;
    const double *pex = S.n_extra > 0 ? H.d_fex.as<double>() : nullptr;
    for (int32_t c = 0; c < C; ++c) {
        S.stride = tsf_theta_stride(&cand[c]);
        S.f_keep = cv_fold_keep(cand[c], S.f_cut);
        const CvViews folds = cv_fold_views(S);
        const PanelKey key = key_of(cand[c]);
        FoldPanels &P = panels[key];
        if (!P.cut) {
            P.g = optimiser_groups(cand[c], nullptr, (size_t)F, S.f_hist.data());
            if (int rc = cv_expand(ctx, S, folds, P.g.lbfgs, &P.E_l)) return rc;
            if (int rc = cv_expand(ctx, S, folds, P.g.newton, &P.E_n)) return rc;
            ctx->tune_expand += (P.E_l.G > 0) + (P.E_n.G > 0);
            P.cut = true;
        }
        auto fit_group = [&](const tsf_spec &gs, const std::vector<int32_t> &gf, RuleLaunch which) -> int {
            if (which != RULE_RETRY) return cv_fit(ctx, S, which == RULE_LBFGS ? P.E_l : P.E_n, gs, fit, &grids, &ctx->tune_fits);
            CvGroup E_r;
            if (int rc = cv_expand(ctx, S, folds, gf, &E_r)) return rc;
            ctx->tune_expand += 1;
            return cv_fit(ctx, S, E_r, gs, fit, &grids, &ctx->tune_fits);
        };
        if (int rc = fit_by_rule(ctx, cand[c], P.g, S.fit, fit_group)) return rc;
        if (int rc = tsf_predict_dev(ctx, &cand[c], F, S.Hmax, fit.theta, fit.y_scale, fit.grid, (int32_t)F,
                                     H.d_fds.as<int64_t>(), 0, pfl, pcap, pex, S.d_yh.as<double>(), nullptr, nullptr))
            return rc;
        HIP_TRY(ctx, hipMemcpy(X.d_sst.p, S.pst.data(), 4 * (size_t)N, hipMemcpyHostToDevice));
        hipLaunchKernelGGL(cv_metrics_kernel, dim3((unsigned)N), dim3(64), 0, nullptr, X.ma);
        HIP_TRY(ctx, hipGetLastError());
        hipLaunchKernelGGL(tune_score_kernel, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, nullptr, N, C, c, mval,
                           X.d_moff.as<int64_t>(), X.d_sst.as<int32_t>(), B->d_score.as<double>(), B->d_cst.as<int32_t>());
        HIP_TRY(ctx, hipGetLastError());
        if (--users[key] == 0) panels.erase(key);       // (its fit launches are over: cv_fit synchronises)
    }
    return 0;
}

// the choice per series, then scores, statuses and choices to the caller
static int tune_select(tsf_ctx *ctx, int64_t N, int32_t C, const TuneScores &B, const tsf_tune_out &out)
{
    const size_t NC = (size_t)N * C;
    hipLaunchKernelGGL(tune_select_kernel, dim3((unsigned)((N + TUNE_SELECT_WAVES - 1) / TUNE_SELECT_WAVES)),
                       dim3(TUNE_SELECT_WAVES * 64), 0, nullptr, N, C, B.d_score.as<double>(), B.d_pst.as<int32_t>(),
                       B.d_best.as<int32_t>(), B.d_sstat.as<int32_t>());
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, hipDeviceSynchronize());
    HIP_TRY(ctx, hipMemcpy(out.score, B.d_score.p, 8 * NC, hipMemcpyDeviceToHost));
    HIP_TRY(ctx, hipMemcpy(out.cand_status, B.d_cst.p, 4 * NC, hipMemcpyDeviceToHost));
    HIP_TRY(ctx, hipMemcpy(out.best, B.d_best.p, 4 * (size_t)N, hipMemcpyDeviceToHost));
    HIP_TRY(ctx, hipMemcpy(out.series_status, B.d_sstat.p, 4 * (size_t)N, hipMemcpyDeviceToHost));
    return 0;
}

// every series fitted on its whole history with its choice best[n] (base for -1): per choice the rule's launches
static int tune_refit(tsf_ctx *ctx, CvCall &S, const tsf_spec *base, const tsf_spec *cand, int32_t C, const int32_t *best,
                      const tsf_fit_out &out)
{
    const int64_t N = S.N, n_grids = S.aligned ? 1 : N;
    int64_t grids = 0;                  // (not reported)
    DevFitOut refit;
    if (int rc = refit.alloc(ctx, N, S.stride, n_grids, FIT_OUT_UNFITTED)) return rc;
    const tsf_fit_out dst = refit.view();
    WholeViews W;
    if (int rc = W.build(ctx, S)) return rc;
    const CvViews whole = W.views();
    auto fit_group = [&](const tsf_spec &gs, const std::vector<int32_t> &sel, RuleLaunch) -> int {
        return fit_whole_group(ctx, S, whole, gs, sel, dst, &grids, &ctx->tune_fits);
    };
    for (int32_t b = -1; b < C; ++b) {
        const tsf_spec &gs = b < 0 ? *base : cand[b];
        std::vector<int32_t> members;
        for (int64_t n = 0; n < N; ++n)
            if (best[n] == b && W.len[(size_t)n] > 0) members.push_back((int32_t)n);
        const OptimiserGroups g = optimiser_groups(gs, members.data(), members.size(), W.len.data());
        if (int rc = fit_by_rule(ctx, gs, g, refit, fit_group)) return rc;
    }
    HIP_TRY(ctx, hipDeviceSynchronize());
    return refit.download(ctx, out, n_grids);
}

extern "C" int tsf_tune(tsf_ctx *ctx, const tsf_spec *base, const tsf_spec *cand, int32_t C, int64_t N, int32_t T,
                        const int64_t *offsets, const int64_t *ds, const void *y, int32_t y_dtype, const double *floor_,
                        const double *cap, const double *extra, const tsf_cv_args *cv, int32_t metric, int32_t refit,
                        tsf_tune_out *out)
{
    if (!ctx) return -1;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const PanelIn p{N, T, offsets, ds, y, y_dtype, floor_, cap, extra};
    tsf_cv_args a;
    if (int rc = tune_check_args(ctx, base, cand, C, p, cv, metric, refit, out, &a)) return rc;
    ctx->order_n = 0;                   // (pending cost hints were meant for a fit call)
    ctx->tune_expand = 0;
    ctx->tune_fits = 0;
    CvCall S;
    cv_plan_call(p, a, base, &S);
    if (int rc = cv_upload(ctx, nullptr, &S)) return rc;
    const size_t NC = (size_t)N * C;
    TuneScores B;
    HIP_TRY(ctx, B.d_score.alloc(8 * NC)); HIP_TRY(ctx, B.d_cst.alloc(4 * NC));
    HIP_TRY(ctx, B.d_pst.put(S.pst.data(), 4 * (size_t)N));
    HIP_TRY(ctx, B.d_best.alloc(4 * (size_t)N)); HIP_TRY(ctx, B.d_sstat.alloc(4 * (size_t)N));
    if (int rc = tune_score_candidates(ctx, S, cand, C, metric, a.rolling_window, &B)) return rc;
    if (int rc = tune_select(ctx, N, C, B, *out)) return rc;
    return refit ? tune_refit(ctx, S, base, cand, C, out->best, out->fit) : 0;
}

// ---- model-structure selection (include/tsf.h) ----------------------------------------------------------------------
// tsf_tune's steps over candidates of different structure: the plan reads no spec field and is made once;
// tune_score_candidates takes each candidate's theta stride, its table of specified changepoints kept per fold and its
// grouping of the folds; the choice is select_choose_kernel's; the refit fits each choice's series into outputs of that
// candidate's own stride (fit_whole_group, as tsf_tune's refit) and select_scatter_kernel pads them.

extern "C" int tsf_select_out_size(void) { return (int)sizeof(tsf_select_out); }

extern "C" int tsf_select_stride(const tsf_spec *cand, int32_t C)
{
    if (!cand || C < 1) return -1;
    int stride_max = 0;
    for (int32_t c = 0; c < C; ++c) {
        if (cand[c].n_seas < 0 || cand[c].n_seas > TSF_MAX_SEAS) return -1;
        const int s = tsf_theta_stride(&cand[c]);
        if (s > stride_max) stride_max = s;
    }
    return stride_max;
}

// *a = the cross-validation arguments with their defaults filled in and one metric row per series
static int select_check_args(tsf_ctx *ctx, const tsf_spec *cand, int32_t C, const PanelIn &p, const tsf_cv_args *cv,
                             int32_t metric, double tolerance, int32_t fallback, int32_t refit, const tsf_select_out *out,
                             tsf_cv_args *a)
{
    if (!cand || !p.ds || !p.y || !out || !out->score || !out->cand_status || !out->best || !out->chosen || !out->series_status)
        return fail(ctx, "NULL input");
    if (C < 1 || C > TSF_TUNE_MAX_CAND) return fail(ctx, "C must be in [1, TSF_TUNE_MAX_CAND]");
    if (metric < TSF_TUNE_MSE || metric > TSF_TUNE_MAPE) return fail(ctx, "bad metric (TSF_TUNE_MSE .. TSF_TUNE_MAPE)");
    if (refit != 0 && refit != 1) return fail(ctx, "refit must be 0 or 1");
    if (!(std::isfinite(tolerance) && tolerance >= 0.0)) return fail(ctx, "tolerance must be finite and >= 0");
    if (fallback < 0 || fallback >= C) return fail(ctx, "fallback must be in [0, C)");
    if (p.y_dtype < TSF_Y_F64 || p.y_dtype > TSF_Y_I32) return fail(ctx, "bad y_dtype");
    if (!cv) return fail(ctx, "cv is NULL");
    tsf_cv_args cv1 = *cv;
    cv1.rolling_window = 1.0;           // one metric row per series, over all its holdout rows
    if (tsf_cv::resolve_args(&cv1, a)) return fail(ctx, "bad cross-validation arguments (horizon_ns > 0)");
    for (int32_t c = 0; c < C; ++c) {
        DevSpec d;
        int mode;
        if (int rc = build_devspec(ctx, &cand[c], &d, &mode)) return rc;       // (every range a launch would refuse)
        if (cand[c].n_extra != cand[0].n_extra)
            return fail(ctx, "the candidates must agree in n_extra (the call has one extra array)");
        if (!same_optimiser(cand[0], cand[c])) return fail(ctx, "the candidates must agree in every optimiser field");
        if (!prior_scales_ok(cand[c])) return fail(ctx, "a candidate's prior scales must be finite and > 0");
        if (cand[c].growth == TSF_GROWTH_LOGISTIC && !p.cap) return fail(ctx, "logistic growth needs cap");
    }
    if (int rc = check_panel_in(ctx, &cand[0], p)) return rc;
    if (refit && !fit_out_complete(out->fit)) return fail(ctx, "tsf_select_out.fit has NULL members");
    return 0;
}

// the choice per series, then scores, statuses and choices to the caller
static int select_choose(tsf_ctx *ctx, int64_t N, int32_t C, double tolerance, int32_t fallback, const TuneScores &B,
                         const tsf_select_out &out)
{
    const size_t NC = (size_t)N * C;
    DevBuf d_chosen;
    HIP_TRY(ctx, d_chosen.alloc(4 * (size_t)N));
    hipLaunchKernelGGL(select_choose_kernel, dim3((unsigned)((N + TUNE_SELECT_WAVES - 1) / TUNE_SELECT_WAVES)),
                       dim3(TUNE_SELECT_WAVES * 64), 0, nullptr, N, C, tolerance, fallback, B.d_score.as<double>(),
                       B.d_pst.as<int32_t>(), B.d_best.as<int32_t>(), d_chosen.as<int32_t>(), B.d_sstat.as<int32_t>());
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, hipDeviceSynchronize());
    HIP_TRY(ctx, hipMemcpy(out.score, B.d_score.p, 8 * NC, hipMemcpyDeviceToHost));
    HIP_TRY(ctx, hipMemcpy(out.cand_status, B.d_cst.p, 4 * NC, hipMemcpyDeviceToHost));
    HIP_TRY(ctx, hipMemcpy(out.best, B.d_best.p, 4 * (size_t)N, hipMemcpyDeviceToHost));
    HIP_TRY(ctx, hipMemcpy(out.chosen, d_chosen.p, 4 * (size_t)N, hipMemcpyDeviceToHost));
    HIP_TRY(ctx, hipMemcpy(out.series_status, B.d_sstat.p, 4 * (size_t)N, hipMemcpyDeviceToHost));
    return 0;
}

// every series fitted on its whole history with cand[chosen[n]]: per candidate the rule's launches into outputs of its
// own stride, then its members' rows padded into the call's (theta rows of stride_max; aligned: grid[c] the candidate's)
static int select_refit(tsf_ctx *ctx, CvCall &S, const tsf_spec *cand, int32_t C, int stride_max, const int32_t *chosen,
                        const tsf_fit_out &out)
{
    const int64_t N = S.N, n_grids = S.aligned ? C : N;
    int64_t grids = 0;                  // (not reported)
    DevFitOut padded;
    if (int rc = padded.alloc(ctx, N, stride_max, n_grids, FIT_OUT_UNFITTED)) return rc;
    WholeViews W;
    if (int rc = W.build(ctx, S)) return rc;
    const CvViews whole = W.views();
    for (int32_t c = 0; c < C; ++c) {
        const tsf_spec &gs = cand[c];
        std::vector<int32_t> members;
        for (int64_t n = 0; n < N; ++n)
            if (chosen[n] == c && W.len[(size_t)n] > 0) members.push_back((int32_t)n);
        if (members.empty()) continue;
        S.stride = tsf_theta_stride(&gs);
        DevFitOut own;                  // (only the members' rows and the grids of their launches are read)
        if (int rc = own.alloc(ctx, N, S.stride, S.aligned ? 1 : N, FIT_OUT_LAUNCH)) return rc;
        const tsf_fit_out dst = own.view();
        auto fit_group = [&](const tsf_spec &ls, const std::vector<int32_t> &sel, RuleLaunch) -> int {
            return fit_whole_group(ctx, S, whole, ls, sel, dst, &grids, &ctx->tune_fits);
        };
        const OptimiserGroups g = optimiser_groups(gs, members.data(), members.size(), W.len.data());
        if (int rc = fit_by_rule(ctx, gs, g, own, fit_group)) return rc;
        DevBuf d_mem;
        HIP_TRY(ctx, d_mem.put(members.data(), 4 * members.size()));
        hipLaunchKernelGGL(select_scatter_kernel, dim3((unsigned)members.size()), dim3(64), 0, nullptr, (int64_t)members.size(),
                           d_mem.as<int32_t>(), S.stride, stride_max, S.aligned ? c : -1, dst, padded.view());
        HIP_TRY(ctx, hipGetLastError());
        HIP_TRY(ctx, hipDeviceSynchronize());       // (this candidate's buffers go back to the pool)
    }
    HIP_TRY(ctx, hipDeviceSynchronize());
    return padded.download(ctx, out, n_grids);
}

extern "C" int tsf_select(tsf_ctx *ctx, const tsf_spec *cand, int32_t C, int64_t N, int32_t T, const int64_t *offsets,
                          const int64_t *ds, const void *y, int32_t y_dtype, const double *floor_, const double *cap,
                          const double *extra, const tsf_cv_args *cv, int32_t metric, double tolerance, int32_t fallback,
                          int32_t refit, tsf_select_out *out)
{
    if (!ctx) return -1;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const PanelIn p{N, T, offsets, ds, y, y_dtype, floor_, cap, extra};
    tsf_cv_args a;
    if (int rc = select_check_args(ctx, cand, C, p, cv, metric, tolerance, fallback, refit, out, &a)) return rc;
    ctx->order_n = 0;                   // (pending cost hints were meant for a fit call)
    ctx->tune_expand = 0;
    ctx->tune_fits = 0;
    const int stride_max = tsf_select_stride(cand, C);
    CvCall S;
    cv_plan_call(p, a, &cand[0], &S);   // (of the spec: n_extra, every candidate's; the rest is set per candidate)
    S.stride = stride_max;              // (the fold fit outputs, allocated once)
    if (int rc = cv_upload(ctx, nullptr, &S)) return rc;
    const size_t NC = (size_t)N * C;
    TuneScores B;
    HIP_TRY(ctx, B.d_score.alloc(8 * NC)); HIP_TRY(ctx, B.d_cst.alloc(4 * NC));
    HIP_TRY(ctx, B.d_pst.put(S.pst.data(), 4 * (size_t)N));
    HIP_TRY(ctx, B.d_best.alloc(4 * (size_t)N)); HIP_TRY(ctx, B.d_sstat.alloc(4 * (size_t)N));
    if (int rc = tune_score_candidates(ctx, S, cand, C, metric, a.rolling_window, &B)) return rc;
    if (int rc = select_choose(ctx, N, C, tolerance, fallback, B, *out)) return rc;
    return refit ? select_refit(ctx, S, cand, C, stride_max, out->chosen, out->fit) : 0;
}

// ---- outlier screening (include/tsf.h) ----------------------------------------------------------------------
// tsf_screen_rows: the rule, one workgroup per series, one launch per power-of-two class of row counts (the LDS of a
// launch is its class's NSP doubles: a panel of 730-row series does not pay for a 16384-row one).  tsf_fit_screened runs
// tsf_tune's pieces -- the panel once on the device, whole-history fit groups per optimiser -- then per round one
// predict over the history, one screening pass, the flag counts back to the host (the destination offsets of the cut,
// as the cross-validation plan stays on the host), one cut and one fit launch per optimiser group.

extern "C" int tsf_screen_args_size(void) { return (int)sizeof(tsf_screen_args); }
extern "C" int tsf_screen_out_size(void) { return (int)sizeof(tsf_screen_out); }
extern "C" int tsf_fit_screened_out_size(void) { return (int)sizeof(tsf_fit_screened_out); }

static int check_screen_args(tsf_ctx *ctx, const tsf_screen_args *a, const tsf_screen_out *out)
{
    if (!out || !out->flag || !out->status) return fail(ctx, "NULL output (tsf_screen_out, its flag and its status are required)");
    if (!a) return fail(ctx, "NULL tsf_screen_args");
    if (!(a->threshold > 0.0) || !std::isfinite(a->threshold)) return fail(ctx, "threshold must be finite and > 0");
    if (!(a->max_share >= 0.0 && a->max_share <= 0.5)) return fail(ctx, "max_share must be in [0, 0.5]");
    if (a->min_rows < 2) return fail(ctx, "min_rows must be >= 2");
    if (a->max_passes < 1 || a->max_passes > 8) return fail(ctx, "max_passes must be in [1, 8]");
    return 0;
}

// what a screening call needs of its panel's shape: aligned 1 <= T, ragged offsets from 0, ascending; N within int32
static int check_screen_panel(tsf_ctx *ctx, int64_t N, int32_t T, const int64_t *h_off)
{
    if (N > (int64_t)INT32_MAX) return fail(ctx, "N too large");
    if (!h_off) return T >= 1 ? 0 : fail(ctx, "bad panel (aligned: T >= 1)");
    if (h_off[0] != 0) return fail(ctx, "bad panel (ragged: offsets[0] = 0)");
    for (int64_t n = 0; n < N; ++n)
        if (h_off[n + 1] < h_off[n]) return fail(ctx, "bad panel (ragged: offsets ascending)");
    return 0;
}

// The rule on device-resident inputs.  h_off: the ragged panel's offsets on the host (the launch classes), null aligned;
// fit_ld: ScreenArgs::fit_ld; active: the series to screen (host, ascending) or null = all N; o: device pointers.
static int screen_run(tsf_ctx *ctx, int64_t N, int32_t T, const int64_t *d_off, const int64_t *h_off, const void *d_y,
                      int32_t y_dtype, const double *d_fit, int64_t fit_ld, const uint8_t *d_excl, const double *d_ms,
                      const tsf_screen_args &a, const tsf_screen_out &o, const int32_t *active, int64_t n_active,
                      hipStream_t st)
{
    ScreenArgs k;
    memset(&k, 0, sizeof(k));
    k.y = d_y; k.fitted = d_fit; k.excluded = d_excl; k.min_scale = d_ms; k.offsets = h_off ? d_off : nullptr;
    k.T = T; k.fit_ld = fit_ld; k.y_dtype = y_dtype; k.min_rows = a.min_rows; k.threshold = a.threshold; k.max_share = a.max_share;
    k.flag = o.flag; k.resid = o.resid; k.center = o.center; k.scale = o.scale; k.n_new = o.n_new; k.n_flagged = o.n_flagged;
    k.status = o.status;
    // class c: NSP = 2^c rows of LDS; a series beyond TSF_SCREEN_MAX_ROWS only reports its status (class 1)
    auto class_of = [](int64_t len) {
        if (len > (int64_t)TSF_SCREEN_MAX_ROWS) return 1;
        int c = 1;
        while (((int64_t)1 << c) < len) ++c;
        return c;
    };
    auto launch = [&](const int32_t *d_sel, int64_t blocks, int c) -> int {
        const int NSP = 1 << c;
        k.sel = d_sel;
        const size_t lds = sizeof(double) * (size_t)NSP + SCREEN_PART_BYTES;
        // beyond the 64 KiB a kernel gets unasked (series of more than 8184 rows); per launch: the attribute is per
        // device, and a process may drive several GPUs
        if (lds > 64 * 1024)
            HIP_TRY(ctx, hipFuncSetAttribute((const void *)screen_rows_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
        hipLaunchKernelGGL(screen_rows_kernel, dim3((unsigned)blocks), dim3(256), lds, st, k, NSP);
        HIP_TRY(ctx, hipGetLastError());
        return 0;
    };
    if (!active) n_active = N;
    if (n_active == 0) return 0;
    if (!h_off && !active) return launch(nullptr, N, class_of(T));
    constexpr int NC = 16;
    int64_t count[NC] = {0}, start[NC + 1] = {0};
    std::vector<int8_t> cls((size_t)n_active);
    for (int64_t i = 0; i < n_active; ++i) {
        const int64_t n = active ? active[i] : i;
        cls[(size_t)i] = (int8_t)class_of(h_off ? h_off[n + 1] - h_off[n] : (int64_t)T);
        count[cls[(size_t)i]]++;
    }
    for (int c = 0; c < NC; ++c) start[c + 1] = start[c] + count[c];
    if (!active)
        for (int c = 0; c < NC; ++c)
            if (count[c] == N) return launch(nullptr, N, c);        // one class: no list
    std::vector<int32_t> sel((size_t)n_active);
    {
        int64_t at[NC];
        for (int c = 0; c < NC; ++c) at[c] = start[c];
        for (int64_t i = 0; i < n_active; ++i) sel[(size_t)at[cls[(size_t)i]]++] = (int32_t)(active ? active[i] : i);
    }
    DevBuf d_sel;
    HIP_TRY(ctx, d_sel.alloc(4 * (size_t)n_active));
    HIP_TRY(ctx, hipMemcpy(d_sel.p, sel.data(), 4 * (size_t)n_active, hipMemcpyHostToDevice));
    for (int c = 0; c < NC; ++c)
        if (count[c] > 0)
            if (int rc = launch(d_sel.as<int32_t>() + start[c], count[c], c)) return rc;
    HIP_TRY(ctx, hipStreamSynchronize(st));         // (the list goes back to the pool)
    return 0;
}

extern "C" int tsf_screen_rows_dev(tsf_ctx *ctx, int64_t N, int32_t T, const int64_t *offsets, const void *y, int32_t y_dtype,
                                   const double *fitted, const uint8_t *excluded, const double *min_scale,
                                   const tsf_screen_args *args, tsf_screen_out *out, void *stream)
{
    if (!ctx) return -1;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (N < 0) return fail(ctx, "N must be >= 0");
    if (int rc = check_screen_args(ctx, args, out)) return rc;
    if (!y || !fitted) return fail(ctx, "NULL input (y and fitted are required)");
    if (y_dtype < TSF_Y_F64 || y_dtype > TSF_Y_I32) return fail(ctx, "bad y_dtype");
    if (N == 0) return 0;
    hipStream_t st = (hipStream_t)stream;
    std::vector<int64_t> h_off;
    if (offsets) {
        h_off.resize((size_t)N + 1);
        HIP_TRY(ctx, hipStreamSynchronize(st));
        HIP_TRY(ctx, hipMemcpy(h_off.data(), offsets, 8 * ((size_t)N + 1), hipMemcpyDeviceToHost));
    }
    if (int rc = check_screen_panel(ctx, N, T, offsets ? h_off.data() : nullptr)) return rc;
    return screen_run(ctx, N, T, offsets, offsets ? h_off.data() : nullptr, y, y_dtype, fitted, 0, excluded, min_scale, *args,
                      *out, nullptr, 0, st);
}

extern "C" int tsf_screen_rows(tsf_ctx *ctx, int64_t N, int32_t T, const int64_t *offsets, const void *y, int32_t y_dtype,
                               const double *fitted, const uint8_t *excluded, const double *min_scale,
                               const tsf_screen_args *args, tsf_screen_out *out)
{
    if (!ctx) return -1;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (N < 0) return fail(ctx, "N must be >= 0");
    if (int rc = check_screen_args(ctx, args, out)) return rc;
    if (!y || !fitted) return fail(ctx, "NULL input (y and fitted are required)");
    if (y_dtype < TSF_Y_F64 || y_dtype > TSF_Y_I32) return fail(ctx, "bad y_dtype");
    if (N == 0) return 0;
    if (int rc = check_screen_panel(ctx, N, T, offsets)) return rc;
    const size_t rows = offsets ? (size_t)offsets[N] : (size_t)N * T, ysz = ysize(y_dtype);
    DevBuf d_off, d_y, d_fit, d_ex, d_ms;
    HostOuts outs;
    if (offsets) HIP_TRY(ctx, d_off.put(offsets, 8 * ((size_t)N + 1)));
    HIP_TRY(ctx, d_y.put(y, ysz * rows));
    HIP_TRY(ctx, d_fit.put(fitted, 8 * rows));
    if (excluded) HIP_TRY(ctx, d_ex.put(excluded, rows));
    if (min_scale) HIP_TRY(ctx, d_ms.put(min_scale, 8 * (size_t)N));
    tsf_screen_out o;
    memset(&o, 0, sizeof(o));
    o.flag = outs.want(out->flag, rows); o.status = outs.want(out->status, 4 * (size_t)N);
    o.resid = outs.want(out->resid, 8 * rows);
    o.center = outs.want(out->center, 8 * (size_t)N); o.scale = outs.want(out->scale, 8 * (size_t)N);
    o.n_new = outs.want(out->n_new, 4 * (size_t)N); o.n_flagged = outs.want(out->n_flagged, 4 * (size_t)N);
    if (int rc = outs.ready(ctx)) return rc;
    if (int rc = screen_run(ctx, N, T, d_off.as<int64_t>(), offsets, d_y.p, y_dtype, d_fit.as<double>(), 0,
                            d_ex.as<uint8_t>(), d_ms.as<double>(), *args, o, nullptr, 0, nullptr))
        return rc;
    HIP_TRY(ctx, hipDeviceSynchronize());
    return outs.fetch(ctx);
}

// ---- the steps of tsf_fit_screened ------------------------------------------------------------------------------

static int screened_check_args(tsf_ctx *ctx, const tsf_spec *spec, const PanelIn &p, double scale_floor_rel,
                               const tsf_screen_args *args, const tsf_fit_screened_out *out)
{
    if (!spec || !p.ds || !p.y || !out) return fail(ctx, "NULL input");
    if (int rc = check_screen_args(ctx, args, &out->screen)) return rc;
    if (p.y_dtype < TSF_Y_F64 || p.y_dtype > TSF_Y_I32) return fail(ctx, "bad y_dtype");
    if (int rc = check_panel_in(ctx, spec, p, INT32_MAX)) return rc;
    if (!(scale_floor_rel >= 0.0) || !std::isfinite(scale_floor_rel)) return fail(ctx, "scale_floor_rel must be finite and >= 0");
    if (!fit_out_complete(out->fit)) return fail(ctx, "tsf_fit_screened_out.fit has NULL members");
    if (out->first && !fit_out_complete(*out->first)) return fail(ctx, "tsf_fit_screened_out.first has NULL members");
    return check_algorithm(ctx, spec);
}

// What the rounds of a tsf_fit_screened call work on: the panel, the current fit of every series (a grid per series
// from the first round on), the history as a future panel, the screening outputs and the host's counts.
struct ScreenedRun {
    CvCall S;
    DevFitOut fit;
    WholeViews W;
    int64_t grids = 0;                  // (not reported)
    int32_t launches = 0;
    int32_t H = 0;                      // columns of the history panel: T, or the longest series' rows
    DevBuf d_hds, d_hex, d_fit, d_ms, d_flag, d_res, d_cen, d_sc, d_nn, d_nf, d_sst;
    tsf_screen_out so;
    std::vector<int32_t> h_new, h_flagged, rounds, active;
    std::vector<int64_t> kept;          // rows without a flag, of the series cut so far
};

// round 0: every series with rows fitted on its whole history by the optimiser rule, as tsf_tune's refit fits base;
// *first (where asked for) receives it, then the one grid of an aligned panel is spread to a grid per series
static int screened_first_fit(tsf_ctx *ctx, ScreenedRun &R, const tsf_spec *spec, const tsf_fit_out *first)
{
    CvCall &S = R.S;
    const int64_t N = S.N;
    if (int rc = R.fit.alloc(ctx, N, S.stride, N, FIT_OUT_UNFITTED)) return rc;
    if (int rc = R.W.build(ctx, S)) return rc;
    const tsf_fit_out dst = R.fit.view();
    const CvViews whole = R.W.views();
    std::vector<int32_t> members;
    for (int64_t n = 0; n < N; ++n) if (R.W.len[(size_t)n] > 0) members.push_back((int32_t)n);
    if (int rc = fit_by_rule(ctx, *spec, optimiser_groups(*spec, members.data(), members.size(), R.W.len.data()), R.fit,
                             [&](const tsf_spec &gs, const std::vector<int32_t> &sel, RuleLaunch) -> int {
                                 return fit_whole_group(ctx, S, whole, gs, sel, dst, &R.grids, &R.launches);
                             }))
        return rc;
    HIP_TRY(ctx, hipDeviceSynchronize());
    if (first)
        if (int rc = R.fit.download(ctx, *first, S.aligned ? 1 : N)) return rc;
    if (S.aligned && N > 1) {
        const int64_t words = (N - 1) * (int64_t)(sizeof(tsf_grid_info) / 8);
        hipLaunchKernelGGL(screen_grid_fill_kernel, dim3((unsigned)((words + 255) / 256)), dim3(256), 0, nullptr, N, dst.grid);
        HIP_TRY(ctx, hipGetLastError());
    }
    return 0;
}

// the buffers of the rounds: the history as a future panel (ragged: padded to H columns), the fitted values, the flags
// (none yet) and the screening outputs the caller asked for
static int screened_rounds_setup(tsf_ctx *ctx, ScreenedRun &R, const tsf_screen_out &want)
{
    CvCall &S = R.S;
    const int64_t N = S.N;
    const int32_t H = R.H = S.aligned ? S.T : (int32_t)R.W.max_len;
    const size_t rows = S.aligned ? (size_t)N * S.T : (size_t)S.offsets[N];
    if (!S.aligned) {
        HIP_TRY(ctx, R.d_hds.alloc(8 * (size_t)N * H));
        if (S.n_extra > 0) HIP_TRY(ctx, R.d_hex.alloc(8 * (size_t)N * S.n_extra * H));
        hipLaunchKernelGGL(screen_history_kernel, dim3((unsigned)(N < 65535 ? N : 65535)), dim3(256), 0, nullptr, S.pn, N, H,
                           R.d_hds.as<int64_t>(), S.n_extra > 0 ? R.d_hex.as<double>() : nullptr);
        HIP_TRY(ctx, hipGetLastError());
    }
    HIP_TRY(ctx, R.d_fit.alloc(8 * (size_t)N * H)); HIP_TRY(ctx, R.d_ms.alloc(8 * (size_t)N));
    HIP_TRY(ctx, R.d_flag.alloc(rows)); HIP_TRY(ctx, hipMemset(R.d_flag.p, 0, rows ? rows : 1));
    HIP_TRY(ctx, R.d_nn.alloc(4 * (size_t)N)); HIP_TRY(ctx, R.d_nf.alloc(4 * (size_t)N)); HIP_TRY(ctx, R.d_sst.alloc(4 * (size_t)N));
    tsf_screen_out &so = R.so;
    memset(&so, 0, sizeof(so));
    so.flag = R.d_flag.as<uint8_t>(); so.n_new = R.d_nn.as<int32_t>(); so.n_flagged = R.d_nf.as<int32_t>();
    so.status = R.d_sst.as<int32_t>();
    if (want.resid) { HIP_TRY(ctx, R.d_res.alloc(8 * rows)); so.resid = R.d_res.as<double>(); }
    if (want.center) { HIP_TRY(ctx, R.d_cen.alloc(8 * (size_t)N)); so.center = R.d_cen.as<double>(); }
    if (want.scale) { HIP_TRY(ctx, R.d_sc.alloc(8 * (size_t)N)); so.scale = R.d_sc.as<double>(); }
    R.h_new.resize((size_t)N); R.h_flagged.resize((size_t)N); R.rounds.assign((size_t)N, 0); R.kept.resize((size_t)N);
    return 0;
}

// the rows without a flag of the series sel as one ragged panel, fitted with gs, the results at the series' positions
static int screened_refit_cut(tsf_ctx *ctx, ScreenedRun &R, const tsf_spec &gs, const std::vector<int32_t> &sel)
{
    CvCall &S = R.S;
    CvGroup E;
    if (int rc = cv_group_layout(ctx, S, sel, R.kept.data(), &E)) return rc;
    const int64_t G = E.G;
    hipLaunchKernelGGL(screen_compact_kernel, dim3((unsigned)(G < 65535 ? G : 65535)), dim3(256), 0, nullptr, S.pn, G,
                       E.d_gf.as<int32_t>(), R.d_flag.as<uint8_t>(), E.d_goff.as<int64_t>(), E.rows,
                       S.has_floor ? S.d_fl.as<double>() : nullptr, S.has_cap ? S.d_cap.as<double>() : nullptr,
                       E.d_gds.as<int64_t>(), E.d_gy.p, S.n_extra > 0 ? E.d_gex.as<double>() : nullptr,
                       S.has_floor ? E.d_gfl.as<double>() : nullptr, S.has_cap ? E.d_gcap.as<double>() : nullptr);
    HIP_TRY(ctx, hipGetLastError());
    return cv_fit(ctx, S, E, gs, R.fit.view(), &R.grids, &R.launches);
}

// round p >= 1: predict over the history, the screening rule on the series still active, the flag counts back, and the
// series with new flags cut and fitted again by the optimiser rule on the rows they keep.  *done: no series was cut.
static int screened_round(tsf_ctx *ctx, ScreenedRun &R, const tsf_spec *spec, double scale_floor_rel,
                          const tsf_screen_args &args, int32_t p, bool *done)
{
    CvCall &S = R.S;
    const int64_t N = S.N;
    const int32_t H = R.H;
    const bool aligned = S.aligned;
    const tsf_fit_out fit = R.fit.view();
    if (int rc = tsf_predict_dev(ctx, spec, N, H, fit.theta, fit.y_scale, fit.grid, (int32_t)N,
                                 aligned ? S.d_ds.as<int64_t>() : R.d_hds.as<int64_t>(), aligned ? 1 : 0,
                                 S.has_floor ? S.d_fl.as<double>() : nullptr, S.has_cap ? S.d_cap.as<double>() : nullptr,
                                 S.n_extra > 0 ? (aligned ? S.d_ex.as<double>() : R.d_hex.as<double>()) : nullptr,
                                 R.d_fit.as<double>(), nullptr, nullptr))
        return rc;
    hipLaunchKernelGGL(screen_mask_failed_kernel, dim3((unsigned)(N < 65535 ? N : 65535)), dim3(256), 0, nullptr, N,
                       (int64_t)H, fit.status, R.d_fit.as<double>());
    HIP_TRY(ctx, hipGetLastError());
    hipLaunchKernelGGL(screen_scale_floor_kernel, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, nullptr, N,
                       scale_floor_rel, fit.y_scale, R.d_ms.as<double>());
    HIP_TRY(ctx, hipGetLastError());
    // (excluded and flag are one array: a thread reads a row's byte before it writes it, and no other thread does)
    if (int rc = screen_run(ctx, N, S.T, S.d_off.as<int64_t>(), S.offsets, S.d_y.p, S.y_dtype, R.d_fit.as<double>(), H,
                            R.d_flag.as<uint8_t>(), R.d_ms.as<double>(), args, R.so, p == 1 ? nullptr : R.active.data(),
                            (int64_t)R.active.size(), nullptr))
        return rc;
    HIP_TRY(ctx, hipMemcpy(R.h_new.data(), R.d_nn.p, 4 * (size_t)N, hipMemcpyDeviceToHost));
    HIP_TRY(ctx, hipMemcpy(R.h_flagged.data(), R.d_nf.p, 4 * (size_t)N, hipMemcpyDeviceToHost));
    std::vector<int32_t> cutl;
    for (int64_t i = 0; i < (p == 1 ? N : (int64_t)R.active.size()); ++i) {
        const int32_t n = p == 1 ? (int32_t)i : R.active[(size_t)i];
        if (R.h_new[(size_t)n] <= 0) continue;
        cutl.push_back(n);
        R.rounds[(size_t)n] += 1;
        R.kept[(size_t)n] = R.W.len[(size_t)n] - R.h_flagged[(size_t)n];
    }
    *done = cutl.empty();
    if (*done) return 0;
    if (int rc = fit_by_rule(ctx, *spec, optimiser_groups(*spec, cutl.data(), cutl.size(), R.kept.data()), R.fit,
                             [&](const tsf_spec &gs, const std::vector<int32_t> &sel, RuleLaunch) -> int {
                                 return screened_refit_cut(ctx, R, gs, sel);
                             }))
        return rc;
    R.active.swap(cutl);
    return 0;
}

// the last fit of every series, the screening outputs and the rounds to the caller
static int screened_download(tsf_ctx *ctx, const ScreenedRun &R, const tsf_fit_screened_out &out)
{
    const CvCall &S = R.S;
    const size_t N = (size_t)S.N, rows = S.aligned ? N * S.T : (size_t)S.offsets[N];
    if (int rc = R.fit.download(ctx, out.fit, S.N)) return rc;
    const tsf_screen_out &ho = out.screen;
    if (rows) HIP_TRY(ctx, hipMemcpy(ho.flag, R.d_flag.p, rows, hipMemcpyDeviceToHost));
    HIP_TRY(ctx, hipMemcpy(ho.status, R.d_sst.p, 4 * N, hipMemcpyDeviceToHost));
    if (ho.resid && rows) HIP_TRY(ctx, hipMemcpy(ho.resid, R.d_res.p, 8 * rows, hipMemcpyDeviceToHost));
    if (ho.center) HIP_TRY(ctx, hipMemcpy(ho.center, R.d_cen.p, 8 * N, hipMemcpyDeviceToHost));
    if (ho.scale) HIP_TRY(ctx, hipMemcpy(ho.scale, R.d_sc.p, 8 * N, hipMemcpyDeviceToHost));
    if (ho.n_new) HIP_TRY(ctx, hipMemcpy(ho.n_new, R.d_nn.p, 4 * N, hipMemcpyDeviceToHost));
    if (ho.n_flagged) HIP_TRY(ctx, hipMemcpy(ho.n_flagged, R.d_nf.p, 4 * N, hipMemcpyDeviceToHost));
    if (out.rounds) memcpy(out.rounds, R.rounds.data(), 4 * N);
    return 0;
}

extern "C" int tsf_fit_screened(tsf_ctx *ctx, const tsf_spec *spec, int64_t N, int32_t T, const int64_t *offsets,
                                const int64_t *ds, const void *y, int32_t y_dtype, const double *floor_, const double *cap,
                                const double *extra, double scale_floor_rel, const tsf_screen_args *args,
                                tsf_fit_screened_out *out)
{
    if (!ctx) return -1;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const PanelIn p{N, T, offsets, ds, y, y_dtype, floor_, cap, extra};
    if (int rc = screened_check_args(ctx, spec, p, scale_floor_rel, args, out)) return rc;
    ctx->order_n = 0;                   // (pending cost hints were meant for a fit call)
    if (offsets && offsets[N] == 0) return fail(ctx, "no rows");
    ScreenedRun R;
    cv_call_shape(p, spec, &R.S);
    if (int rc = cv_upload(ctx, nullptr, &R.S)) return rc;
    if (int rc = screened_first_fit(ctx, R, spec, out->first)) return rc;
    if (int rc = screened_rounds_setup(ctx, R, out->screen)) return rc;
    bool done = false;
    for (int32_t p = 1; p <= args->max_passes && !done; ++p)
        if (int rc = screened_round(ctx, R, spec, scale_floor_rel, *args, p, &done)) return rc;
    HIP_TRY(ctx, hipDeviceSynchronize());
    return screened_download(ctx, R, *out);
}

// ---- conformal interval calibration (include/tsf.h) ---------------------------------------------------------
// tsf_calibrate_rows: the rule, one workgroup per series, one launch per power-of-two class of row counts, as the
// screening rule is launched (the LDS of a launch is its class's: calib_lds_bytes).  tsf_apply_calibration: one
// elementwise launch.  tsf_calibrate is cross_validate_run with the rule behind its metrics.

extern "C" int tsf_calib_args_size(void) { return (int)sizeof(tsf_calib_args); }
extern "C" int tsf_calib_table_size(void) { return (int)sizeof(tsf_calib_table); }

static int check_calib_args(tsf_ctx *ctx, const tsf_calib_args *a)
{
    if (!a) return fail(ctx, "NULL tsf_calib_args");
    if (a->mode != TSF_CALIB_ABS && a->mode != TSF_CALIB_CQR) return fail(ctx, "mode must be TSF_CALIB_ABS or TSF_CALIB_CQR");
    if (a->n_levels < 1 || a->n_levels > TSF_CALIB_MAX_LEVELS) return fail(ctx, "n_levels must be in [1, TSF_CALIB_MAX_LEVELS]");
    for (int l = 0; l < a->n_levels; ++l)
        if (!(a->levels[l] > 0.0 && a->levels[l] < 1.0)) return fail(ctx, "every level must be strictly inside (0, 1)");
    if (a->horizon_ns <= 0) return fail(ctx, "horizon_ns must be > 0");
    if (a->n_buckets < 1 || a->n_buckets > TSF_CALIB_MAX_BUCKETS) return fail(ctx, "n_buckets must be in [1, TSF_CALIB_MAX_BUCKETS]");
    if (a->min_scores < 1) return fail(ctx, "min_scores must be >= 1");
    return 0;
}

static int check_calib_table(tsf_ctx *ctx, const tsf_calib_table *t)
{
    if (!t || !t->q || !t->n || !t->status) return fail(ctx, "NULL output (tsf_calib_table, its q, n and status are required)");
    return 0;
}

static int check_calib_rows(tsf_ctx *ctx, int64_t N, const int64_t *h_off)
{
    if (N > (int64_t)INT32_MAX) return fail(ctx, "N too large");
    if (h_off[0] != 0) return fail(ctx, "bad rows (row_off[0] = 0)");
    for (int64_t n = 0; n < N; ++n)
        if (h_off[n + 1] < h_off[n]) return fail(ctx, "bad rows (row_off ascending)");
    return 0;
}

// the table of a call without a single holdout row (host)
static int calib_no_table(const tsf_calib_args &a, int64_t N, const tsf_calib_table &t)
{
    const size_t cells = (size_t)(a.n_buckets + 1) * a.n_levels;
    for (size_t i = 0; i < (size_t)N * cells; ++i) { t.q[i] = std::numeric_limits<double>::quiet_NaN(); t.n[i] = 0; }
    for (int64_t n = 0; n < N; ++n) t.status[n] = TSF_CALIB_NO_SCORES;
    return 0;
}

// The rule on device-resident rows.  h_off: row_off on the host (the launch classes); o: device pointers.
static int calib_run(tsf_ctx *ctx, int64_t N, const int64_t *d_off, const int64_t *h_off, const int64_t *d_h, const double *d_y,
                     const double *d_yhat, const double *d_lower, const double *d_upper, const tsf_calib_args &a,
                     const tsf_calib_table &o, hipStream_t st)
{
    if (N == 0) return 0;
    CalibRowsArgs k;
    memset(&k, 0, sizeof(k));
    k.row_off = d_off; k.h = d_h; k.y = d_y; k.yhat = d_yhat;
    k.lower = a.mode == TSF_CALIB_CQR ? d_lower : nullptr; k.upper = a.mode == TSF_CALIB_CQR ? d_upper : nullptr;
    k.R = h_off[N]; k.horizon = a.horizon_ns; k.w = (a.horizon_ns + a.n_buckets - 1) / a.n_buckets;
    k.mode = a.mode; k.L = a.n_levels; k.B = a.n_buckets; k.min_scores = a.min_scores;
    for (int l = 0; l < a.n_levels; ++l) k.levels[l] = a.levels[l];
    k.q = o.q; k.n = o.n; k.status = o.status;
    // class c: NSP = 2^c rows of LDS; a series beyond TSF_CALIB_MAX_ROWS only reports its status (class 1)
    auto class_of = [](int64_t len) {
        if (len > (int64_t)TSF_CALIB_MAX_ROWS) return 1;
        int c = 1;
        while (((int64_t)1 << c) < len) ++c;
        return c;
    };
    auto launch = [&](const int32_t *d_sel, int64_t blocks, int c) -> int {
        const int NSP = 1 << c;
        k.sel = d_sel;
        const size_t lds = calib_lds_bytes(NSP);
        if (lds > 64 * 1024)        // (per launch: the attribute is per device, and a process may drive several GPUs)
            HIP_TRY(ctx, hipFuncSetAttribute((const void *)calib_rows_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
        hipLaunchKernelGGL(calib_rows_kernel, dim3((unsigned)blocks), dim3(256), lds, st, k, NSP);
        HIP_TRY(ctx, hipGetLastError());
        return 0;
    };
    constexpr int NC = 16;
    int64_t count[NC] = {0}, start[NC + 1] = {0};
    std::vector<int8_t> cls((size_t)N);
    for (int64_t n = 0; n < N; ++n) {
        cls[(size_t)n] = (int8_t)class_of(h_off[n + 1] - h_off[n]);
        count[cls[(size_t)n]]++;
    }
    for (int c = 0; c < NC; ++c) start[c + 1] = start[c] + count[c];
    for (int c = 0; c < NC; ++c)
        if (count[c] == N) return launch(nullptr, N, c);        // one class: no list
    std::vector<int32_t> sel((size_t)N);
    {
        int64_t at[NC];
        for (int c = 0; c < NC; ++c) at[c] = start[c];
        for (int64_t n = 0; n < N; ++n) sel[(size_t)at[cls[(size_t)n]]++] = (int32_t)n;
    }
    DevBuf d_sel;
    HIP_TRY(ctx, d_sel.alloc(4 * (size_t)N));
    HIP_TRY(ctx, hipMemcpy(d_sel.p, sel.data(), 4 * (size_t)N, hipMemcpyHostToDevice));
    for (int c = 0; c < NC; ++c)
        if (count[c] > 0)
            if (int rc = launch(d_sel.as<int32_t>() + start[c], count[c], c)) return rc;
    HIP_TRY(ctx, hipStreamSynchronize(st));         // (the list goes back to the pool)
    return 0;
}

static int check_calib_rows_call(tsf_ctx *ctx, int64_t N, const int64_t *row_off, const int64_t *h, const double *y,
                                 const double *yhat, const double *lower, const double *upper, const tsf_calib_args *args,
                                 const tsf_calib_table *table)
{
    if (N < 0) return fail(ctx, "N must be >= 0");
    if (int rc = check_calib_args(ctx, args)) return rc;
    if (int rc = check_calib_table(ctx, table)) return rc;
    if (!row_off || !h || !y || !yhat) return fail(ctx, "NULL input (row_off, horizon_ns, y and yhat are required)");
    if (args->mode == TSF_CALIB_CQR && (!lower || !upper)) return fail(ctx, "TSF_CALIB_CQR needs lower and upper");
    return 0;
}

extern "C" int tsf_calibrate_rows_dev(tsf_ctx *ctx, int64_t N, const int64_t *row_off, const int64_t *horizon_ns,
                                      const double *y, const double *yhat, const double *lower, const double *upper,
                                      const tsf_calib_args *args, tsf_calib_table *table, void *stream)
{
    if (!ctx) return -1;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (int rc = check_calib_rows_call(ctx, N, row_off, horizon_ns, y, yhat, lower, upper, args, table)) return rc;
    if (N == 0) return 0;
    hipStream_t st = (hipStream_t)stream;
    std::vector<int64_t> h_off((size_t)N + 1);
    HIP_TRY(ctx, hipStreamSynchronize(st));
    HIP_TRY(ctx, hipMemcpy(h_off.data(), row_off, 8 * ((size_t)N + 1), hipMemcpyDeviceToHost));
    if (int rc = check_calib_rows(ctx, N, h_off.data())) return rc;
    return calib_run(ctx, N, row_off, h_off.data(), horizon_ns, y, yhat, lower, upper, *args, *table, st);
}

extern "C" int tsf_calibrate_rows(tsf_ctx *ctx, int64_t N, const int64_t *row_off, const int64_t *horizon_ns, const double *y,
                                  const double *yhat, const double *lower, const double *upper, const tsf_calib_args *args,
                                  tsf_calib_table *table)
{
    if (!ctx) return -1;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (int rc = check_calib_rows_call(ctx, N, row_off, horizon_ns, y, yhat, lower, upper, args, table)) return rc;
    if (N == 0) return 0;
    if (int rc = check_calib_rows(ctx, N, row_off)) return rc;
    const size_t R = (size_t)row_off[N], L = (size_t)args->n_levels, cells = (size_t)(args->n_buckets + 1) * L;
    const bool cqr = args->mode == TSF_CALIB_CQR;
    DevBuf d_off, d_h, d_y, d_yh, d_lo, d_hi;
    HostOuts outs;
    HIP_TRY(ctx, d_off.put(row_off, 8 * ((size_t)N + 1)));
    HIP_TRY(ctx, d_h.put(horizon_ns, 8 * R)); HIP_TRY(ctx, d_y.put(y, 8 * R)); HIP_TRY(ctx, d_yh.put(yhat, 8 * R));
    if (cqr) { HIP_TRY(ctx, d_lo.put(lower, 8 * L * R)); HIP_TRY(ctx, d_hi.put(upper, 8 * L * R)); }
    const tsf_calib_table dt{outs.want(table->q, 8 * (size_t)N * cells), outs.want(table->n, 4 * (size_t)N * cells),
                             outs.want(table->status, 4 * (size_t)N)};
    if (int rc = outs.ready(ctx)) return rc;
    if (int rc = calib_run(ctx, N, d_off.as<int64_t>(), row_off, d_h.as<int64_t>(), d_y.as<double>(), d_yh.as<double>(),
                           d_lo.as<double>(), d_hi.as<double>(), *args, dt, nullptr))
        return rc;
    HIP_TRY(ctx, hipDeviceSynchronize());
    return outs.fetch(ctx);
}

static int check_calib_apply_call(tsf_ctx *ctx, int64_t N, int32_t H, const double *yhat, const double *lower,
                                  const double *upper, const int64_t *ds_future, const int64_t *origin_ns, const double *q,
                                  const int32_t *n, const tsf_calib_args *args, const double *lo, const double *hi)
{
    if (N < 0 || H < 0) return fail(ctx, "N and H must be >= 0");
    if (int rc = check_calib_args(ctx, args)) return rc;
    if (!yhat || !ds_future || !origin_ns || !q || !n || !lo || !hi)
        return fail(ctx, "NULL input (yhat, ds_future, origin_ns, q, n, lo and hi are required)");
    if (args->mode == TSF_CALIB_CQR && (!lower || !upper)) return fail(ctx, "TSF_CALIB_CQR needs lower and upper");
    return 0;
}

static int calib_apply_run(tsf_ctx *ctx, int64_t N, int32_t H, const double *yhat, const double *lower, const double *upper,
                           const int64_t *ds_future, int32_t shared_future, const int64_t *origin_ns, const double *q,
                           const int32_t *n, const tsf_calib_args &a, double *lo, double *hi, int8_t *cell, hipStream_t st)
{
    CalibApplyArgs k;
    memset(&k, 0, sizeof(k));
    k.N = N; k.H = H; k.L = a.n_levels; k.B = a.n_buckets; k.mode = a.mode; k.min_scores = a.min_scores;
    k.shared_future = shared_future ? 1 : 0; k.w = (a.horizon_ns + a.n_buckets - 1) / a.n_buckets;
    k.yhat = yhat; k.lower = a.mode == TSF_CALIB_CQR ? lower : nullptr; k.upper = a.mode == TSF_CALIB_CQR ? upper : nullptr;
    k.ds_future = ds_future; k.origin = origin_ns; k.q = q; k.n = n; k.lo = lo; k.hi = hi; k.cell = cell;
    const int64_t total = N * (int64_t)a.n_levels * H, blocks = (total + 255) / 256;
    hipLaunchKernelGGL(calib_apply_kernel, dim3((unsigned)(blocks < 65535 ? blocks : 65535)), dim3(256), 0, st, k);
    HIP_TRY(ctx, hipGetLastError());
    return 0;
}

extern "C" int tsf_apply_calibration_dev(tsf_ctx *ctx, int64_t N, int32_t H, const double *yhat, const double *lower,
                                         const double *upper, const int64_t *ds_future, int32_t shared_future,
                                         const int64_t *origin_ns, const double *q, const int32_t *n,
                                         const tsf_calib_args *args, double *lo, double *hi, int8_t *cell, void *stream)
{
    if (!ctx) return -1;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (int rc = check_calib_apply_call(ctx, N, H, yhat, lower, upper, ds_future, origin_ns, q, n, args, lo, hi)) return rc;
    if (N == 0 || H == 0) return 0;
    return calib_apply_run(ctx, N, H, yhat, lower, upper, ds_future, shared_future, origin_ns, q, n, *args, lo, hi, cell,
                           (hipStream_t)stream);
}

extern "C" int tsf_apply_calibration(tsf_ctx *ctx, int64_t N, int32_t H, const double *yhat, const double *lower,
                                     const double *upper, const int64_t *ds_future, int32_t shared_future,
                                     const int64_t *origin_ns, const double *q, const int32_t *n, const tsf_calib_args *args,
                                     double *lo, double *hi, int8_t *cell)
{
    if (!ctx) return -1;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (int rc = check_calib_apply_call(ctx, N, H, yhat, lower, upper, ds_future, origin_ns, q, n, args, lo, hi)) return rc;
    if (N == 0 || H == 0) return 0;
    const size_t NH = (size_t)N * H, L = (size_t)args->n_levels, cells = (size_t)(args->n_buckets + 1) * L;
    const size_t n_ds = shared_future ? (size_t)H : NH;
    const bool cqr = args->mode == TSF_CALIB_CQR;
    DevBuf d_yh, d_lw, d_up, d_ds, d_or, d_q, d_n;
    HostOuts outs;
    HIP_TRY(ctx, d_yh.put(yhat, 8 * NH));
    if (cqr) { HIP_TRY(ctx, d_lw.put(lower, 8 * L * NH)); HIP_TRY(ctx, d_up.put(upper, 8 * L * NH)); }
    HIP_TRY(ctx, d_ds.put(ds_future, 8 * n_ds));
    HIP_TRY(ctx, d_or.put(origin_ns, 8 * (size_t)N));
    HIP_TRY(ctx, d_q.put(q, 8 * (size_t)N * cells));
    HIP_TRY(ctx, d_n.put(n, 4 * (size_t)N * cells));
    double *d_lo = outs.want(lo, 8 * L * NH), *d_hi = outs.want(hi, 8 * L * NH);
    int8_t *d_cell = outs.want(cell, L * NH);
    if (int rc = outs.ready(ctx)) return rc;
    if (int rc = calib_apply_run(ctx, N, H, d_yh.as<double>(), d_lw.as<double>(), d_up.as<double>(), d_ds.as<int64_t>(),
                                 shared_future, d_or.as<int64_t>(), d_q.as<double>(), d_n.as<int32_t>(), *args, d_lo, d_hi,
                                 d_cell, nullptr))
        return rc;
    HIP_TRY(ctx, hipDeviceSynchronize());
    return outs.fetch(ctx);
}

extern "C" int tsf_calibrate(tsf_ctx *ctx, const tsf_spec *spec, int64_t N, int32_t T, const int64_t *offsets,
                             const int64_t *ds, const void *y, int32_t y_dtype, const double *floor_, const double *cap,
                             const double *extra, const tsf_cv_args *args, const int64_t *series_key, int32_t n_samples,
                             double interval_width, uint64_t seed, const tsf_calib_args *calib, tsf_calib_table *table,
                             tsf_cv_out *cv_out)
{
    if (!ctx) return -1;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (int rc = check_calib_args(ctx, calib)) return rc;
    if (int rc = check_calib_table(ctx, table)) return rc;
    return cross_validate_run(ctx, spec, PanelIn{N, T, offsets, ds, y, y_dtype, floor_, cap, extra}, args, series_key,
                              n_samples, interval_width, seed, cv_out, calib, table);
}
