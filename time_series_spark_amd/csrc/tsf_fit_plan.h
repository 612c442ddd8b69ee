// tsf_fit_plan.h -- which kernels a fit call runs and on what workspace: the decision of run_fit (tsf_api.hip) as a
// pure host function.  plan_fit makes no HIP call, touches no context and does not allocate; tsf_fit_plan
// (include/tsf_dev.h) exposes it, and tests/test_fit_plan.py pins it on the CPU.
#pragma once
#include <cmath>
#include <cstring>

#include "../../include/tsf_dev.h"
#include "tsf_fit_kernels.h"
#include "tsf_quad_kernels.h"
#include "tsf_mfma_tabs.h"
#include "tsf_launch.h"

namespace tsf {

// parameters of the FIT: with no changepoints the model is fitted on one dummy changepoint
// (GridTab::S_fit), so there is always at least one delta
static inline int fit_P(int n_cp, int K) { return 3 + (n_cp > 0 ? n_cp : 1) + K; }

// launch plan of the matrix-core residual kernel
struct MfmaPlan { int on, NG, KF, NCB, rr0, blocks; };

// The host's choice for one fit launch (tsf_fit_plan_info mirrors it field by field).  What a launch function falls
// back to where a shape has no instance, and what is decided on the device, is not in it.
struct FitPlan {
    int rc, err;                    // 0, or -1 and TSF_PLAN_* (fit_plan_message: the text)
    int route;                      // TSF_ROUTE_*
    int NTmax;                      // row steps per lane of the longest series
    int64_t n_grids;                // grid tables: 1 (aligned), one per calendar class, or one per series
    int shared_grids;               // the caller's calendar classes are used (FitArgs::grid_of)
    int64_t lat_U;                  // points of the shared lattice table (0: tables per grid)
    QuadPlan qp;                    // grid / LDS plan of the quadratic-form kernels (zero where none runs)
    int quad_ragged;                // Z^T Z slots per resident wave (WsLayout::Mslot)
    MfmaPlan mp;
    int coop, coop_after, coop_slots, coop_stride;      // cooperative tail of the one-wave kernel
    int sparse_try;                 // sparse_extra_kernel decides on the device whether the sparse-column form runs
    int64_t quad_pre;               // Z^T Z prebuilt per calendar class: their number
    int harm, gram_harm, resid_harm, map_harm;          // base-pair expansion (harm_code) per consumer; 0: tables
    int bw_ns;                      // seasonalities of the base-pair table (0: none)
    int raw_y;                      // the fit reads the caller's y rows (no scaled copy)
};

static inline const char *fit_plan_message(int err)
{
    static const char *const msg[TSF_PLAN_ERR_COUNT] = {
        "",
        "no rows",
        "series too long (TSF_MAX_T rows per series)",
        "Newton needs 3 + n_changepoints + K <= 128",
        "eval_form QUADRATIC needs linear growth, additive columns only and history == 5",
        "the quadratic form needs an aligned panel, linear growth, additive columns only and 3 + n_changepoints + K <= 64",
        "residual_kernel MFMA does not take specified changepoints (changepoints_specified = 1)",
        "residual_kernel MFMA needs an aligned panel, K <= 28 columns of one mode, 3+S+K <= 64 and S <= 28",
        "residual_kernel COOP needs a residual-form L-BFGS fit of series of at most 4096 rows"};
    return (err >= 0 && err < TSF_PLAN_ERR_COUNT) ? msg[err] : "";
}

static inline FitPlan fit_plan_error(int err)
{
    FitPlan p;
    memset(&p, 0, sizeof(p));
    p.rc = -1; p.err = err;
    return p;
}

// "bytes this context can have" (free memory + its own workspace), asked at most once per plan and only where the
// table rule below needs it; < 0: unknown
struct MemQuery { int64_t (*fn)(void *); void *arg; };

// checkpoint slots of the cooperative tail: one per fit that can be suspended at a time -- the blocks
// resident when the launch runs dry (a few thousand), all series of a small call
// (after: FitArgs::coop_after.  COOP_DIRECT suspends nothing; the tail rule (< 0) suspends at most the fits
// still running when no more of them are left than there are CUs -- 2 n_cu covers the waves racing past the
// test; an explicit hand-over point (>= 0: tests, latency mode) can suspend every running fit)
static inline int coop_slots_for(int64_t N, int after, int n_cu)
{
    if (after == COOP_DIRECT) return 0;
    const int64_t cap = after >= 0 ? 8192 : 8 * (int64_t)n_cu;      // (hand-over at up to ~4 fits per CU, twice that for the waves racing past the test)
    return (int)(N < cap ? N : cap);
}

// grid / LDS plan of the quadratic-form kernel for this device
static inline void quad_plan(const DevSpec &hs, int64_t N, const int *opt, int n_cu, QuadPlan *qp)
{
    const int P = fit_P(hs.n_cp, hs.K);
    qp->PPL = (hs.KP == 64) ? 2 : 1;
    // rows of M the kernel walks: compile-time 40 / 56 / 64 for the one-slot kernels (zero rows
    // beyond P are bit-neutral), P rounded up to 4 for the two-slot kernel
    qp->P4 = (qp->PPL == 2) ? ((P + 3) & ~3) : (P <= 40 ? 40 : (P <= 56 ? 56 : 64));
    qp->NW = quad_waves_per_block(qp->PPL);       // the most any variant launches: sizes the slots
    qp->n_cu = n_cu;
    qp->opt = opt;
    int64_t blocks = n_cu;                          // persistent: LDS admits one workgroup per CU
    const int64_t need = (N + qp->NW - 1) / qp->NW;
    if (blocks > need) blocks = need;
    if (blocks < 1) blocks = 1;
    qp->blocks = (int)blocks;
    // resident waves over all kernel variants (their workgroups hold 4, 8 or 12 waves; each launcher
    // sizes its own grid): at most n_cu x NW, and no more than one per series rounded up to a workgroup
    int64_t slots = (int64_t)n_cu * qp->NW;
    if (slots > N + qp->NW) slots = N + qp->NW;
    qp->slots = (int)slots;
    if (qp->slots < qp->P4) qp->slots = qp->P4;
}

// The model's Fourier block has a compiled base-pair expansion (eval_fg HARM): yearly 10 + weekly 3 on the 28-column
// kernel, weekly 3 + daily 4 (16 columns), weekly 3 (8 columns).  (DevSpec::harm is 0 for mixed column modes.)
static inline bool harm_compiled(const DevSpec &hs)
{
    return (hs.harm == HARM_Y10_W3 && hs.KP == 28) || (hs.harm == HARM_W3_D4 && hs.KP == 16) || (hs.harm == HARM_W3 && hs.KP == 8);
}

// ... and the model is exactly that block: nothing behind the Fourier columns
static inline bool harm_only(const DevSpec &hs) { return harm_compiled(hs) && hs.K == harm_kf(hs.harm); }

// Points of the shared lattice table a residual-form fit of a ragged panel on a timestamp lattice uses; 0: a table
// per grid.  (Explicit columns are per row, not per timestamp: never the lattice.)
static inline int64_t plan_lattice(const DevSpec &hs, const tsf_fit_shape &sh, const int *opt, const FitPlan &p, MemQuery mem)
{
    if (sh.aligned || hs.n_extra > 0 || sh.lat_step <= 0 || sh.lat_U <= 0) return 0;
    // Series that share timestamp vectors (grid_of) have step-major tables per DISTINCT vector: where those fit the
    // caches (<= 64 MB of design tables) every wave reads them coalesced, as on an aligned panel, and the lattice
    // table with its gathered rows (64 cache lines per load instruction) is the slower of the two.
    // tsf_set_option(TSF_OPT_LATTICE, 0): never the lattice table; 1: always where it applies.
    // Round 5: a model whose Fourier columns have a compiled expansion reads 32-byte base pairs per row from its OWN
    // tables (eval_fg HARM) -- faster than the gathered 224-byte rows of the lattice table in the one-wave kernel (ragged
    // bench panel, a grid per series: 93 -> 60 ms) and, above all, in the cooperative tail (gathered rows stream: 11 us
    // per evaluation against 5) -- wherever a table per series is affordable: <= 32 GB of design tables per call
    // (~190 000 series of 730 rows) AND no more than two fifths of the memory this context can have (what is free
    // now + its own cached workspace; the tables are ~4/5 of the layout): several contexts or ranks on one GPU, or
    // a smaller part, keep the shared lattice table -- the route that needs no table per series -- instead of
    // failing in ensure_ws (round-5 advice).
    // Round 6: the base-pair kernels read a lattice panel too (rows of 22 bytes + the lattice POINTS' pairs from one
    // shared table, FitArgs::Bu: as fast or faster than a table per series -- 10 000 / 2 000 series at their own subsets
    // of a daily lattice: 75.9 -> 74.5 / 31.1 -> 27.0 ms -- for 0.44 of the traffic and none of the 2 GB of tables), so
    // such a model keeps the lattice (its MAP continuation too).
    const int el = opt[TSF_OPT_LATTICE];
    if (el >= 0) return el == 0 ? 0 : sh.lat_U;
    const size_t tab = sizeof(double) * (size_t)p.n_grids * (size_t)p.NTmax * hs.KP * W;
    if (p.shared_grids && tab <= ((size_t)64 << 20)) return 0;
    if (opt[TSF_OPT_HARM] != 0 && harm_compiled(hs) && !harm_only(hs)) {
        size_t harm_cap = (size_t)32 << 30;
        if (tab > ((size_t)256 << 20)) {        // (the one place a plan asks the device anything; unknown: the 32 GB stand)
            const int64_t avail = mem.fn(mem.arg);
            if (avail >= 0 && (size_t)avail / 5 * 2 < harm_cap) harm_cap = (size_t)avail / 5 * 2;
        }
        if (tab <= harm_cap) return 0;
    }
    return sh.lat_U;
}

// matrix-core residual kernel (tsf_mfma_kernels.h): aligned panel, L-BFGS, one parameter per lane
// (KP <= 28 implies one column mode and P <= 64), at most MT_SP changepoints, and an upper bound
// on the changepoint rows one chunk can hold (the exact count is checked on the device:
// MfmaTabs::overflow routes the call to the one-wave kernel)
static inline MfmaPlan plan_mfma(const DevSpec &hs, const tsf_fit_shape &sh, int NTmax, int n_cu)
{
    MfmaPlan mp;
    memset(&mp, 0, sizeof(mp));
    if (!sh.aligned || hs.KP > 28) return mp;
    const int hist_rows = (int)floor((double)sh.Tm * hs.cp_range);
    int S = hs.n_cp;
    if (S + 1 > hist_rows) S = hist_rows - 1;
    if (S < 1) S = 1;
    const double step = (hs.n_cp > 0 && S > 0) ? (double)(hist_rows - 1) / (double)S : 1e30;
    const int per_chunk = (int)ceil((double)NTmax / (step > 1.0 ? step : 1.0)) + 2;
    if (S <= MT_SP && per_chunk <= MT_MAXCP && mfma_lds_bytes(hs.KP) <= 160 * 1024) {
        mp.on = 1;
        mp.NG = (NTmax + 15) / 16;
        mp.KF = hs.KP / 4;
        mp.NCB = (hs.KP + 15) / 16;
        mp.rr0 = (16 * mp.NG - NTmax) / 4;
        int64_t blocks = (sh.N + MT_NS - 1) / MT_NS;
        if (blocks > n_cu) blocks = n_cu;
        mp.blocks = (int)blocks;
    }
    return mp;
}

// The cooperative tail of the one-wave residual kernel (coop_ok: the call can have one), and where fits are handed over
// (FitArgs::coop_after).  TSF_RK_COOP: the cooperative kernel runs every fit from
// its first evaluation (no one-wave phase, no checkpoints).  AUTO does the same for the models whose one-wave
// kernel holds two parameters per lane (KP = 64) on series too long for the grouped column sums: that kernel
// needs > 256 registers (one wave per SIMD) and measures 9.6 M evaluations/s on 50 000 x 730 with 56 columns,
// the workgroup kernel 11.4+ M.
// Round 3: on series of <= 768 rows the one-wave kernel of these models takes its per-column sums in groups
// of 8 (eval_fg GNTR: 187 instead of 379 registers, two waves per SIMD) and allocates only the history pairs
// it uses (wave_lds_bytes: eight blocks per CU instead of six): 17.0 M evaluations/s on cfg4 against the
// workgroup kernel's 15.4 M (2.27 against 2.50 s) -- so AUTO runs it, with the workgroup kernel for the tail
// as for the narrower models.  tsf_set_option(TSF_OPT_FIT_GROUPED, 0): every series on the workgroup kernel, as before.
static inline void plan_coop(const DevSpec &hs, const tsf_spec *spec, int64_t N, const int *opt, int n_cu, bool coop_ok, FitPlan *p)
{
    p->coop = coop_ok && spec->residual_kernel != TSF_RK_WAVE;
    p->coop_after = spec->residual_kernel == TSF_RK_COOP ? COOP_DIRECT : spec->coop_after;
    if (!p->coop) return;
    const bool grouped = p->NTmax <= 12 && opt[TSF_OPT_FIT_GROUPED] != 0 && p->lat_U == 0;
    // (with sparse_try the slots of the tail exist either way: the dense route of longer series is then launched
    // in direct mode by the launch function itself)
    if (spec->residual_kernel == TSF_RK_AUTO && spec->coop_after < 0 && hs.KP == 64 && !grouped && !p->sparse_try) p->coop_after = COOP_DIRECT;
    p->coop_slots = coop_slots_for(N, p->coop_after, n_cu);
    p->coop_stride = coop_slot_doubles(hs.KP == 64 ? 2 : 1);
}

// Who reads the Fourier columns as base pairs (harm_code of the model, 0: from the design table).
// tsf_set_option(TSF_OPT_HARM, 0): nobody.  residual_lbfgs, quad, quad_eval: the route, as in plan_fit.
static inline void plan_harm(const DevSpec &hs, const tsf_spec *spec, const tsf_fit_shape &sh, const int *opt, bool residual_lbfgs,
                             bool quad, bool quad_eval, FitPlan *p)
{
    if (opt[TSF_OPT_HARM] == 0) return;
    // Fourier columns expanded from the rows' base pairs (eval_fg HARM): the residual-form one-wave kernel of models
    // whose harmonic structure has a compiled kernel -- yearly 10 + weekly 3 on the 28-column kernel and its
    // sparse-column form, weekly 3 + daily 4 (16 columns), weekly 3 (8 columns); never with the
    // matrix-core / workgroup-from-the-start routes.
    // Round 6: WITH the lattice table where the model is exactly one of those (nothing behind the Fourier block): a row keeps t, y, its segment word and its lattice point (22 bytes instead of 50) and the base pairs
    // are the point's, from one table of 32 bytes per point that every series shares (FitArgs::Bu) -- no table per series.
    if (residual_lbfgs && (p->lat_U > 0 ? harm_only(hs) : (harm_compiled(hs) || (hs.harm == HARM_Y10_W3 && p->sparse_try))))
        p->harm = hs.harm;
    // The same base pairs for the Gram build of a ragged quadratic-form panel whose series have a calendar each (the M-in-
    // registers kernel builds Z^T Z per series: gram_columns_harm, tsf_quad_kernels.h); shared calendars build once per
    // calendar (quad_pre) and keep reading the tables.
    if (quad && !sh.aligned && !p->quad_pre && hs.harm == HARM_Y10_W3 && hs.KP == 28) p->gram_harm = hs.harm;
    // ... and for the residual passes of an ALIGNED quadratic-form call with one parameter per lane (the 12- and 16-wave
    // kernels, the M-in-registers kernel, tsf_eval_quadratic): rows as base pairs, the column sums taken in the row sweep
    // itself (ztr_sweep_harm, tsf_quad_kernels.h) -- every compiled shape, dense columns behind the Fourier block allowed.
    // Two-slot kernels (P > 64), ragged calls and other models keep the two-sweep table route.
    if ((quad || quad_eval) && sh.aligned && p->qp.PPL == 1 && harm_compiled(hs)) p->resid_harm = hs.harm;
    // ... and for the MAP continuation (tsf_map_kernels.h): its evaluator reads base-pair rows wherever the model has a
    // compiled expansion, whatever kernel ran the Stan-rule fit (the quadratic-form route builds the table for it)
    if (spec->converge == TSF_CONVERGE_MAP && sh.call == TSF_CALL_FIT && harm_only(hs)) p->map_harm = hs.harm;
}

// The plan of one fit launch.  hs, mode: build_devspec's; opt: the context's route switches; mem: asked at most once,
// and only by plan_lattice's table rule.
static inline FitPlan plan_fit(const DevSpec &hs, int mode, const tsf_spec *spec, const tsf_fit_shape &sh, const int *opt,
                               int n_cu, MemQuery mem)
{
    if (sh.Tm < 1) return fit_plan_error(TSF_PLAN_NO_ROWS);
    if (sh.Tm > TSF_MAX_T) return fit_plan_error(TSF_PLAN_TOO_LONG);
    FitPlan p;
    memset(&p, 0, sizeof(p));
    p.NTmax = (sh.Tm + W - 1) / W;
    // ragged panel whose series share timestamp vectors (fit_host found n_distinct < N of them): one set of grid tables
    // per distinct vector
    p.shared_grids = !sh.aligned && sh.classes && sh.n_distinct > 0 && sh.n_distinct < sh.N;
    p.n_grids = sh.aligned ? 1 : (p.shared_grids ? sh.n_distinct : sh.N);
    const bool fit = sh.call == TSF_CALL_FIT;
    const bool linear_additive = hs.growth == TSF_GROWTH_LINEAR && mode == 0;
    // Stan's Newton optimiser (tsf_newton_kernels.h): explicitly, or by fbprophet's rule on the
    // longest series of the call
    const bool newton = fit && (spec->algorithm == TSF_ALGO_NEWTON ||
                                (spec->algorithm == TSF_ALGO_AUTO && sh.Tm < TSF_NEWTON_BELOW_T));
    // (more than 64 parameters, or mixed additive / multiplicative columns: newton_kernel2, two parameters per lane)
    if (newton && fit_P(hs.n_cp, hs.K) > 2 * W) return fit_plan_error(TSF_PLAN_NEWTON_WIDE);
    // quadratic (Gram) form of the data term: see tsf_quad_kernels.h
    const bool quad_ok = linear_additive && hs.history == QH && fit && !newton;
    if (spec->eval_form == TSF_EVAL_QUADRATIC && !quad_ok && fit) return fit_plan_error(TSF_PLAN_QUAD_FORM);
    const bool quad = quad_ok && spec->eval_form != TSF_EVAL_RESIDUAL;
    // Newton on the same models: residual form at the accepted points, quadratic form for the
    // finite-difference and halving evaluations (tsf_newton_quad.h); aligned panels
    const bool newton_quad = newton && linear_additive && hs.KP <= 28 && spec->eval_form != TSF_EVAL_RESIDUAL && p.NTmax <= 16;
    // tsf_eval_quadratic: one quadratic-form evaluation at theta_in around the reference point theta_ref
    const bool quad_eval = sh.call == TSF_CALL_EVAL_QUADRATIC;
    if (quad_eval && !(sh.aligned && linear_additive && hs.KP != 64)) return fit_plan_error(TSF_PLAN_QUAD_EVAL);
    if (quad || newton_quad || quad_eval) {
        quad_plan(hs, sh.N, opt, n_cu, &p.qp);
        if (newton_quad) {          // one-wave workgroups, up to 16 per CU: that many Z^T Z slots (ragged)
            p.qp.slots = n_cu * 16;
            if (p.qp.slots < p.qp.P4) p.qp.slots = p.qp.P4;
        }
    }
    p.quad_ragged = (quad || newton_quad) && !sh.aligned;
    // a residual-form L-BFGS fit, whichever kernel runs it
    const bool residual_fit = fit && !quad && !newton;
    if (residual_fit) p.lat_U = plan_lattice(hs, sh, opt, p, mem);
    // TSF_RK_AUTO = the one-wave kernel.  Measured (profiles/r02_mfma_vs_wave.txt): both kernels issue
    // the same number of vector instructions per evaluation and are bound by them -- fp64 MFMA has
    // the vector unit's rate, and the 672 multiply-adds it takes over are 16 % of an evaluation --
    // so once the reductions of the optimiser were cut (uniform butterflies) the one-wave kernel,
    // which has no rounds to synchronise, is ahead on every panel measured (100 000 x 730, iteration
    // cap 150: 271 vs 326 ms; reference settings with their stragglers: 1.27 vs 1.62 s).  The
    // matrix-core kernel stays available (TSF_RK_MFMA), bit-identical.
    // Specified changepoints: rejected -- plan_mfma's per_chunk bounds the changepoint rows of a chunk by the automatic
    // rule's spacing, which dates at arbitrary places do not have.
    const bool want_mfma = spec->residual_kernel == TSF_RK_MFMA;
    if (want_mfma && hs.cp_spec && fit) return fit_plan_error(TSF_PLAN_MFMA_CHANGEPOINTS);
    if (want_mfma && residual_fit) {
        p.mp = plan_mfma(hs, sh, p.NTmax, n_cu);
        if (!p.mp.on) return fit_plan_error(TSF_PLAN_MFMA_SHAPE);
    }
    // ... on the one-wave kernel (with its cooperative tail): the guard of everything that kernel alone can do
    const bool residual_lbfgs = residual_fit && !p.mp.on;
    p.route = newton_quad ? TSF_ROUTE_NEWTON_QUAD : newton ? TSF_ROUTE_NEWTON : quad_eval ? TSF_ROUTE_QUAD_EVAL :
              quad ? TSF_ROUTE_QUAD_LBFGS : p.mp.on ? TSF_ROUTE_MFMA : TSF_ROUTE_WAVE;
    // cooperative tail of the one-wave residual kernel: series of at most COOP_MAX_NT steps per chunk
    // (the rows of one evaluation are staged in the workgroup's LDS)
    const bool coop_ok = residual_lbfgs && p.NTmax <= COOP_MAX_NT;
    if (spec->residual_kernel == TSF_RK_COOP && !coop_ok && fit) return fit_plan_error(TSF_PLAN_COOP_SHAPE);
    // Wide models (64-column tables) whose columns from the 29th on are explicit columns -- holidays: 0 / 1 indicators,
    // almost all 0 -- are tried on the sparse-column form of the 28-column kernel (eval_fg<..., SPARSE>, tsf_fit_kernels.h):
    // sparse_extra_kernel decides on the device whether every grid qualifies, the dense route is launched behind it
    // with the opposite guard (series of <= 768 rows: the grouped one-wave kernel; up to 4 096 rows: the workgroup
    // kernel from the first evaluation; longer: the ungrouped one-wave kernel).  tsf_set_option(TSF_OPT_SPARSE_EXTRA, 0): never.
    p.sparse_try = residual_lbfgs && p.lat_U == 0 && hs.KP == 64 && mode != 2 &&
                   spec->residual_kernel == TSF_RK_AUTO && hs.K > SP_DENSE && hs.K <= SP_DENSE + SP_MAXC &&
                   hs.K - hs.n_extra <= SP_DENSE && p.NTmax <= SP_MAX_NT && opt[TSF_OPT_SPARSE_EXTRA] != 0;
    plan_coop(hs, spec, sh.N, opt, n_cu, coop_ok, &p);
    // ragged panel, quadratic form, series sharing timestamp vectors: Z^T Z once per distinct vector (gram_grids_kernel)
    // instead of once per series inside the fit kernel -- when that at least halves the builds (TSF_OPT_GRAM_SHARE 0: never)
    p.quad_pre = (quad && p.shared_grids && p.n_grids * 2 <= sh.N && opt[TSF_OPT_GRAM_SHARE] != 0) ? p.n_grids : 0;
    plan_harm(hs, spec, sh, opt, residual_lbfgs, quad, quad_eval, &p);
    p.bw_ns = (p.harm || p.gram_harm || p.resid_harm || p.map_harm) ? hs.n_seas : 0;
    // Quadratic-form L-BFGS fits read the caller's y rows themselves (FitArgs::y_raw) instead of a scaled step-major copy
    // that setup_series_kernel would write and they would read back -- a second f64 panel on the device and half of the
    // step's HBM bytes.  Not when the MAP continuation follows (its evaluator reads yw).
    p.raw_y = quad && spec->converge != TSF_CONVERGE_MAP && opt[TSF_OPT_QUAD_RAW_Y] != 0;
    return p;
}

static inline void fit_plan_info(const FitPlan &p, tsf_fit_plan_info *o)
{
    memset(o, 0, sizeof(*o));
    o->n_grids = p.n_grids; o->lat_U = p.lat_U; o->quad_pre = p.quad_pre;
    o->err = p.err; o->route = p.route; o->NTmax = p.NTmax; o->shared_grids = p.shared_grids;
    o->quad_P4 = p.qp.P4; o->quad_PPL = p.qp.PPL; o->quad_NW = p.qp.NW; o->quad_blocks = p.qp.blocks;
    o->quad_slots = p.qp.slots; o->quad_ragged = p.quad_ragged;
    o->mfma_on = p.mp.on; o->mfma_NG = p.mp.NG; o->mfma_KF = p.mp.KF; o->mfma_NCB = p.mp.NCB; o->mfma_rr0 = p.mp.rr0;
    o->mfma_blocks = p.mp.blocks;
    o->coop = p.coop; o->coop_after = p.coop_after; o->coop_slots = p.coop_slots; o->coop_stride = p.coop_stride;
    o->sparse_try = p.sparse_try; o->harm = p.harm; o->gram_harm = p.gram_harm; o->resid_harm = p.resid_harm;
    o->map_harm = p.map_harm; o->bw_ns = p.bw_ns; o->raw_y = p.raw_y;
}

}  // namespace tsf
