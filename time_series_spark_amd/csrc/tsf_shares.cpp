// tsf_shares.cpp -- the host-only solvers of include/tsf.h and the host-only plans and checks beside them: the shares
// of the two-level, tree and temporal reconciliation (tsf_reconcile_shares, tsf_reconcile_tree_shares,
// tsf_temporal_shares), the conditional mean of the AR(1) start (tsf_noise_ar_mean, ar_start_p0), the window checks
// and the roll-up's add plan.  No HIP header, no tsf_ctx: the file builds with any C++17 compiler, so it can join the
// stand-alone host builds (tests/c/host_san.cpp).
//
// Compile flags: build.py gives a .cpp file the flags of the .hip files, -ffp-contract=off among them, and that must stay
// so: the reference tests (tests/test_reconcile_ref.py, test_tree_ref.py, test_temporal_ref.py, test_ar_start_ref.py)
// compare bits, and the sums here are written for it -- from +0.0 in ascending index, `a = a + b`, one rounding per
// operation.
#include "tsf_shares.h"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <utility>

void rollup_plan(const int64_t *group, int64_t N, int64_t chunk, RollupPlan *P)
{
    P->member.resize((size_t)N);
    std::vector<std::pair<int64_t, int32_t>> order;
    for (int64_t n0 = 0; n0 < N; n0 += chunk) {
        const int64_t nc = (N - n0 < chunk) ? N - n0 : chunk;
        order.clear();
        for (int64_t i = 0; i < nc; ++i) order.push_back({group[n0 + i], (int32_t)i});
        std::sort(order.begin(), order.end());              // by group, then by index in the call
        P->t0.push_back(P->touched.size());
        P->f0.push_back(P->first.size());
        for (int64_t i = 0; i < nc; ++i) {
            if (i == 0 || order[i].first != order[i - 1].first) {
                P->touched.push_back((int32_t)order[i].first);
                P->first.push_back((int32_t)i);
            }
            P->member[(size_t)(n0 + i)] = order[i].second;
        }
        P->first.push_back((int32_t)nc);
    }
}

// p0 = phi^steps: phi multiplied by itself steps - 1 more times, one rounding each.  The loop stops at the first zero (an
// underflow, or phi == 0) and keeps that zero with its sign.
double ar_start_p0(double phi, int32_t steps)
{
    double p0 = phi;
    for (int32_t k = 1; k < steps && p0 != 0.0; ++k) p0 = p0 * phi;
    return p0;
}

extern "C" int tsf_noise_ar_mean(int64_t n, const double *phi, const double *resid, const int32_t *steps, int32_t H,
                                 double *mean)
{
    if (n < 0 || H < 0 || (n > 0 && (!phi || !resid || !steps)) || (n > 0 && H > 0 && !mean)) return -1;
    for (int64_t i = 0; i < n; ++i)
        if (!(std::fabs(phi[i]) < 1.0) || !std::isfinite(resid[i]) || steps[i] < 1) return -1;
    for (int64_t i = 0; i < n; ++i) {
        double m = resid[i] * ar_start_p0(phi[i], steps[i]);
        for (int32_t h = 0; h < H; ++h) {
            mean[(size_t)i * H + h] = m;
            m = phi[i] * m;
        }
    }
    return 0;
}

// a refusal of the window checks: its message into the caller's buffer, non-zero
static int refuse(char (&msg)[WINDOW_MSG], const char *why)
{
    snprintf(msg, sizeof(msg), "%s", why);
    return -1;
}

// the windows of a call against H: they index the sample buffer
int check_windows(int32_t H, const WindowCall &w, char (&msg)[WINDOW_MSG])
{
    if (w.K < 1 || w.K > TSF_MAX_WINDOWS) return refuse(msg, "K must be in [1, TSF_MAX_WINDOWS]");
    if (!w.win_start || !w.win_end) return refuse(msg, "NULL win_start or win_end");
    for (int32_t k = 0; k < w.K; ++k)
        if (w.win_start[k] < 0 || w.win_start[k] >= w.win_end[k] || w.win_end[k] > H) {
            snprintf(msg, sizeof(msg), "window %d = [%d, %d): a window needs 0 <= win_start < win_end <= H = %d", (int)k,
                     (int)w.win_start[k], (int)w.win_end[k], (int)H);
            return -1;
        }
    return 0;
}

extern "C" int tsf_reconcile_shares(int64_t N, const int64_t *group, const double *w, int64_t G, const double *v,
                                    double *share, double *share_total)
{
    if (N < 0 || G < 0 || (N > 0 && (!group || !share)) || (G > 0 && (!v || !share_total))) return -1;
    for (int64_t n = 0; n < N; ++n) {
        if (group[n] < 0 || group[n] >= G) return -1;
        if (w && !(w[n] > 0.0 && std::isfinite(w[n]))) return -1;
    }
    for (int64_t g = 0; g < G; ++g)
        if (!std::isnan(v[g]) && !(v[g] > 0.0 && std::isfinite(v[g]))) return -1;
    // W_g in share_total, from +0.0 in ascending member index
    for (int64_t g = 0; g < G; ++g) share_total[g] = 0.0;
    for (int64_t n = 0; n < N; ++n) share_total[group[n]] = share_total[group[n]] + (w ? w[n] : 1.0);
    for (int64_t n = 0; n < N; ++n) {
        const int64_t g = group[n];
        share[n] = std::isnan(v[g]) ? 0.0 : (w ? w[n] : 1.0) / (v[g] + share_total[g]);
    }
    for (int64_t g = 0; g < G; ++g) {
        const double W = share_total[g];
        share_total[g] = (std::isnan(v[g]) || W == 0.0) ? 0.0 : W / (v[g] + W);
    }
    return 0;
}

extern "C" int tsf_reconcile_tree_shares(int64_t N, const int64_t *group, const double *w, int64_t G, int32_t n_upper,
                                         const int64_t *n_nodes, const int64_t *parent, const double *v, double *share,
                                         double *mu, double *e, double *kappa)
{
    if (N < 0 || G < 1 || n_upper < 0 || n_upper > TSF_TREE_MAX_LEVELS) return -1;
    if ((N > 0 && (!group || !share)) || !v || !mu || !e || !kappa || (n_upper > 0 && (!n_nodes || !parent))) return -1;
    int64_t M = G, below = G, n_par = 0;
    for (int32_t k = 0; k < n_upper; ++k) {
        if (n_nodes[k] < 1) return -1;
        for (int64_t c = 0; c < below; ++c)
            if (parent[n_par + c] < 0 || parent[n_par + c] >= n_nodes[k]) return -1;
        n_par += below; below = n_nodes[k]; M += below;
    }
    for (int64_t n = 0; n < N; ++n) {
        if (group[n] < 0 || group[n] >= G) return -1;
        if (w && !(w[n] > 0.0 && std::isfinite(w[n]))) return -1;
    }
    for (int64_t i = 0; i < M; ++i)
        if (!std::isnan(v[i]) && !(v[i] > 0.0 && std::isfinite(v[i]))) return -1;
    // E of a level in kappa's slots of that level until its own kappa is known
    double *E = kappa;
    for (int64_t g = 0; g < G; ++g) E[g] = 0.0;
    for (int64_t n = 0; n < N; ++n) E[group[n]] = E[group[n]] + (w ? w[n] : 1.0);
    for (int64_t n = 0; n < N; ++n) share[n] = (w ? w[n] : 1.0) / E[group[n]];
    int64_t off = 0;
    below = G; n_par = 0;
    for (int32_t k = 0; k <= n_upper; ++k) {
        for (int64_t i = off; i < off + below; ++i) {
            const double En = E[i];
            if (!std::isnan(v[i]) && En > 0.0) {
                mu[i] = En / (v[i] + En);
                e[i] = (En * v[i]) / (v[i] + En);
            } else {
                mu[i] = 0.0;
                e[i] = En;
            }
        }
        if (k == n_upper) {
            for (int64_t i = off; i < off + below; ++i) kappa[i] = 0.0;        // the top level has no parent
            break;
        }
        const int64_t up = off + below, n_up = n_nodes[k];
        for (int64_t p = 0; p < n_up; ++p) E[up + p] = 0.0;
        for (int64_t c = 0; c < below; ++c) E[up + parent[n_par + c]] = E[up + parent[n_par + c]] + e[off + c];
        for (int64_t c = 0; c < below; ++c) {
            const double Ep = E[up + parent[n_par + c]];
            kappa[off + c] = Ep == 0.0 ? 0.0 : e[off + c] / Ep;
        }
        n_par += below; off = up; below = n_up;
    }
    return 0;
}

// No row in two windows (the windows have passed check_windows).
int check_disjoint_windows(int32_t H, const WindowCall &w, char (&msg)[WINDOW_MSG])
{
    std::vector<int32_t> owner((size_t)H, -1);
    for (int32_t k = 0; k < w.K; ++k)
        for (int32_t h = w.win_start[k]; h < w.win_end[k]; ++h) {
            if (owner[(size_t)h] >= 0) {
                snprintf(msg, sizeof(msg), "windows %d and %d overlap at row %d: a row would get two corrections",
                         (int)owner[(size_t)h], (int)k, (int)h);
                return -1;
            }
            owner[(size_t)h] = k;
        }
    return 0;
}

extern "C" int tsf_temporal_shares(int64_t N, int32_t H, int32_t K, const int32_t *win_start, const int32_t *win_end,
                                   const double *w, const double *v, double *share, double *share_total)
{
    if (N < 0 || H < 1 || (N > 0 && (!v || !share || !share_total))) return -1;
    const WindowCall wc = {K, win_start, win_end, nullptr};
    char msg[WINDOW_MSG];           // (this entry has no context to leave it in)
    try {
        if (check_windows(H, wc, msg) || check_disjoint_windows(H, wc, msg)) return -1;
    } catch (const std::bad_alloc &) {
        return -1;
    }
    const size_t nh = (size_t)N * H, nk = (size_t)N * K;
    for (size_t i = 0; w && i < nh; ++i)
        if (!(w[i] > 0.0 && std::isfinite(w[i]))) return -1;
    for (size_t i = 0; i < nk; ++i)
        if (!std::isnan(v[i]) && !(v[i] > 0.0 && std::isfinite(v[i]))) return -1;
    for (int64_t n = 0; n < N; ++n) {
        const double *wn = w ? w + (size_t)n * H : nullptr;
        double *sh = share + (size_t)n * H;
        for (int32_t h = 0; h < H; ++h) sh[h] = 0.0;
        for (int32_t k = 0; k < K; ++k) {
            const double vk = v[(size_t)n * K + k];
            double *mu = share_total + (size_t)n * K + k;
            if (std::isnan(vk)) { *mu = vk; continue; }
            double W = 0.0;
            for (int32_t h = win_start[k]; h < win_end[k]; ++h) W = W + (wn ? wn[h] : 1.0);
            const double D = vk + W;
            for (int32_t h = win_start[k]; h < win_end[k]; ++h) sh[h] = (wn ? wn[h] : 1.0) / D;
            *mu = W / D;
        }
    }
    return 0;
}
