// tsf_shares.h -- what the device unit (tsf_api.hip) shares with the host-only code of tsf_shares.cpp.  No HIP header and no
// tsf_ctx: a check here writes its message into the caller's buffer and returns non-zero; the device unit hands that
// message to fail(ctx, ...) (tsf_api.hip).  The four solvers themselves are declared in include/tsf.h.
#pragma once
#include <cstddef>
#include <cstdint>
#include <new>
#include <vector>

#include "../../include/tsf.h"

#pragma GCC visibility push(hidden)

// The windows of a call (host data, like the levels) and the observed window totals (device memory behind the entries).
struct WindowCall {
    int32_t K;
    const int32_t *win_start, *win_end;
    const double *y_win;
};

constexpr size_t WINDOW_MSG = 160;      // bytes of the message a window check writes

// the windows of a call against H: they index the sample buffer
int check_windows(int32_t H, const WindowCall &w, char (&msg)[WINDOW_MSG]);
// No row in two windows (the windows have passed check_windows).  May throw std::bad_alloc.
int check_disjoint_windows(int32_t H, const WindowCall &w, char (&msg)[WINDOW_MSG]);

// The small CSR of one add call, per scratch chunk [n0, n0 + nc): the groups the chunk touches (ascending) and, per
// such group, its chunk-local members in ascending order.  One int32 buffer: touched | first | member.
struct RollupPlan {
    std::vector<int32_t> touched, first, member;            // all chunks, one after another
    std::vector<size_t> t0, f0;                             // per chunk: where its touched / first entries start
};

void rollup_plan(const int64_t *group, int64_t N, int64_t chunk, RollupPlan *P);

// p0 = phi^steps as tsf_set_noise_ar_start and tsf_noise_ar_mean form it
double ar_start_p0(double phi, int32_t steps);

#pragma GCC visibility pop
