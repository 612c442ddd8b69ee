// tsf_cond_kernels.h -- the design columns of conditional seasonalities (include/tsf.h, "conditional seasonalities":
// tsf_cond_columns).  One launch: cond_columns_kernel, one thread per (row, seasonality), consecutive threads on
// consecutive rows, so every store of a wave is one contiguous run of one column.
// A value is a function of (ds[i], period, harmonic, cond[c][i]) alone: the base pair from dm_sincos at
// fourier_base_arg, the harmonics by fourier_harmonics -- the statements setup_grid_kernel makes for an unconditional
// seasonality (tsf_aux_kernels.h), so the bits are those of its table --, and +0.0 where the condition is false.
// Nothing here knows the panel's first timestamp, the number of rows or the launch shape.
// Non-template __global__ function: include from exactly one translation unit (tsf_api.hip).
#pragma once
#include "tsf_common.h"

namespace tsf {

struct CondArgs {
    const int64_t *ds;                  // [rows]
    const uint8_t *cond;                // [n_cond][rows], non-zero = true
    double *cols;                       // [sum 2 * order][col_stride]
    int64_t rows, col_stride;
    int32_t n;                          // conditional seasonalities (gridDim.y)
    double period[TSF_MAX_SEAS];
    int32_t order[TSF_MAX_SEAS];
    int32_t cond_row[TSF_MAX_SEAS];     // its row of cond
    int32_t col0[TSF_MAX_SEAS];         // its first column: sin 1, cos 1, sin 2, cos 2, ... from there
};

constexpr int COND_BLOCK = 256;

__global__ __launch_bounds__(COND_BLOCK) void cond_columns_kernel(CondArgs a)
{
    const int se = blockIdx.y;
    const double period = a.period[se];
    const int order = a.order[se];
    const uint8_t *__restrict__ on = a.cond + (size_t)a.cond_row[se] * (size_t)a.rows;
    double *__restrict__ out = a.cols + (size_t)a.col0[se] * (size_t)a.col_stride;
    for (int64_t i = (int64_t)blockIdx.x * COND_BLOCK + threadIdx.x; i < a.rows; i += (int64_t)gridDim.x * COND_BLOCK) {
        const bool keep = on[i] != 0;
        double s1, c1;
        dm_sincos(fourier_base_arg(a.ds[i], period), s1, c1);
        fourier_harmonics(s1, c1, order, [&](int h, double sv, double cv) {
            out[(size_t)(2 * (h - 1)) * (size_t)a.col_stride + (size_t)i] = keep ? sv : 0.0;
            out[(size_t)(2 * (h - 1) + 1) * (size_t)a.col_stride + (size_t)i] = keep ? cv : 0.0;
        });
    }
}

}  // namespace tsf
