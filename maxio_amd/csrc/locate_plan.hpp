// locate_plan.hpp — host side of mxec_locate: the per-(k, m) tables the
// locate kernel (rs_kernel.hip rs_locate_*) reads on a syndrome mismatch,
// and what a finished mxec_locate_result amounts to (mxec_locate_outcome).
//
// With P the m x k parity rows of the encoding matrix, a corruption e confined
// to data shard j leaves the syndrome column s = P[:, j] * e, so
// s_1 / s_0 = P[1][j] / P[0][j] whatever e is.  The matrix is MDS: every
// entry of P is non-zero and no two columns are proportional, so that ratio
// names j.  The kernel looks j up in `ratio -> j` and confirms the other rows
// against log(P[i][j] / P[0][j]).
//
// Host-only (no HIP, no I/O): built into libmaxio_ec.so and, on its own with
// -fsanitize=address,undefined, into the CPU test harness
// tests/c_manifest/locate_plan_check.cpp.
#pragma once

#include <cstdint>
#include <cstring>

#include "../../include/maxio_ec.h"

namespace mxec {

// Field tables the kernel's slow path divides with: log at [0, 256) (log[0]
// unused), exp at [256, 512) (exp[255] = exp[0]).  Polynomial 0x11D,
// generator 2, as gf256.cpp.
constexpr uint32_t kLocateFieldBytes = 512;
inline void locate_field_tables(uint8_t* out) {
    std::memset(out, 0, kLocateFieldBytes);
    unsigned b = 1;
    for (unsigned i = 0; i < 255; ++i) {
        out[256 + i] = uint8_t(b);
        out[b] = uint8_t(i);
        b <<= 1;
        if (b & 0x100) b ^= 0x11D;
    }
    out[256 + 255] = out[256];
}

// No data shard has this ratio.
constexpr uint8_t kLocateNoColumn = 0xFF;

// One (k, m)'s table: [0, 256) ratio -> j (kLocateNoColumn where no column
// has it), then m rows of 256: row i, entry j = log(P[i][j] / P[0][j]) for
// j < k (row 0 is zero, row 1 the log of column j's ratio).
inline uint32_t locate_table_bytes(int m) { return 256u * uint32_t(1 + m); }

// rows: the m x k parity rows, row-major.  2 <= m <= 8, 1 <= k <= 254 (so a
// column index never equals kLocateNoColumn).  MXEC_E_SINGULAR_MATRIX if an
// entry is zero or two columns share a ratio -- a matrix that is not MDS.
inline int locate_build_table(const uint8_t* rows, int k, int m, uint8_t* out) {
    if (!rows || !out || m < 2 || m > 8 || k < 1 || k > 254) return MXEC_E_INVALID_ARG;
    uint8_t f[kLocateFieldBytes];
    locate_field_tables(f);
    const uint8_t* lg = f;
    const uint8_t* ex = f + 256;
    std::memset(out, 0, locate_table_bytes(m));
    std::memset(out, kLocateNoColumn, 256);
    for (int j = 0; j < k; ++j) {
        const uint8_t p0 = rows[j];
        if (!p0) return MXEC_E_SINGULAR_MATRIX;
        for (int i = 1; i < m; ++i) {
            const uint8_t pi = rows[size_t(i) * size_t(k) + size_t(j)];
            if (!pi) return MXEC_E_SINGULAR_MATRIX;
            int d = int(lg[pi]) - int(lg[p0]);
            if (d < 0) d += 255;
            out[256 * (1 + i) + j] = uint8_t(d);
        }
        const uint8_t ratio = ex[out[256 * 2 + j]];
        if (out[ratio] != kLocateNoColumn) return MXEC_E_SINGULAR_MATRIX;  // proportional columns
        out[ratio] = uint8_t(j);
    }
    return MXEC_OK;
}

// CLEAN: no bad column.  ONE: every bad column named the same shard.  MANY:
// anything else (two shards, or a column that fits no single shard).
inline int locate_outcome(const mxec_locate_result* r, uint32_t* shard) {
    if (r->n_bad == 0) return MXEC_LOCATE_CLEAN;
    if (r->shard_min == r->shard_max && r->shard_min < 256) {
        if (shard) *shard = r->shard_min;
        return MXEC_LOCATE_ONE;
    }
    return MXEC_LOCATE_MANY;
}

}  // namespace mxec
