// scrub_plan.hpp — what a scrub's findings amount to (mxec_scrub_object,
// storage_scrub.cpp): shard states -> damaged count -> whether a heal may run ->
// verdict.
//
// Host-only (no HIP, no I/O): built into libmaxio_ec.so and, on its own with
// -fsanitize=address,undefined, into the CPU test harness
// tests/c_manifest/scrub_plan_check.cpp.
#pragma once

#include <cstdint>

#include "../../include/maxio_ec.h"

namespace mxec {

// Shards of the first `total` states that are not MXEC_SHARD_OK.
inline uint32_t scrub_damaged(const uint8_t* state, uint32_t total) {
    uint32_t n = 0;
    for (uint32_t i = 0; i < total; ++i) n += (state[i] & ~MXEC_SHARD_HEALED) != MXEC_SHARD_OK;
    return n;
}

// A heal rebuilds every damaged shard from the others: at least one to
// rebuild, at most m (k good shards must remain).
inline bool scrub_can_heal(uint32_t n_damaged, uint32_t m) { return n_damaged >= 1 && n_damaged <= m; }

// parity_consistent: 1 / 0 / -1 (not checked).  heal: MXEC_SCRUB_HEAL was
// asked.  rebuilt_ok: the heal ran and every rebuilt shard's digest equals
// the manifest's (so the shards were written).
//  * nothing damaged: CLEAN, unless the parity check failed -- some shard
//    differs from what the others encode, though no check named one (PARITY
//    mode alone; or digests that match a manifest written over bad parity):
//    DAMAGED, and nothing a heal could rebuild;
//  * damaged, no heal asked: DAMAGED;
//  * heal asked: HEALED if it ran and was written, else UNRECOVERABLE.
inline uint32_t scrub_verdict(uint32_t n_damaged, uint32_t m, int32_t parity_consistent, bool heal,
                              bool rebuilt_ok) {
    if (n_damaged == 0) return parity_consistent == 0 ? MXEC_SCRUB_DAMAGED : MXEC_SCRUB_CLEAN;
    if (!heal) return MXEC_SCRUB_DAMAGED;
    return scrub_can_heal(n_damaged, m) && rebuilt_ok ? MXEC_SCRUB_HEALED : MXEC_SCRUB_UNRECOVERABLE;
}

}  // namespace mxec
