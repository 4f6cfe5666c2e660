// wave_cut.hpp -- the waves of a host-batch call's share of one device
// (pipeline.hpp PipeCall::run_waves).  Header-only and free of HIP so
// tests/c_manifest/wave_cut_check.cpp can test it on the CPU.
//
// A wave is a run of consecutive objects whose device images (k + m shard
// slots each) fit the lane's pool together; an object larger than the pool
// allowance is a wave of its own.  Each object's image starts where the
// previous one of its wave ended.
#pragma once

#include <cstddef>
#include <cstdint>
#include <vector>

namespace mxec {

struct WaveCuts {
    struct Wave {
        size_t begin, end;  // objects [begin, end)
        uint64_t pool;      // bytes of pool the wave needs
        uint64_t arena;     // bytes of descriptor arena to reserve for it
    };
    std::vector<Wave> waves;
    std::vector<uint64_t> pool_off;  // per object, within its wave's pool
};

// pool[o] / desc[o]: object o's device image and its share of the wave's
// descriptor tables, in bytes; cap: pool bytes per wave.
inline WaveCuts cut_waves(const std::vector<uint64_t>& pool, const std::vector<uint64_t>& desc, uint64_t cap) {
    WaveCuts c;
    c.pool_off.resize(pool.size());
    for (size_t o = 0; o < pool.size();) {
        uint64_t need = 0, tables = 1 << 20;
        size_t e = o;
        while (e < pool.size() && (e == o || need + pool[e] <= cap)) {
            c.pool_off[e] = need;
            need += pool[e];
            tables += desc[e];
            ++e;
        }
        c.waves.push_back(WaveCuts::Wave{o, e, need, tables * 2});
        o = e;
    }
    return c;
}

}  // namespace mxec
