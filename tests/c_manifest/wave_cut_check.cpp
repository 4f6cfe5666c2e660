// CPU unit test of the host pipeline's wave cutter
// (maxio_amd/csrc/wave_cut.hpp): consecutive objects share a wave while
// their device images fit the pool allowance, an object larger than the
// allowance is a wave of its own, every object's pool offset is the running
// sum within its wave, and each wave's pool and descriptor-arena needs are
// the sums of its objects'.  The GPU tests only ever see one wave (the
// allowance is 96 GiB), so the multi-wave cases live here.  The expected
// cuts come from a plain restatement of the loop the PUT and the GET each
// carried before they shared this function.
#include <cstdio>
#include <random>

#include "../../maxio_amd/csrc/wave_cut.hpp"

using namespace mxec;

static int fails = 0;
#define CHECK(c)                                                      \
    do {                                                              \
        if (!(c)) {                                                   \
            std::fprintf(stderr, "FAIL line %d: %s\n", __LINE__, #c); \
            ++fails;                                                  \
        }                                                             \
    } while (0)

struct Obj {
    int k, m;
    uint64_t S;
};
static uint64_t rup(uint64_t x, uint64_t a) { return (x + a - 1) / a * a; }
static uint64_t bytes(const Obj& o) { return uint64_t(o.k + o.m) * rup(o.S, 256); }
// The two descriptor formulas (pipeline_put.cpp HostObj, pipeline_get.cpp RecObj).
static uint64_t put_desc(const Obj& o) { return uint64_t(o.k + o.m) * 48 + 256; }
static uint64_t get_desc(const Obj& o) { return uint64_t(o.k + o.m) * 96 + 512 + (o.S / 8192 + 2) * 32; }

// The earlier loop, as it stood in both run() and run_rec(): returns, per
// wave, (begin, end, pool need, arena reserve) and fills pool_off.
struct Old {
    size_t o, e;
    uint64_t need, reserve;
};
static std::vector<Old> old_loop(const std::vector<Obj>& objs, bool get, uint64_t cap, std::vector<uint64_t>& pool_off) {
    std::vector<Old> out;
    pool_off.assign(objs.size(), 0);
    size_t o = 0;
    while (o < objs.size()) {
        uint64_t need = 0, desc = 1 << 20;
        size_t e = o;
        while (e < objs.size() && (e == o || need + bytes(objs[e]) <= cap)) {
            pool_off[e] = need;
            need += bytes(objs[e]);
            desc += get ? get_desc(objs[e]) : put_desc(objs[e]);
            ++e;
        }
        out.push_back(Old{o, e, need, desc * 2});
        o = e;
    }
    return out;
}

static WaveCuts cut(const std::vector<Obj>& objs, bool get, uint64_t cap) {
    std::vector<uint64_t> pool, desc;
    for (const Obj& o : objs) {
        pool.push_back(bytes(o));
        desc.push_back(get ? get_desc(o) : put_desc(o));
    }
    return cut_waves(pool, desc, cap);
}

// Same cuts as the old loop, and the properties that define a cut.
static void check(const std::vector<Obj>& objs, uint64_t cap) {
    for (bool get : {false, true}) {
        std::vector<uint64_t> off;
        const std::vector<Old> want = old_loop(objs, get, cap, off);
        const WaveCuts c = cut(objs, get, cap);
        CHECK(c.waves.size() == want.size());
        CHECK(c.pool_off == off);
        size_t next = 0;  // every object in exactly one wave, in order
        for (size_t w = 0; w < c.waves.size(); ++w) {
            const WaveCuts::Wave& v = c.waves[w];
            CHECK(v.begin == next && v.end > v.begin && v.end <= objs.size());
            next = v.end;
            if (w < want.size())
                CHECK(v.begin == want[w].o && v.end == want[w].e && v.pool == want[w].need &&
                      v.arena == want[w].reserve);
            uint64_t sum = 0;
            for (size_t o = v.begin; o < v.end && o < objs.size(); ++o) {
                CHECK(c.pool_off[o] == sum);  // running sums
                sum += bytes(objs[o]);
            }
            CHECK(v.pool == sum);
            CHECK(sum <= cap || v.end - v.begin == 1);  // over the cap only alone
            // the next object would not have fitted
            if (v.end < objs.size()) CHECK(sum + bytes(objs[v.end]) > cap);
        }
        CHECK(next == objs.size());
    }
}

int main() {
    const uint64_t MiB = uint64_t(1) << 20;
    const Obj a{4, 2, 10 * MiB};  // 60 MiB
    // an empty list: no wave
    {
        const WaveCuts c = cut({}, false, 64 * MiB);
        CHECK(c.waves.empty() && c.pool_off.empty());
        check({}, 64 * MiB);
    }
    // one wave when everything fits; its arena need is twice (1 MiB + the tables)
    {
        const WaveCuts c = cut({a, a, a}, false, 96 * 1024 * MiB);
        CHECK(c.waves.size() == 1 && c.waves[0].begin == 0 && c.waves[0].end == 3);
        CHECK(c.waves[0].pool == 180 * MiB && c.waves[0].arena == 2 * (MiB + 3 * (6 * 48 + 256)));
        CHECK(c.pool_off[0] == 0 && c.pool_off[1] == 60 * MiB && c.pool_off[2] == 120 * MiB);
        const WaveCuts g = cut({a}, true, 96 * 1024 * MiB);
        CHECK(g.waves[0].arena == 2 * (MiB + 6 * 96 + 512 + (10 * MiB / 8192 + 2) * 32));
    }
    // an exact fit stays one wave; one byte less of cap (the second object one byte over) cuts
    {
        const WaveCuts fit = cut({a, a}, false, 120 * MiB);
        CHECK(fit.waves.size() == 1 && fit.waves[0].pool == 120 * MiB);
        const WaveCuts over = cut({a, a}, false, 120 * MiB - 1);
        CHECK(over.waves.size() == 2 && over.waves[1].begin == 1 && over.pool_off[1] == 0);
        const Obj b{4, 2, 10 * MiB + 1};  // one byte over: a whole 256-byte slot step per shard
        const WaveCuts odd = cut({a, b}, false, 120 * MiB);
        CHECK(odd.waves.size() == 2 && odd.waves[1].pool == 6 * (10 * MiB + 256));
        check({a, a}, 120 * MiB);
        check({a, a}, 120 * MiB - 1);
        check({a, b}, 120 * MiB);
    }
    // an object larger than the cap is alone in its wave (the e == o rule), wherever it stands
    {
        const Obj big{8, 4, 64 * MiB};  // 768 MiB
        for (const std::vector<Obj>& v :
             std::vector<std::vector<Obj>>{{big}, {big, a, a}, {a, big, a}, {a, a, big}, {big, big}}) {
            const WaveCuts c = cut(v, true, 128 * MiB);
            for (const auto& w : c.waves)
                if (w.pool > 128 * MiB) CHECK(w.end - w.begin == 1 && v[w.begin].S == big.S);
            check(v, 128 * MiB);
        }
        CHECK(cut({a, big, a}, true, 128 * MiB).waves.size() == 3);
        check({a, a}, 1);  // every object over a 1-byte cap
        CHECK(cut({a, a}, false, 1).waves.size() == 2);
    }
    // mixed (k, m, S)
    check({{4, 2, 65536}, {8, 4, MiB}, {10, 4, 4096 + 16}, {4, 2, 17}, {1, 2, 3000}, {3, 5, 100}}, 2 * MiB);
    check({{4, 2, 65536}, {8, 4, MiB}, {10, 4, 4096 + 16}, {4, 2, 17}, {1, 2, 3000}, {3, 5, 100}}, 13 * MiB);
    // seeded random lists
    std::mt19937_64 rng(0x77617665);
    for (int t = 0; t < 400; ++t) {
        std::vector<Obj> v(size_t(rng() % 40));
        for (Obj& o : v) {
            o.k = 1 + int(rng() % 12);
            o.m = 1 + int(rng() % 6);
            o.S = 1 + rng() % (rng() % 4 ? 64 * 1024 : 8 * MiB);
        }
        const uint64_t caps[] = {1, 300 * 1024, 4 * MiB, 64 * MiB, uint64_t(96) << 30};
        check(v, caps[rng() % 5]);
    }
    if (fails) return 1;
    std::printf("wave cut ok\n");
    return 0;
}
