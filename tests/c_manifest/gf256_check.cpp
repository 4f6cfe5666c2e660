// CPU unit test of the host GF(2^8) algebra behind the RS kernels
// (maxio_amd/csrc/gf256.cpp) against the oracle (oracle/rs_oracle.c), at the
// wide shapes of tests/test_wide_stripes_gpu.py: a GPU failure there is the
// kernel's if this passes, the host algebra's if it does not.
//
// * coef_entry: for all 256 c and all 256 x, T0[x & 7] ^ T1[(x >> 3) & 7] ^
//   T2[x >> 6], each read out of the packed dwords as one of the kernel's three
//   v_perm selects reads it, equals the oracle's gf_mul(c, x);
// * rs_matrix(k, m) equals the oracle's matrix for every wide shape, for the
//   256-shard shapes (252, 4) and (255, 1), and for 200 seeded (k, m) with
//   k + m <= 256;
// * DecodeCache::get over 300 seeded erasure patterns of those shapes, 1..m
//   missing, data_only both ways: valid is the first k present, missing is data
//   before parity, rows applied on the CPU to random 64-byte shards gives the
//   oracle's reconstruct (and the original bytes), the table is coef_tables of
//   the rows; fewer than k present is null; asking again is the same plan.
//
// Built from this file, gf256.cpp and the oracle's C sources (see
// tests/test_host_planning.py).
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <random>
#include <utility>
#include <vector>

#include "../../maxio_amd/csrc/gf256.hpp"
#include "../../oracle/oracle.h"

using namespace mxec;

static int fails = 0;
#define CHECK(c)                                                      \
    do {                                                              \
        if (!(c)) {                                                   \
            std::fprintf(stderr, "FAIL line %d: %s\n", __LINE__, #c); \
            ++fails;                                                  \
        }                                                             \
    } while (0)

// tests/test_wide_stripes_gpu.py WIDE, then the two shapes of 256 shards that
// only the reconstructs accept.
static const int kWide[][2] = {{127, 2}, {129, 3}, {130, 4}, {250, 5}, {200, 8}, {247, 8},
                               {251, 4}, {254, 1}, {243, 12}, {252, 4}, {255, 1}};
constexpr int kNWide = int(sizeof kWide / sizeof kWide[0]);
constexpr size_t kBytes = 64;

// v_perm_b32 with a selector byte below 8: byte `sel` of the 8 bytes {hi, lo}.
static uint8_t perm_byte(uint32_t lo, uint32_t hi, unsigned sel) {
    return uint8_t((sel < 4 ? lo : hi) >> (8 * (sel & 3)));
}

static void check_coef_entry() {
    for (int c = 0; c < 256; ++c) {
        uint32_t t[kCoefDwords];
        coef_entry(uint8_t(c), t);
        CHECK(t[5] == 0 && t[6] == 0 && t[7] == 0);
        for (int x = 0; x < 256; ++x) {
            const uint8_t got = perm_byte(t[0], t[1], unsigned(x) & 7) ^ perm_byte(t[2], t[3], (unsigned(x) >> 3) & 7) ^
                                perm_byte(t[4], t[5], unsigned(x) >> 6);
            if (got != orc_gf_mul(uint8_t(c), uint8_t(x))) {
                std::fprintf(stderr, "FAIL coef_entry c=%d x=%d\n", c, x);
                ++fails;
            }
        }
    }
}

static std::vector<uint8_t> oracle_matrix(int k, int m) {
    std::vector<uint8_t> want(size_t(k + m) * size_t(k));
    CHECK(orc_rs_matrix(k, m, want.data()) == ORC_OK);
    return want;
}

static void check_matrix(int k, int m) {
    const std::vector<uint8_t> want = oracle_matrix(k, m);
    auto got = rs_matrix(k, m);
    CHECK(got && got->rows == k + m && got->cols == k);
    if (!got || got->v != want) {
        std::fprintf(stderr, "FAIL rs_matrix(%d, %d)\n", k, m);
        ++fails;
    }
    CHECK(rs_matrix(k, m) == got);  // cached per (k, m)
}

// One erasure pattern: `lost` shard indices of (k, m), checked as the header says.
static void check_pattern(DecodeCache& cache, std::mt19937_64& rng, int k, int m, const std::vector<int>& lost,
                          bool data_only) {
    const int total = k + m;
    const size_t n_shards = size_t(total);
    std::vector<std::vector<uint8_t>> orig(n_shards, std::vector<uint8_t>(kBytes));
    std::vector<uint8_t*> ptr(static_cast<size_t>(total));
    for (int i = 0; i < total; ++i) {
        if (i < k)
            for (uint8_t& b : orig[size_t(i)]) b = uint8_t(rng());
        ptr[size_t(i)] = orig[size_t(i)].data();
    }
    CHECK(orc_rs_encode(k, m, kBytes, ptr.data()) == ORC_OK);

    std::vector<uint8_t> present(size_t(total), 1);
    for (int i : lost) present[size_t(i)] = 0;
    auto plan = cache.get(k, m, present.data(), data_only);
    CHECK(plan != nullptr);
    if (!plan) return;
    CHECK(cache.get(k, m, present.data(), data_only) == plan);
    CHECK(plan->k == k && plan->m == m);

    std::vector<int> valid, missing;
    for (int i = 0; i < total && int(valid.size()) < k; ++i)
        if (present[size_t(i)]) valid.push_back(i);
    for (int i = 0; i < k; ++i)
        if (!present[size_t(i)]) missing.push_back(i);
    for (int i = k; i < total && !data_only; ++i)
        if (!present[size_t(i)]) missing.push_back(i);
    CHECK(plan->valid == valid);
    CHECK(plan->missing == missing);
    CHECK(plan->rows.rows == int(missing.size()) && plan->rows.cols == k);
    CHECK(plan->table == coef_tables(plan->rows));
    CHECK(plan->table.size() == missing.size() * size_t(k) * kCoefDwords);
    if (plan->valid != valid || plan->missing != missing || plan->rows.rows != int(missing.size())) return;

    // The oracle's reconstruct over the same shards, the lost ones scribbled on.
    std::vector<std::vector<uint8_t>> work = orig;
    std::vector<uint8_t> opresent = present;
    for (int i = 0; i < total; ++i) {
        if (!present[size_t(i)]) std::fill(work[size_t(i)].begin(), work[size_t(i)].end(), uint8_t(0xA5));
        ptr[size_t(i)] = work[size_t(i)].data();
    }
    CHECK(orc_rs_reconstruct(k, m, kBytes, ptr.data(), opresent.data(), data_only ? 1 : 0) == ORC_OK);
    for (size_t t = 0; t < missing.size(); ++t) {
        uint8_t out[kBytes] = {0};
        for (int c = 0; c < k; ++c) {
            const uint8_t coef = plan->rows.at(int(t), c);
            const uint8_t* in = orig[size_t(valid[size_t(c)])].data();
            for (size_t b = 0; b < kBytes; ++b) out[b] ^= orc_gf_mul(coef, in[b]);
        }
        const size_t s = size_t(missing[t]);
        const bool same = std::memcmp(out, work[s].data(), kBytes) == 0 && std::memcmp(out, orig[s].data(), kBytes) == 0;
        if (!same) {
            std::fprintf(stderr, "FAIL rows (%d, %d) data_only=%d shard %zu of %zu lost\n", k, m, int(data_only), s,
                         lost.size());
            ++fails;
        }
    }
}

static std::vector<int> draw_lost(std::mt19937_64& rng, int total, int n) {
    std::vector<int> all(static_cast<size_t>(total));
    for (int i = 0; i < total; ++i) all[size_t(i)] = i;
    std::shuffle(all.begin(), all.end(), rng);
    all.resize(size_t(n));
    return all;
}

int main() {
    check_coef_entry();

    std::mt19937_64 rng(0x67663235);
    std::vector<std::pair<int, int>> shapes;
    for (int i = 0; i < kNWide; ++i) shapes.push_back({kWide[i][0], kWide[i][1]});
    // 200 seeded shapes: the inversion is cubic in k, so seven in eight are
    // drawn below k = 64 and the rest up to 255; every tenth fills all 256 shards.
    for (int i = 0; i < 200; ++i) {
        const int k = 1 + int(rng() % (i % 8 == 7 ? 255 : 64));
        const int room = 256 - k;
        const int m = i % 10 == 9 ? room : 1 + int(rng() % uint64_t(std::min(room, 16)));
        shapes.push_back({k, m});
    }
    for (auto& s : shapes) {
        CHECK(s.first >= 1 && s.second >= 1 && s.first + s.second <= 256);
        check_matrix(s.first, s.second);
    }

    // 300 patterns: each wide shape three times, with shard 0, the last data
    // shard, index 128 where there is one and the last shard (255 at 256 shards)
    // among the lost; then seeded shapes in turn.
    DecodeCache cache;
    int n_patterns = 0;
    for (int i = 0; i < kNWide; ++i) {
        const int k = kWide[i][0], m = kWide[i][1], total = k + m;
        check_pattern(cache, rng, k, m, {k - 1}, true);
        std::vector<int> lost = {total - 1};
        if (m >= 2) lost.push_back(0);
        if (m >= 3 && k > 128) lost.push_back(128);
        check_pattern(cache, rng, k, m, lost, false);
        check_pattern(cache, rng, k, m, draw_lost(rng, total, m), (i & 1) != 0);
        n_patterns += 3;
        // Fewer than k present: no plan.
        std::vector<uint8_t> present(size_t(total), 1);
        for (int e : draw_lost(rng, total, m + 1)) present[size_t(e)] = 0;
        CHECK(cache.get(k, m, present.data(), false) == nullptr);
        CHECK(cache.get(k, m, present.data(), true) == nullptr);
    }
    for (size_t at = size_t(kNWide); n_patterns < 300; ++n_patterns, ++at) {
        if (at == shapes.size()) at = size_t(kNWide);
        const int k = shapes[at].first, m = shapes[at].second;
        const int n = 1 + int(rng() % uint64_t(m));
        check_pattern(cache, rng, k, m, draw_lost(rng, k + m, n), (rng() & 1) != 0);
    }
    CHECK(n_patterns == 300);

    if (fails) {
        std::fprintf(stderr, "%d failures\n", fails);
        return 1;
    }
    std::printf("gf256 ok\n");
    return 0;
}
