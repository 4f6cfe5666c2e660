// CPU unit test of the reconstructs' decode table builder
// (maxio_amd/csrc/decode_tables.hpp): a few hundred seeded batches against a
// plain per-object restatement of its rules.  The builder reads only `valid`
// and `missing` of a plan, so the plans are made by hand; shard addresses are
// made up and never dereferenced.
//
// Mixed per batch: both shard-location forms (pointer table, base + i *
// stride), (k, m) from (1, 2) to (10, 4), 0..m missing shards, objects with no
// plan and with nothing missing, shard sizes from 1 byte up with per-shard
// lengths that are full, short and zero, and windows whose off lies before,
// inside and past a short shard with pw smaller and larger than what remains.
#include <cstdio>
#include <memory>
#include <random>
#include <set>

#include "../../maxio_amd/csrc/decode_tables.hpp"

using namespace mxec;

static int fails = 0;
#define CHECK(c)                                                      \
    do {                                                              \
        if (!(c)) {                                                   \
            std::fprintf(stderr, "FAIL line %d: %s\n", __LINE__, #c); \
            ++fails;                                                  \
        }                                                             \
    } while (0)

// One object as the check keeps it; the DecodeItem points into it.
struct Obj {
    int k, m;
    uint64_t S;
    std::vector<uint64_t> len;
    std::vector<uint8_t*> table;  // pointer-table form, else empty
    uint8_t* base = nullptr;      // base + i * stride form
    uint64_t stride = 0;
    std::unique_ptr<DecodePlan> plan;  // null: short of k shards
    uint32_t coef = 0;                 // unique per object: how the check finds it again
    uint8_t* addr(int i) const { return table.empty() ? base + uint64_t(i) * stride : table[size_t(i)]; }
};

static const int kShapes[][2] = {{1, 2}, {2, 1}, {2, 2}, {3, 3}, {4, 2}, {6, 3}, {8, 4}, {10, 4}};
static const uint64_t kSizes[] = {1, 15, 64, 4097, 65536 + 16};

static Obj make_obj(std::mt19937_64& rng, uint32_t id) {
    auto pick = [&rng](uint64_t n) { return rng() % n; };
    Obj ob;
    const int* km = kShapes[pick(sizeof kShapes / sizeof kShapes[0])];
    ob.k = km[0], ob.m = km[1];
    ob.S = kSizes[pick(sizeof kSizes / sizeof kSizes[0])];
    ob.coef = 1000 + id * 8;
    const int total = ob.k + ob.m;
    for (int i = 0; i < total; ++i) {
        const uint64_t c = pick(4);  // full, zero, short, one short of full
        ob.len.push_back(c == 0 ? ob.S : c == 1 ? 0 : c == 2 ? pick(ob.S + 1) : ob.S - 1);
    }
    uint8_t* const at = reinterpret_cast<uint8_t*>(uintptr_t(0x7000000000) + uintptr_t(id) * 0x10000000);
    if (pick(2)) {
        for (int i = 0; i < total; ++i) ob.table.push_back(at + pick(4096) * 256 + uint64_t(i));  // scattered, any alignment
    } else {
        ob.base = at + pick(16);
        ob.stride = (ob.S + 255) / 256 * 256 + pick(2) * 256;
    }
    // 0..m shards absent, sometimes more (no plan); data_only rebuilds the absent data shards only.
    const int absent = int(pick(uint64_t(ob.m) + 2));
    if (absent > ob.m) return ob;
    std::set<int> gone;
    while (int(gone.size()) < absent) gone.insert(int(pick(uint64_t(total))));
    const bool data_only = pick(3) == 0;
    ob.plan.reset(new DecodePlan);
    ob.plan->k = ob.k, ob.plan->m = ob.m;
    for (int i = 0; i < total; ++i) {
        if (!gone.count(i) && int(ob.plan->valid.size()) < ob.k) ob.plan->valid.push_back(i);
        if (gone.count(i) && (i < ob.k || !data_only)) ob.plan->missing.push_back(i);
    }
    return ob;
}

// One batch through the builder (tables kept by the caller across batches, as
// a re-run of a launch does), checked object by object.
static void run_batch(std::mt19937_64& rng, DecodeTables& tables, size_t n, bool windowed) {
    std::vector<Obj> objs;
    for (size_t o = 0; o < n; ++o) objs.push_back(make_obj(rng, uint32_t(o)));
    uint64_t off = 0, pw = ~uint64_t(0);
    if (windowed && n) {
        // Around one object's shard: before, inside and past a short shard's
        // end, at and past the shard size; pw under and over what remains.
        const Obj& ref = objs[rng() % n];
        const uint64_t L = ref.len[rng() % ref.len.size()];
        const uint64_t offs[] = {0, L / 2, L ? L - 1 : 0, L, L + 1, ref.S - 1, ref.S, ref.S + 5};
        const uint64_t pws[] = {1, 7, 64, ref.S / 2 + 1, ref.S, ref.S + 9, ~uint64_t(0)};
        off = offs[rng() % 8];
        pw = pws[rng() % 7];
    }
    std::vector<DecodeItem> items;
    size_t want_objs = 0, want_in = 0, want_out = 0;
    for (const Obj& ob : objs) {
        DecodeItem it{ob.k, ob.m, ob.S, ob.len.data(), nullptr, ob.table.empty() ? nullptr : ob.table.data(), ob.base, ob.stride};
        // the caller's rule: an object that ends before the window has no plan
        it.plan = ob.S > off ? ob.plan.get() : nullptr;
        it.coef_off = ob.coef;
        items.push_back(it);
        if (it.plan && !it.plan->missing.empty()) ++want_objs, want_in += size_t(ob.k), want_out += it.plan->missing.size();
    }
    const auto groups = off == 0 && pw == ~uint64_t(0) && (rng() & 1) ? tables.build(items) : tables.build(items, off, pw);
    CHECK(tables.in.size() == want_in && tables.in_len.size() == want_in);
    CHECK(tables.out.size() == want_out && tables.out_len.size() == want_out);
    size_t got_objs = 0;
    for (const auto& g : groups) {
        CHECK(g.first > 0 && !g.second.empty());
        got_objs += g.second.size();
    }
    CHECK(got_objs == want_objs);
    if (want_objs == 0) CHECK(groups.empty());
    std::set<const void*> in_rows, out_rows;  // no two objects share table entries
    for (size_t o = 0; o < n; ++o) {
        const Obj& ob = objs[o];
        const DecodePlan* p = items[o].plan;
        size_t met = 0;
        const RsMixedObject* got = nullptr;
        int key = 0;
        for (const auto& g : groups)
            for (const RsMixedObject& x : g.second)
                if (x.o.coef_off == ob.coef) ++met, got = &x, key = g.first;
        if (!p || p->missing.empty()) {
            CHECK(met == 0);  // contributes nothing
            continue;
        }
        CHECK(met == 1);  // exactly once ...
        if (met != 1) continue;
        const int r = int(p->missing.size());
        CHECK(key == r);  // ... under its number of rebuilt shards
        CHECK(got->k == ob.k && got->shard_size == std::min(pw, ob.S - off) && got->shard_size >= 1);
        const RsObject& x = got->o;
        CHECK(!x.first_bad && !x.locate && !x.seed);
        // Its rows lie inside the tables as they stand now.
        const bool inside = x.in >= tables.in.data() && x.in + ob.k <= tables.in.data() + tables.in.size() &&
                            x.in_len >= tables.in_len.data() && x.in_len + ob.k <= tables.in_len.data() + tables.in_len.size() &&
                            x.out >= tables.out.data() && x.out + r <= tables.out.data() + tables.out.size() &&
                            x.out_len >= tables.out_len.data() && x.out_len + r <= tables.out_len.data() + tables.out_len.size();
        CHECK(inside);
        CHECK(x.in - tables.in.data() == x.in_len - tables.in_len.data());
        CHECK(x.out - tables.out.data() == x.out_len - tables.out_len.data());
        CHECK(in_rows.insert(x.in).second && out_rows.insert(x.out).second);
        auto window = [&](int i) { return ob.len[size_t(i)] > off ? std::min(pw, ob.len[size_t(i)] - off) : uint64_t(0); };
        for (int v = 0; v < ob.k; ++v) {  // read through the RsObject: ASan sees a dangling row
            CHECK(x.in[v] == ob.addr(p->valid[size_t(v)]) + off);
            CHECK(x.in_len[v] == window(p->valid[size_t(v)]) && x.in_len[v] <= got->shard_size);
        }
        for (int e = 0; e < r; ++e) {
            CHECK(x.out[e] == ob.addr(p->missing[size_t(e)]) + off);
            CHECK(x.out_len[e] == window(p->missing[size_t(e)]) && x.out_len[e] <= got->shard_size);
        }
    }
}

int main() {
    DecodeTables tables;
    CHECK(tables.build({}).empty() && tables.in.empty() && tables.out.empty());  // an empty batch
    CHECK(tables.build({}, 5, 3).empty());
    for (uint64_t seed = 1; seed <= 400; ++seed) {
        std::mt19937_64 rng(seed);
        // the same tables batch after batch; every fourth batch through fresh ones
        DecodeTables fresh;
        run_batch(rng, seed % 4 ? tables : fresh, size_t(rng() % 14), seed % 3 != 0);
    }
    {  // objects with no plan or nothing missing only: an empty map, empty tables
        Obj a, b;
        a.k = b.k = 4, a.m = b.m = 2, a.S = b.S = 100;
        a.len.assign(6, 100), b.len.assign(6, 100);
        a.base = b.base = reinterpret_cast<uint8_t*>(uintptr_t(0x7000000000));
        a.stride = b.stride = 256;
        b.plan.reset(new DecodePlan);
        b.plan->valid = {0, 1, 2, 3};
        std::vector<DecodeItem> items;
        for (const Obj* ob : {&a, &b}) {
            items.push_back(DecodeItem{ob->k, ob->m, ob->S, ob->len.data(), nullptr, nullptr, ob->base, ob->stride});
            items.back().plan = ob->plan.get();
        }
        CHECK(tables.build(items).empty() && tables.in.empty() && tables.out_len.empty());
    }
    if (fails) return 1;
    std::printf("decode tables ok\n");
    return 0;
}
