// CPU unit test of the Reed-Solomon launch planner
// (maxio_amd/csrc/rs_plan.hpp): the descriptor tables of the uniform,
// unaligned, grouped, verify / locate and multi-r launches, and which
// launches a mixed call becomes.  Pointer values are made up and never
// dereferenced; the tile sizes are the kernels' (256 lanes x 16 bytes x 4
// vectors for r <= 4, x 2 for r in 5..8).
//
// Every table image is checked twice: section by section against a plain
// construction from RsArgs' documented layout (rs_args.hpp), and by walking
// the launch as the kernel does -- tile / tiles_per_obj, the edge list, or
// the tile record -- asserting that every (object, tile) is met exactly once
// and lands on that object's pointers, clamped lengths, coefficient offset,
// result pointer and locate table.
#include <cstdio>
#include <cstring>
#include <set>

#include "../../maxio_amd/csrc/rs_plan.hpp"

using namespace mxec;

static int fails = 0;
#define CHECK(c)                                                      \
    do {                                                              \
        if (!(c)) {                                                   \
            std::fprintf(stderr, "FAIL line %d: %s\n", __LINE__, #c); \
            ++fails;                                                  \
        }                                                             \
    } while (0)

static uint64_t tile_of(int r) {
    CHECK(r >= 1 && r <= 8);  // the planner never asks for more rows
    return r <= 4 ? 16384 : 8192;
}
static uint64_t r16(uint64_t x) { return (x + 15) & ~uint64_t(15); }
static uint64_t tiles(uint64_t S, uint64_t tile) { return (S + tile - 1) / tile; }

// One object with made-up, 16-byte aligned pointers; input 0 is empty, input
// 1 and output 0 claim more than the shard size (clamped).
static uint64_t next_addr = 0x7000000000;
struct Obj {
    int k, r;
    uint64_t S;
    std::vector<const uint8_t*> in;
    std::vector<uint8_t*> out;
    std::vector<uint64_t> in_len, out_len;
    uint32_t coef;
    RsPass pass;
    void* res = nullptr;  // its first_bad entries or its LocateRec
    Obj(int k_, int r_, uint64_t S_, RsPass pass_ = kRsStore) : k(k_), r(r_), S(S_), pass(pass_) {
        auto addr = [] { return reinterpret_cast<uint8_t*>(next_addr += 0x1000); };
        for (int j = 0; j < k; ++j) {
            in.push_back(addr());
            in_len.push_back(j == 0 ? 0 : j == 1 ? S + 7 : S);
        }
        for (int i = 0; i < r; ++i) {
            out.push_back(addr());
            out_len.push_back(i == 0 ? S + 1 : S / 2);
        }
        coef = uint32_t(next_addr >> 8);
        if (pass != kRsStore) res = addr();
    }
    RsObject view() const {
        RsObject o{in.data(), in_len.data(), out.data(), out_len.data(), coef};
        if (pass == kRsLocate) o.locate = res;
        if (pass == kRsVerify) o.first_bad = static_cast<uint64_t*>(res);
        return o;
    }
};

template <class T, class U>
static bool same(const T* got, const std::vector<U>& want) {
    static_assert(sizeof(T) == sizeof(U), "entry size");
    return want.empty() || std::memcmp(got, want.data(), sizeof(U) * want.size()) == 0;
}

// A made-up (k, r) locate table: enough to tell which one an offset names.
static int fake_table(int k, int r, uint8_t* out) {
    std::memset(out, 0xA5, locate_table_bytes(r));
    out[0] = uint8_t(k);
    out[1] = uint8_t(r);
    return 0;
}

// One launch as the check restates it.
struct Launch {
    std::vector<const Obj*> objs;
    uint32_t stride;  // output entries per object
    uint64_t tile;
    bool tiled, multi, aligned;
    RsPass pass;
};

// The sections, built plainly from the layout rs_args.hpp documents.
static void check_sections(const Launch& l, const RsArgs& a) {
    const size_t n = l.objs.size();
    std::vector<const uint8_t*> in;
    std::vector<uint8_t*> out(n * l.stride, nullptr);
    std::vector<uint64_t> il, ol(n * l.stride, 0), ed;
    std::vector<uint32_t> co;
    std::vector<RsTileRec> tr;
    std::vector<void*> res;
    for (size_t o = 0; o < n; ++o) {
        const Obj& ob = *l.objs[o];
        const uint32_t in0 = uint32_t(in.size());
        for (int j = 0; j < ob.k; ++j) {
            in.push_back(ob.in[size_t(j)]);
            il.push_back(std::min(ob.in_len[size_t(j)], ob.S));
        }
        for (int i = 0; i < ob.r; ++i) {
            out[o * l.stride + size_t(i)] = ob.out[size_t(i)];
            ol[o * l.stride + size_t(i)] = std::min(ob.out_len[size_t(i)], ob.S);
        }
        co.push_back(ob.coef);
        res.push_back(ob.res);
        for (uint64_t t = 0; t < tiles(ob.S, l.tile); ++t) {
            if (l.tiled) tr.push_back(RsTileRec{uint32_t(o), uint32_t(ob.k) | (l.multi ? uint32_t(ob.r) << 16 : 0u), in0, uint32_t(t)});
            else if (!l.aligned) ed.push_back(uint64_t(o) << 32 | t);
        }
    }
    CHECK(a.n_obj == n && a.r_total == l.stride && a.r == l.stride && a.row0 == 0);
    CHECK(a.aligned == (l.aligned ? 1u : 0u) && a.multi == (l.multi ? 1u : 0u));
    CHECK(same(a.in_ptrs, in) && same(a.out_ptrs, out) && same(a.in_len, il) && same(a.out_len, ol));
    CHECK(same(a.coef_off, co));
    if (l.tiled) {
        CHECK(a.tiles && a.n_tiles == tr.size() && same(a.tiles, tr) && !a.edge_list && a.n_edge == 0);
    } else {
        CHECK(!a.tiles && a.n_tiles == 0 && a.n_edge == ed.size() && same(a.edge_list, ed));
        CHECK(a.edge_tile_bytes == l.tile);
    }
    CHECK((a.first_bad != nullptr) == (l.pass == kRsVerify) && (a.locate != nullptr) == (l.pass == kRsLocate));
    if (l.pass == kRsVerify) CHECK(same(a.first_bad, res));
    if (l.pass == kRsLocate) CHECK(same(a.locate, res) && a.loc_field && a.loc_tab && a.loc_off);
}

// The launch as the kernel walks it (uniform: a.k and a.shard_size set).
static void check_walk(const Launch& l, const RsArgs& a) {
    std::set<std::pair<uint64_t, uint64_t>> met;
    uint64_t want = 0;
    for (const Obj* ob : l.objs) want += tiles(ob->S, l.tile);
    const uint64_t tpo = l.tiled ? 0 : tiles(a.shard_size, l.tile);
    const uint64_t n_walk = l.tiled ? a.n_tiles : l.aligned ? a.n_obj * tpo : a.n_edge;
    CHECK(n_walk == want);
    for (uint64_t t = 0; t < n_walk; ++t) {
        uint64_t obj, local, in0;
        uint32_t k, r = a.r_total;
        if (l.tiled) {
            const RsTileRec& rec = a.tiles[t];
            obj = rec.obj, local = rec.local, in0 = rec.in0, k = l.multi ? rec.k & 0xFFFFu : rec.k;
            if (l.multi) r = rec.k >> 16 & 0xFFu;
        } else {
            obj = l.aligned ? t / tpo : a.edge_list[t] >> 32;
            local = l.aligned ? t % tpo : a.edge_list[t] & 0xFFFFFFFFu;
            k = a.k, in0 = obj * k;
        }
        CHECK(obj < l.objs.size());
        if (obj >= l.objs.size()) return;
        const Obj& ob = *l.objs[obj];
        CHECK(met.emplace(obj, local).second);  // exactly once ...
        CHECK(local < tiles(ob.S, l.tile));     // ... and within the object
        CHECK(k == uint32_t(ob.k) && r == uint32_t(ob.r));
        if (l.tiled && obj > 0 && local == 0) CHECK(in0 == a.tiles[t - 1].in0 + uint32_t(l.objs[obj - 1]->k));
        for (uint32_t j = 0; j < k && j < uint32_t(ob.k); ++j) {
            CHECK(a.in_ptrs[in0 + j] == ob.in[j]);
            CHECK(a.in_len[in0 + j] == std::min(ob.in_len[j], ob.S) && a.in_len[in0 + j] <= ob.S);
        }
        for (uint32_t i = 0; i < l.stride; ++i) {
            const uint64_t e = obj * l.stride + i;
            if (i < uint32_t(ob.r)) CHECK(a.out_ptrs[e] == ob.out[i] && a.out_len[e] == std::min(ob.out_len[i], ob.S));
            else CHECK(a.out_ptrs[e] == nullptr && a.out_len[e] == 0);  // unused (multi)
        }
        CHECK(a.coef_off[obj] == ob.coef);
        if (l.pass == kRsVerify) CHECK(a.first_bad[obj] == ob.res);
        if (l.pass == kRsLocate) {
            CHECK(a.locate[obj] == ob.res);
            const uint8_t* tab = a.loc_tab + a.loc_off[obj];  // its own (k, r) table
            CHECK(tab[0] == uint8_t(ob.k) && tab[1] == uint8_t(ob.r) && tab[locate_table_bytes(ob.r) - 1] == 0xA5);
        }
    }
    CHECK(met.size() == want);
}

// A uniform launch as run_rs builds it: the table, its image, the args of
// each row block (one table set).  Returns the image's size.
static size_t uniform(const std::vector<Obj>& objs, int k, int r, uint64_t S, RsPass pass = kRsStore) {
    bool aligned = true;
    std::vector<const Obj*> ptrs;
    for (const Obj& ob : objs) {
        aligned = aligned && rs_aligned(ob.view(), k, r);
        ptrs.push_back(&ob);
    }
    const uint64_t tile = r <= 4 ? 16384 : 8192;  // rs_default_variant's: r_total <= 4, or more
    RsTable t = RsTable::uniform(objs.size(), k, r, S, tile, aligned, pass);
    if (pass == kRsLocate) t.locate_k(k);
    RsImage img;
    t.lay(img, true);
    if (pass == kRsLocate) CHECK(rs_locate_fill(img.data(), &t, 1, fake_table) == 0);
    for (const Obj& ob : objs) t.put(img.data(), ob.view(), k, r, S);
    RsArgs a = t.args(img.data());
    a.k = uint32_t(k);
    a.shard_size = S;
    const Launch l{ptrs, uint32_t(r), tile, false, false, aligned, pass};
    check_sections(l, a);
    check_walk(l, a);
    if (!aligned) CHECK(a.n_edge == objs.size() * tiles(S, tile) && a.edge_tile_bytes == tile);
    if (pass == kRsLocate) {
        uint8_t f[kLocateFieldBytes];
        locate_field_tables(f);
        CHECK(!std::memcmp(a.loc_field, f, sizeof f));
        for (size_t o = 0; o < objs.size(); ++o) CHECK(a.loc_off[o] == 0);  // one table
    }
    int blocks = 0, rows = 0;  // ops.cpp's row blocks over the one table set
    for (int row0 = 0; row0 < r; row0 += 8) {
        a.row0 = uint32_t(row0);
        a.r = uint32_t(std::min(8, r - row0));
        CHECK(a.r_total == uint32_t(r) && a.row0 + a.r <= a.r_total);
        rows += int(a.r);
        ++blocks;
    }
    CHECK(rows == r && blocks == (r + 7) / 8);
    // Sections in order, each at its 16-byte-rounded size.
    const uint64_t n = objs.size(), ne = aligned ? 0 : n * tiles(S, tile);
    size_t at = 0;
    auto sec = [&at](size_t off, size_t bytes) {
        CHECK(off == at);
        at += bytes;
    };
    sec(t.o_in, r16(8 * n * k));
    sec(t.o_out, r16(8 * n * r));
    sec(t.o_inlen, r16(8 * n * k));
    sec(t.o_outlen, r16(8 * n * r));
    sec(t.o_coef, r16(4 * n));
    sec(t.o_list, r16(8 * ne));
    if (pass != kRsStore) sec(t.o_res, r16(8 * n));
    if (pass == kRsLocate) {
        sec(t.o_lf, kLocateFieldBytes);
        sec(t.o_lt, locate_table_bytes(r));
        sec(t.o_lo, r16(4 * n));
    }
    CHECK(img.v.size() == at);
    return img.v.size();
}

// Grouped launches as run_rs_mixed builds them: every launch's tables in one
// image, the field block once behind them; or, with multi, one launch over
// every group.  Returns the image's size.
static size_t grouped(const std::vector<std::vector<Obj>>& groups, RsPass pass, bool multi) {
    std::vector<RsTable> ts;
    std::vector<Launch> ls;
    const uint64_t m_tile = tile_of(int(kMultiR));
    if (multi) {
        ts.push_back(RsTable::grouped(0, 0, 0, kMultiR, m_tile, pass, true));
        ls.push_back(Launch{{}, kMultiR, m_tile, true, true, true, pass});
    }
    for (const auto& g : groups) {
        const uint64_t tile = tile_of(g[0].r);
        uint64_t sum_k = 0, n_tiles = 0;
        for (const Obj& ob : g) sum_k += uint64_t(ob.k), n_tiles += tiles(ob.S, tile);
        if (multi) {
            ts[0].n_obj += g.size(), ts[0].n_in += sum_k, ts[0].n_list += n_tiles;
        } else {
            ts.push_back(RsTable::grouped(g.size(), sum_k, n_tiles, uint32_t(g[0].r), tile, pass));
            ls.push_back(Launch{{}, uint32_t(g[0].r), tile, true, false, true, pass});
            if (pass == kRsLocate)
                for (const Obj& ob : g) ts.back().locate_k(ob.k);
        }
        for (const Obj& ob : g) ls.back().objs.push_back(&ob);
    }
    RsImage img;
    for (RsTable& t : ts) t.lay(img, false);
    const size_t o_lf = pass == kRsLocate ? img.add(kLocateFieldBytes) : 0;
    for (RsTable& t : ts) t.o_lf = o_lf;
    if (pass == kRsLocate) CHECK(rs_locate_fill(img.data(), ts.data(), ts.size(), fake_table) == 0);
    for (size_t i = 0; i < groups.size(); ++i)
        for (const Obj& ob : groups[i]) ts[multi ? 0 : i].put(img.data(), ob.view(), ob.k, ob.r, ob.S);
    size_t at = 0;  // sections in order, each at its 16-byte-rounded size
    auto sec = [&at](size_t off, size_t bytes) {
        CHECK(off == at);
        at += bytes;
    };
    for (size_t i = 0; i < ts.size(); ++i) {
        const RsTable& t = ts[i];
        const RsArgs a = t.args(img.data());
        check_sections(ls[i], a);
        check_walk(ls[i], a);
        std::set<int> ks;
        for (const Obj* ob : ls[i].objs) ks.insert(ob->k);
        const uint64_t n = t.n_obj;
        sec(t.o_in, r16(8 * t.n_in));
        sec(t.o_out, r16(8 * n * t.r));
        sec(t.o_inlen, r16(8 * t.n_in));
        sec(t.o_outlen, r16(8 * n * t.r));
        sec(t.o_coef, r16(4 * n));
        sec(t.o_list, 16 * t.n_list);
        if (pass != kRsStore) sec(t.o_res, r16(8 * n));
        if (pass != kRsLocate) continue;
        sec(t.o_lt, ks.size() * locate_table_bytes(int(t.r)));  // one table per distinct k
        sec(t.o_lo, r16(4 * n));
        std::set<uint32_t> offs;
        for (size_t o = 0; o < n; ++o) offs.insert(a.loc_off[o]);
        CHECK(offs.size() == ks.size());
        uint8_t f[kLocateFieldBytes];
        locate_field_tables(f);
        CHECK(a.loc_field == reinterpret_cast<const uint8_t*>(img.data() + o_lf) && !std::memcmp(a.loc_field, f, sizeof f));
    }
    if (pass == kRsLocate) sec(o_lf, kLocateFieldBytes);  // the field block once, last
    CHECK(img.v.size() == at);
    return img.v.size();
}

// ---- the mixed-call plan -------------------------------------------------------
using Groups = std::map<int, std::vector<RsMixedObject>>;
static void add(Groups& g, const Obj& ob) { g[ob.r].push_back(RsMixedObject{ob.k, ob.S, ob.view()}); }
static RsMixedPlan plan(const Groups& g, bool multi_on = true, bool checked = false) {
    return rs_plan_mixed(g, tile_of, tile_of(int(kMultiR)), multi_on, checked);
}
// Every object of the call in exactly one launch.
static void check_partition(const Groups& g, const RsMixedPlan& p) {
    std::multiset<const void*> in, got;
    for (const auto& kv : g)
        if (kv.first != 0)
            for (const RsMixedObject& ob : kv.second) in.insert(ob.o.in);
    for (const auto& gr : p.grouped)
        for (const RsMixedObject& ob : gr.objs) got.insert(ob.o.in);
    for (const auto& u : p.rest)
        for (const RsObject& ob : u.objs) got.insert(ob.in);
    CHECK(in == got);
}

int main() {
    // ---- uniform ----
    for (uint64_t S : {uint64_t(1), uint64_t(16384), uint64_t(16385)}) {
        const std::vector<Obj> objs{Obj(4, 2, S), Obj(4, 2, S), Obj(4, 2, S)};
        const size_t bytes = uniform(objs, 4, 2, S);
        CHECK(bytes == 2 * r16(8 * 12) + 2 * r16(8 * 6) + r16(4 * 3));  // aligned: no edge list
        std::vector<Obj> v{Obj(4, 2, S, kRsVerify), Obj(4, 2, S, kRsVerify)};
        uniform(v, 4, 2, S, kRsVerify);
        std::vector<Obj> lo{Obj(4, 2, S, kRsLocate), Obj(4, 2, S, kRsLocate)};
        uniform(lo, 4, 2, S, kRsLocate);
    }
    {  // r = 9 at the 8 192-byte tile: r_total 9, row blocks 8 + 1 over one table set
        const std::vector<Obj> objs{Obj(4, 9, 20000), Obj(4, 9, 20000), Obj(4, 9, 20000)};
        uniform(objs, 4, 9, 20000);
    }
    // ---- uniform, one pointer at +1: every (o << 32 | t) in order ----
    for (uint64_t S : {uint64_t(1), uint64_t(16384), uint64_t(16385)})
        for (int which : {0, 1}) {
            std::vector<Obj> objs{Obj(4, 2, S), Obj(4, 2, S), Obj(4, 2, S)};
            if (which == 0) objs[1].in[2] += 1;
            else objs[2].out[1] += 1;
            CHECK(!rs_aligned(objs[which + 1].view(), 4, 2) && rs_aligned(objs[0].view(), 4, 2));
            const size_t bytes = uniform(objs, 4, 2, S);
            CHECK(bytes == 2 * r16(8 * 12) + 2 * r16(8 * 6) + r16(4 * 3) + r16(8 * 3 * tiles(S, 16384)));
        }
    // ---- grouped: r = 2, k in {1, 4, 10}, S in {1, 16 384, 49 153} ----
    {
        std::vector<Obj> g;
        for (int k : {1, 4, 10})
            for (uint64_t S : {uint64_t(1), uint64_t(16384), uint64_t(49153)}) g.push_back(Obj(k, 2, S));
        const size_t bytes = grouped({g}, kRsStore, false);
        const uint64_t n_in = 3 * (1 + 4 + 10), n_t = 3 * (1 + 1 + 4);
        CHECK(bytes == 2 * r16(8 * n_in) + 2 * r16(8 * 9 * 2) + r16(4 * 9) + 16 * n_t);
    }
    // ---- grouped verify and locate: r = 2, two distinct k; and two launches in one image ----
    for (RsPass pass : {kRsVerify, kRsLocate}) {
        std::vector<Obj> g, h;
        for (int k : {4, 10, 4, 10, 10}) g.push_back(Obj(k, 2, 16385, pass));
        grouped({g}, pass, false);
        for (int k : {3, 3, 5}) h.push_back(Obj(k, 5, 8193, pass));
        grouped({g, h}, pass, false);
    }
    {  // a table the caller cannot build fails the fill with its status
        RsTable t = RsTable::grouped(1, 4, 1, 2, 16384, kRsLocate);
        t.locate_k(4);
        RsImage img;
        t.lay(img, true);
        CHECK(rs_locate_fill(img.data(), &t, 1, [](int, int, uint8_t*) { return 7; }) == 7);
    }
    // ---- multi-r: groups r = 1, 2, 4 with mixed k ----
    {
        std::vector<std::vector<Obj>> gs(3);
        for (int k : {1, 4}) gs[0].push_back(Obj(k, 1, 16385));
        for (int k : {10, 2, 4}) gs[1].push_back(Obj(k, 2, 1));
        for (int k : {8, 3}) gs[2].push_back(Obj(k, 4, 49153));
        const size_t bytes = grouped(gs, kRsStore, true);
        const uint64_t n_in = 5 + 16 + 11, n_t = 2 * 2 + 3 + 2 * 4;
        CHECK(bytes == 2 * r16(8 * n_in) + 2 * r16(8 * 7 * kMultiR) + r16(4 * 7) + 16 * n_t);
        grouped(gs, kRsStore, false);  // the same groups, one launch per r
    }

    // ---- the plan, no tables ----
    {  // a lone uniform aligned group: one uniform launch
        Groups g;
        const std::vector<Obj> objs{Obj(4, 2, 1 << 20), Obj(4, 2, 1 << 20), Obj(4, 2, 1 << 20)};
        for (const Obj& ob : objs) add(g, ob);
        const RsMixedPlan p = plan(g);
        CHECK(p.grouped.empty() && p.rest.size() == 1 && !p.multi);
        CHECK(p.rest[0].r == 2 && p.rest[0].k == 4 && p.rest[0].shard_size == (1 << 20) && p.rest[0].objs.size() == 3);
        check_partition(g, p);
    }
    {  // ... with one unaligned object: the aligned ones grouped, that one to rest
        Groups g;
        std::vector<Obj> objs{Obj(4, 2, 1 << 20), Obj(4, 2, 1 << 20), Obj(4, 2, 1 << 20)};
        objs[1].out[0] += 1;
        for (const Obj& ob : objs) add(g, ob);
        const RsMixedPlan p = plan(g);
        CHECK(p.grouped.size() == 1 && p.grouped[0].objs.size() == 2 && p.grouped[0].r == 2);
        CHECK(p.grouped[0].sum_k == 8 && p.grouped[0].n_tiles == 128 && p.grouped[0].tile == 16384);
        CHECK(p.rest.size() == 1 && p.rest[0].objs.size() == 1 && p.rest[0].objs[0].out == objs[1].out.data());
        check_partition(g, p);
    }
    {  // r = 9 always goes to rest, beside a grouped r = 2; an r = 0 or empty group is nothing
        Groups g;
        const std::vector<Obj> objs{Obj(4, 9, 4096), Obj(5, 9, 4096), Obj(4, 2, 4096), Obj(5, 2, 4096)};
        for (const Obj& ob : objs) add(g, ob);
        g[0].push_back(RsMixedObject{4, 4096, objs[0].view()});
        g[3];
        const RsMixedPlan p = plan(g);
        CHECK(p.grouped.size() == 1 && p.grouped[0].r == 2 && p.rest.size() == 2 && !p.multi);
        CHECK(p.rest[0].r == 9 && p.rest[0].k == 4 && p.rest[1].r == 9 && p.rest[1].k == 5);
        check_partition(g, p);
    }
    {  // two (k, S) classes in rest keep first-appearance order, per r in map order
        Groups g;
        std::vector<Obj> objs{Obj(10, 3, 777), Obj(4, 3, 777), Obj(10, 3, 777), Obj(4, 3, 778), Obj(4, 3, 777), Obj(6, 1, 5)};
        for (Obj& ob : objs) ob.in[0] += 1;  // all unaligned
        for (const Obj& ob : objs) add(g, ob);
        const RsMixedPlan p = plan(g);
        CHECK(p.grouped.empty() && p.rest.size() == 4);
        CHECK(p.rest[0].r == 1 && p.rest[0].k == 6 && p.rest[0].shard_size == 5);
        CHECK(p.rest[1].r == 3 && p.rest[1].k == 10 && p.rest[1].shard_size == 777 && p.rest[1].objs.size() == 2);
        CHECK(p.rest[2].r == 3 && p.rest[2].k == 4 && p.rest[2].shard_size == 777 && p.rest[2].objs.size() == 2);
        CHECK(p.rest[3].r == 3 && p.rest[3].k == 4 && p.rest[3].shard_size == 778 && p.rest[3].objs.size() == 1);
        CHECK(p.rest[1].objs[0].in == objs[0].in.data() && p.rest[1].objs[1].in == objs[2].in.data());
        check_partition(g, p);
    }
    {  // the multi-r verdict
        const std::vector<Obj> objs{Obj(4, 2, 4096), Obj(5, 2, 100), Obj(8, 4, 4096), Obj(3, 5, 4096)};
        Groups g24, g25;
        for (int i : {0, 1, 2}) add(g24, objs[size_t(i)]);
        for (int i : {0, 1, 3}) add(g25, objs[size_t(i)]);
        const RsMixedPlan p = plan(g24);
        CHECK(p.grouped.size() == 2 && p.rest.empty() && p.multi);
        CHECK(p.m_obj == 3 && p.m_k == 17 && p.m_tiles == 3);
        CHECK(plan(g25).grouped.size() == 2 && !plan(g25).multi);  // r = 5: beyond kMultiR, another tile
        CHECK(plan(g24, true, true).grouped.size() == 2 && !plan(g24, true, true).multi);  // a verify / locate
        CHECK(plan(g24, false).grouped.size() == 2 && !plan(g24, false).multi);            // switched off
        Groups g2;  // one grouped launch is not multi
        for (int i : {0, 1}) add(g2, objs[size_t(i)]);
        CHECK(plan(g2).grouped.size() == 1 && !plan(g2).multi);
    }
    {  // RsTileRec's 32-bit tile index: exactly 2^32 tiles of 16 384 bytes fit, one more does not
        const uint64_t half = uint64_t(1) << 45;
        for (uint64_t extra : {uint64_t(0), uint64_t(1)}) {
            Groups g;
            const std::vector<Obj> objs{Obj(1, 2, half), Obj(2, 2, half + extra)};
            for (const Obj& ob : objs) add(g, ob);
            const RsMixedPlan p = plan(g);
            if (!extra) CHECK(p.grouped.size() == 1 && p.grouped[0].n_tiles == (uint64_t(1) << 32) && p.rest.empty());
            else CHECK(p.grouped.empty() && p.rest.size() == 2 && p.rest[0].k == 1 && p.rest[1].k == 2);
            check_partition(g, p);
        }
    }
    if (fails) return 1;
    std::printf("rs plan ok\n");
    return 0;
}
